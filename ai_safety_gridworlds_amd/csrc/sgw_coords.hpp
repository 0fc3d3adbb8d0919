// sgw_coords.hpp -- object coordinates of byte planes: the set cells of every plane as a padded (count, coordinate list) pair
// (info_observation_coordinates, safety_game_mo.py:422-457 / safety_game_moma.py:583-603; the agent-relative form
// info_agent_observation_coordinates, safety_game_moma.py:528-580).  A stream compaction with np.argwhere's order.
//
// Mapping: a SEGMENT of S lanes takes one plane, S = the power of two >= ceil((cells + 3) / 4), at most a wave; a wave takes
// 64 / S planes at once (island's 6 x 8 board: S = 16, four planes per wave; firemaker's 17 x 17: a wave per plane, two passes).
// A lane loads the four cells of one ALIGNED dword of the plane (planes start at any byte: the dwords that hang over the plane's
// ends come in as single bytes, so no byte outside the plane is read) and reduces them to four bits.  One __ballot per byte
// position gives every lane the bits of the whole wave; masked to the lanes of its own segment below it, their population counts
// are the exclusive prefix of the lane -- no shuffle scan, no LDS, no atomics -- and masked to the whole segment they are the
// pass's total, which the running base carries to the next pass.  A set cell's rank addresses ONE 4-byte store of its
// coordinate pair; ranks >= cap and the entries past the count are never stored, so the store traffic follows the objects.
#pragma once
#include "sgw_common.hpp"       // div_recip

namespace sgw {

struct CoordGeom {
  int L, A;                            // planes per (env, agent); agents (1: the global form)
  int seg_shift, n_pass, cap;          // S = 1 << seg_shift lanes per plane; passes of 4 * S cells that cover the largest plane
  int cells[SGW_MAX_AGENTS], W[SGW_MAX_AGENTS], recip_W[SGW_MAX_AGENTS];     // a plane's cells and row length; ceil(2^32 / W) (0: W == 1)
  int off[SGW_MAX_AGENTS];             // byte offset of the agent's L planes in the env's row
  int own[SGW_MAX_AGENTS];             // the plane that holds the agent itself (-1: none)
  long long row_bytes;                 // bytes of one env's row of planes
};

template <class T> __device__ __forceinline__ T coords_pick(const T (&v)[SGW_MAX_AGENTS], int a) {    // (no dynamic index into the kernel arguments)
  return a == 0 ? v[0] : a == 1 ? v[1] : a == 2 ? v[2] : v[3];
}

// bit k = cell c0 + k of the plane is set; plane + c0 is dword-aligned, cells outside [0, cells) read as clear and are not loaded
__device__ __forceinline__ uint32_t coords_bits4(const uint8_t* plane, int c0, int cells) {
  uint32_t bits = 0;
  if (c0 >= 0 && c0 + 4 <= cells) {
    const uint32_t w = *reinterpret_cast<const uint32_t*>(plane + c0);
    bits = ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (c0 + k >= 0 && c0 + k < cells && plane[c0 + k]) bits |= 1u << k;
  }
  return bits;
}

__device__ __forceinline__ int coords_popc_below(uint64_t m) {      // set bits of m in the lanes below this one
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// REL = false: counts int32 [items], coords int16 [items, cap, 2] = (row, col); items = N * L planes of g.cells[0] bytes.
// REL = true: items = N * A * L; the centre (ay, ax) of an (env, agent) is the first set cell of the agent's own plane (each segment
// finds it for itself: one more read of a plane that is in L2, one ballot and a find-first per pass, instead of a barrier and a
// second role for one wave); coords = (x - ax, y - ay); no centre: every count of the (env, agent) is -1, nothing is stored.
template <bool REL>
__global__ __launch_bounds__(256) void k_plane_coords(const uint8_t* planes, unsigned items, const CoordGeom g, int* counts, int16_t* coords) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int S = 1 << g.seg_shift, sub = lane >> g.seg_shift, sl = lane & (S - 1), per_wave = WAVE >> g.seg_shift;
  const uint64_t segmask = (S == WAVE ? ~0ull : ((1ull << S) - 1)) << (sub * S);
  const unsigned n_waves = gridDim.x * (blockDim.x >> 6), wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const unsigned AL = (unsigned)(g.A * g.L), wave_loads = (items + per_wave - 1) / per_wave;
  for (unsigned wv = wave; wv < wave_loads; wv += n_waves) {       // uniform per wave: every lane reaches the ballots
    const unsigned it = wv * per_wave + sub;
    const bool live = it < items;
    const unsigned env = live ? it / AL : 0, r = live ? it - env * AL : 0;
    const int a = REL ? (int)(r / (unsigned)g.L) : 0, l = (int)(r - (unsigned)a * g.L);
    const int cells = live ? coords_pick(g.cells, a) : 0, W = coords_pick(g.W, a);
    const uint32_t recip = (uint32_t)coords_pick(g.recip_W, a);
    const uint8_t* block = planes + (size_t)env * g.row_bytes + coords_pick(g.off, a);
    int ar = 0, ac = 0;
    bool present = true;
    if (REL) {
      const int own = coords_pick(g.own, a);
      const uint8_t* mine = block + (size_t)(own < 0 ? 0 : own) * cells;
      const int m = (int)(reinterpret_cast<uintptr_t>(mine) & 3);
      const int own_cells = own < 0 ? 0 : cells;
      int centre = -1;
      for (int p = 0; p < g.n_pass; ++p) {
        const uint32_t bits = coords_bits4(mine, 4 * (p * S + sl) - m, own_cells);
        const uint64_t any = __ballot(bits != 0) & segmask;
        const int src = any ? __builtin_ctzll(any) : lane;             // the segment's first lane with a set cell
        const uint32_t fb = (uint32_t)__shfl((int)bits, src);
        if (centre < 0 && any) centre = 4 * (p * S + (src & (S - 1))) - m + __builtin_ctz(fb);
      }
      present = centre >= 0;
      if (present) { ar = (int)div_recip((uint32_t)centre, recip); ac = centre - ar * W; }
    }
    const uint8_t* plane = block + (size_t)l * cells;
    const int m = (int)(reinterpret_cast<uintptr_t>(plane) & 3);
    const int my_cells = present ? cells : 0;
    uint32_t* dst = reinterpret_cast<uint32_t*>(coords) + (size_t)it * g.cap;
    int base = 0;
    for (int p = 0; p < g.n_pass; ++p) {
      const int c0 = 4 * (p * S + sl) - m;
      const uint32_t bits = coords_bits4(plane, c0, my_cells);
      int rank = base;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint64_t b = __ballot((bits >> k) & 1u);
        rank += coords_popc_below(b & segmask);
        base += __popcll(b & segmask);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((bits >> k) & 1u) {
          if (rank < g.cap) {
            const int c = c0 + k, row = (int)div_recip((uint32_t)c, recip), col = c - row * W;
            const int first = REL ? col - ac : row, second = REL ? row - ar : col;
            dst[rank] = (uint32_t)(uint16_t)first | ((uint32_t)(uint16_t)second << 16);
          }
          ++rank;
        }
      }
    }
    if (live && sl == 0) counts[it] = present ? base : -1;
  }
}

}  // namespace sgw
