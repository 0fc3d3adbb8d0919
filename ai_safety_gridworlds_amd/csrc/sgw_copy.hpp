// sgw_copy.hpp -- sgw_copy_envs: env dst_idx[i] of one engine becomes a bit-exact copy of env src_idx[i] of another (or of the
// same) engine -- every state word, and the env's row of every requested output -- in ONE launch.  Pure data movement: no
// family code, no LDS, no scratch.
//
// The per-item logic is plain __host__ __device__ C++: tests/host_shim/copy_check.cpp compiles this file for the host with the
// sanitizers and walks the same grid the kernel runs (copy_item over every wave and lane).  The kernel at the end is compiled
// by hipcc only.
//
// Work mapping (one wave = 64 lanes, 4 waves per workgroup):
//   state : wave (c, p) moves word pair p of the pairs 64 c .. 64 c + 63, a lane per pair of envs: 16 bytes per lane through
//           state_index, so identity and contiguous index lists are 1 KiB coalesced per wave on both sides
//   rows  : per output plane the lanes of a wave cooperate along rows: 2^k lanes per row (16 bytes of the row each per pass),
//           64 >> k rows per wave, so a 1-byte row costs a lane and a 1156-byte row a whole wave
#pragma once

#include <stdint.h>

#include "sgw_common.hpp"

namespace sgw {

constexpr int COPY_PLANES = 20;        // the fields of struct sgw_out, in its order

struct alignas(16) CopyV16 { uint32_t x, y, z, w; };

struct CopyPlane {
  const uint8_t* src;                  // the [N_pad, row_bytes] buffers of the two engines
  uint8_t* dst;
  int row_bytes;
  int lane_shift;                      // 2^lane_shift lanes share a row
  long long wave_end;                  // waves of the plane list up to and including this plane
};

struct CopyArgs {
  const uint64_t* src_state;
  uint64_t* dst_state;
  const int32_t* src_idx;              // nullptr: i
  const int32_t* dst_idx;
  long long n;                         // pairs
  long long src_n, dst_n;              // n_envs of the two engines: a pair with an index outside is skipped
  int words;
  int same;                            // dst and src are one engine: a pair of equal indices is skipped
  int n_planes;
  long long state_waves;               // ceil(n / 64) * state_pairs(words)
  CopyPlane planes[COPY_PLANES];
};

// lanes that share a row of row_bytes bytes: the power of two that gives each lane one 16-byte piece, at most a wave
__host__ __device__ inline int copy_lane_shift(int row_bytes) {
  int s = 0;
  while (s < 6 && (16 << s) < row_bytes) ++s;
  return s;
}

// The pair (si, di) of item i, or false where it is skipped: an index outside its engine, or a copy onto itself
__host__ __device__ inline bool copy_resolve(const CopyArgs& a, long long i, long long& si, long long& di) {
  si = a.src_idx ? (long long)a.src_idx[i] : i;
  di = a.dst_idx ? (long long)a.dst_idx[i] : i;
  if (si < 0 || si >= a.src_n || di < 0 || di >= a.dst_n) return false;
  return !(a.same && si == di);
}

// State: words 2p and 2p + 1 of env si -> env di, as the 16 bytes one lane owns (with odd `words` the padding half of the
// last pair travels with it)
__host__ __device__ inline void copy_state_pair(const uint64_t* src, uint64_t* dst, int words, long long si, long long di, int p) {
  const CopyV16* s = reinterpret_cast<const CopyV16*>(src + state_index(2 * p, si, words));
  CopyV16* d = reinterpret_cast<CopyV16*>(dst + state_index(2 * p, di, words));
  *d = *s;
}

// One row: `lanes` lanes (this one is `lane`) copy bytes [0, n) from s to d, any alignment of either.  Where s and d agree
// mod 16 (mod 4) the body moves as naturally aligned 16-byte (4-byte) units and only the head up to the first aligned
// destination byte and the tail go byte by byte; rows whose alignments disagree go byte by byte.  No access is wider than its
// alignment, and no byte outside [d, d + n) is written.
__host__ __device__ inline void copy_row(const uint8_t* s, uint8_t* d, int n, int lane, int lanes) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(s), da = reinterpret_cast<uintptr_t>(d);
  const int unit = ((sa ^ da) & 15) == 0 ? 16 : ((sa ^ da) & 3) == 0 ? 4 : 1;
  int head = (int)((0 - da) & (uintptr_t)(unit - 1));
  if (head > n) head = n;
  const int body = unit == 1 ? 0 : (n - head) / unit;
  const int tail0 = head + body * unit;
  if (unit == 16) {
    const CopyV16* sv = reinterpret_cast<const CopyV16*>(s + head);
    CopyV16* dv = reinterpret_cast<CopyV16*>(d + head);
    for (int k = lane; k < body; k += lanes) dv[k] = sv[k];
  } else if (unit == 4) {
    const uint32_t* sv = reinterpret_cast<const uint32_t*>(s + head);
    uint32_t* dv = reinterpret_cast<uint32_t*>(d + head);
    for (int k = lane; k < body; k += lanes) dv[k] = sv[k];
  }
  for (int k = lane; k < head; k += lanes) d[k] = s[k];
  for (int k = tail0 + lane; k < n; k += lanes) d[k] = s[k];
}

// What lane `lane` of wave `wave` of the launch does (a launch has fewer than 2^31 waves: 32-bit division)
__host__ __device__ inline void copy_item(const CopyArgs& a, unsigned wave, int lane) {
  if (wave < a.state_waves) {
    const unsigned pairs = (unsigned)state_pairs(a.words);
    const unsigned c = wave / pairs;
    const int p = (int)(wave - c * pairs);
    const long long i = (long long)c * WAVE + lane;
    long long si, di;
    if (i < a.n && copy_resolve(a, i, si, di)) copy_state_pair(a.src_state, a.dst_state, a.words, si, di, p);
    return;
  }
  long long w = wave - a.state_waves, begin = 0;
  for (int q = 0; q < a.n_planes; ++q) {
    const CopyPlane& pl = a.planes[q];
    if (w < pl.wave_end) {
      const int sh = pl.lane_shift;
      const long long i = ((w - begin) << (6 - sh)) + (lane >> sh);
      long long si, di;
      if (i < a.n && copy_resolve(a, i, si, di))
        copy_row(pl.src + si * pl.row_bytes, pl.dst + di * pl.row_bytes, pl.row_bytes, lane & ((1 << sh) - 1), 1 << sh);
      return;
    }
    begin = pl.wave_end;
  }
}

// Waves of the whole launch; fills state_waves and the planes' lane_shift / wave_end from n, words and the planes' row_bytes
__host__ __device__ inline long long copy_plan(CopyArgs& a) {
  const long long chunks = (a.n + WAVE - 1) / WAVE;
  a.state_waves = chunks * state_pairs(a.words);
  long long end = 0;
  for (int q = 0; q < a.n_planes; ++q) {
    CopyPlane& pl = a.planes[q];
    pl.lane_shift = copy_lane_shift(pl.row_bytes);
    const long long rows_per_wave = WAVE >> pl.lane_shift;
    end += (a.n + rows_per_wave - 1) / rows_per_wave;
    pl.wave_end = end;
  }
  return a.state_waves + end;
}

constexpr int COPY_THREADS = 256;

#if !defined(SGW_COPY_HOST_ONLY)
__global__ void __launch_bounds__(COPY_THREADS) k_copy_envs(CopyArgs a, unsigned waves) {
  // (the wave number is wave-uniform: said so, the plane search and the pair split stay scalar)
  const unsigned wave = blockIdx.x * (COPY_THREADS / WAVE) + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave < waves) copy_item(a, wave, (int)(threadIdx.x & 63));
}
#endif

}  // namespace sgw
