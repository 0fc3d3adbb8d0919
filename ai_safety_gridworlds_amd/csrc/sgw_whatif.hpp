// sgw_whatif.hpp -- sgw_simulate_moves / sgw_fold_q_values: where each action of the action set would take an agent, WITHOUT
// playing it, and the reference's per-tile-type Q-value table built from that (SafetyEnvironmentMo.step(actions,
// q_value_per_action), safety_game_mo.py:810-857; AgentSafetySpriteMo.simulate_update, 1340-1379, 1442-1576).  The inputs are
// outputs of every step (board, agent_pos, agent_flags), so both kernels stand beside the step launch and change nothing of it.
//
// The rule of one (env, agent), whatif_moves below, ONE __host__ __device__ function (tests/host_shim/whatif_check.cpp compiles the
// same text for the host).  (r, c) is the agent's cell, d its action direction (Directions LEFT=0 RIGHT=1 UP=2 DOWN=3; read only when
// the env's action_direction_mode is 1 or 2), I its impassable characters.  carry = (r, c); for j = 0, 1, ..., NA-1 IN THAT ORDER
// (action = j: the spec's action_lo is 0, Actions NOOP=0 LEFT=1 RIGHT=2 UP=3 DOWN=4, turning actions 5..8):
//   absolute = j, or for a relative env and j in 1..4 the move seen from d (get_absolute_action, safety_game_mo_base.py:458-503)
//   motion   = LEFT (0,-1), RIGHT (0,+1), UP (-1,0), DOWN (+1,0); NOOP and the turning actions (0,0)
//   blocked[j] = motion != (0,0) and (the target is off the board or board[target] is in I)   (_check_motion, pycolab
//                prefab_parts/sprites.py:479-540: "moving nowhere is always fine", so j = 0 is never refused)
//   if not blocked[j]: carry = target                 <- the reference's quirk: _simulated_position is written on success only,
//   target_pos[j] = carry; target_tile[j] = board[carry]  so a refused action reports the cell of the last action that passed
// An agent_pos outside the board (the engine never writes one) reports itself, tile 0 and blocked = 1 for every action.
//
// The fold, whatif_fold below, for one (env, agent, d) and every l < L: over the j with target_tile[j] == tile_chars[l], in order
// of j, sum = q[first j][d], then sum = sum + q[j][d] (one IEEE double addition each), table[l][d] = sum / (double)count, seen[l]
// = 1; a tile type no action reached keeps its table row and its seen byte (q_value_per_tiletype.update, np.mean(list, axis=0)).
//
// Work mapping of k_simulate_moves, as k_policy_act: a workgroup takes 64 consecutive envs, whose board rows are contiguous and
// come into LDS as 16-byte loads (whole chunks inside the rows n < N, then single bytes: no byte of a row n >= N is read); lane q
// evaluates pair (env = q / A, agent = q % A) with its NA results in registers (instantiated per NA, nothing indexed at run time)
// and leaves them in LDS; the group then stores its contiguous slice of each output with consecutive lanes on consecutive bytes.
// k_fold_q_values: one lane per (env, agent, d): its NA tile bytes and NA q values in registers; lanes d = 0 .. D-1 of a pair
// read and write neighbouring doubles.  Every cell has one writer: no atomics.  Plain C++ stores only.
// LDS (dynamic) of k_simulate_moves: round16(64 * H*W) | pos [pairs * NA * 2] | tile [pairs * NA] | blocked [pairs * NA].
#pragma once

#include <stdint.h>

#include "sgw_common.hpp"

namespace sgw {

constexpr int WHATIF_MAX_ACTIONS = 9;        // NOOP, four moves, four turning actions: simulate_update raises beyond (MO:1376-1377)
constexpr int WHATIF_ENVS = 64;              // envs per workgroup: a multiple of 16 keeps the group's first board byte 16-byte aligned
constexpr int WHATIF_THREADS_MAX = 256;
constexpr int WHATIF_MAX_TILES = 64;

struct WhatifArgs {
  const uint8_t* board;          // [n, H*W]
  const uint8_t* agent_pos;      // [n, A, 2]
  const uint8_t* agent_flags;    // [n, A] or nullptr (direction UP)
  uint8_t* target_pos;           // [n, A, NA, 2] or nullptr
  uint8_t* target_tile;          // [n, A, NA] or nullptr
  uint8_t* blocked;              // [n, A, NA] or nullptr
  unsigned long long impassable[SGW_MAX_AGENTS];   // up to 8 characters per agent, one per byte, 0 = unused
  long long n;
  int H, W, A, n_actions, relative;
};

struct FoldArgs {
  const uint8_t* target_tile;    // [n, A, NA]
  const double* q;               // [n, A, NA, D]
  const uint8_t* tile_chars;     // [L]
  double* table;                 // [n, A, L, D]
  uint8_t* seen;                 // [n, A, L] or nullptr
  long long n;
  int A, n_actions, D, L;
};

__host__ __device__ inline bool whatif_impassable(unsigned long long set, int ch) {
  bool hit = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = (int)((set >> (8 * k)) & 0xff);
    hit |= (c != 0) & (c == ch);
  }
  return hit;
}

// pos[2j], pos[2j+1] = (row, col) reported for action j; tile[j]; blk[j]
template <int NA>
__host__ __device__ inline void whatif_moves(const uint8_t* board, int H, int W, int row, int col, int dir, bool relative,
                                             unsigned long long impassable, uint8_t (&pos)[2 * NA], uint8_t (&tile)[NA],
                                             uint8_t (&blk)[NA]) {
  const bool on_board = (row < H) & (col < W);
  int cr = row, cc = col;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    int absolute = j;
    if (relative && j >= 1 && j <= 4) {
      // Directions LEFT=0 RIGHT=1 UP=2 DOWN=3; the move named LEFT / RIGHT / UP / DOWN seen from `dir` (MO base:458-503)
      const int back = dir ^ 1;
      const int left = dir == 2 ? 0 : (dir == 3 ? 1 : (dir == 0 ? 3 : 2));
      const int d = j == 3 ? dir : (j == 4 ? back : (j == 1 ? left : (left ^ 1)));
      absolute = d + 1;
    }
    const int dr = (absolute == 4) - (absolute == 3), dc = (absolute == 2) - (absolute == 1);
    const int nr = row + dr, nc = col + dc;
    const bool inside = (nr >= 0) & (nr < H) & (nc >= 0) & (nc < W);
    const int ch = (inside & on_board) ? (int)board[nr * W + nc] : 0;
    const bool moving = (dr | dc) != 0;
    const bool refused = !on_board | (moving & (!inside | whatif_impassable(impassable, ch)));
    cr = refused ? cr : nr; cc = refused ? cc : nc;
    pos[2 * j] = (uint8_t)cr; pos[2 * j + 1] = (uint8_t)cc;
    tile[j] = on_board ? board[cr * W + cc] : (uint8_t)0;
    blk[j] = refused ? 1 : 0;
  }
}

// one (env, agent, d): tile[NA] the pair's target tiles, q the pair's [NA][D] block offset to column d, table the pair's [L][D]
// block offset to column d, seen the pair's [L] bytes (written when first_dim, i.e. by the pair's lane d == 0) or nullptr
template <int NA>
__host__ __device__ inline void whatif_fold(const uint8_t* tile, const double* q, int D, const uint8_t* tile_chars, int L,
                                            double* table, uint8_t* seen, bool first_dim) {
  uint8_t t[NA];
  double v[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) { t[j] = tile[j]; v[j] = q[(long long)j * D]; }
  for (int l = 0; l < L; ++l) {
    const uint8_t c = tile_chars[l];
    int count = 0;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const bool hit = t[j] == c;
      sum = hit ? (count == 0 ? v[j] : sum + v[j]) : sum;
      count += hit ? 1 : 0;
    }
    if (count > 0) {
      table[(long long)l * D] = sum / (double)count;
      if (seen && first_dim) seen[l] = 1;
    }
  }
}

template <int NA>
__device__ __forceinline__ void simulate_moves_block(const WhatifArgs& a, uint8_t* lds) {
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const int HW = a.H * a.W;
  const long long env0 = (long long)blockIdx.x * WHATIF_ENVS;
  const long long left = a.n - env0;
  const int nrow = left < WHATIF_ENVS ? (int)left : WHATIF_ENVS;                     // a ragged last group takes only its own rows
  const int nbytes = nrow * HW;
  const uint8_t* src = a.board + env0 * HW;                                          // 16-byte aligned: WHATIF_ENVS % 16 == 0
  for (int i = tid * 16; i + 16 <= nbytes; i += nthr * 16)
    *reinterpret_cast<uint4*>(lds + i) = *reinterpret_cast<const uint4*>(src + i);
  for (int i = (nbytes & ~15) + tid; i < nbytes; i += nthr) lds[i] = src[i];
  __syncthreads();
  const int pairs = nrow * a.A;
  uint8_t* o_pos = lds + (WHATIF_ENVS * HW + 15) / 16 * 16;
  uint8_t* o_tile = o_pos + WHATIF_ENVS * a.A * NA * 2;
  uint8_t* o_blk = o_tile + WHATIF_ENVS * a.A * NA;
  for (int q = tid; q < pairs; q += nthr) {
    const int env = q / a.A, ag = q - env * a.A;
    const long long pair = env0 * a.A + q;
    const int row = a.agent_pos[pair * 2], col = a.agent_pos[pair * 2 + 1];
    const int dir = a.agent_flags ? (a.agent_flags[pair] >> 1) & 3 : 2;
    static_assert(SGW_MAX_AGENTS == 4, "the impassable sets are selected among four agents");
    const unsigned long long imp = ag == 0 ? a.impassable[0] : ag == 1 ? a.impassable[1] : ag == 2 ? a.impassable[2] : a.impassable[3];
    uint8_t pos[2 * NA], tile[NA], blk[NA];
    whatif_moves<NA>(lds + env * HW, a.H, a.W, row, col, dir, a.relative != 0, imp, pos, tile, blk);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      o_pos[(q * NA + j) * 2] = pos[2 * j]; o_pos[(q * NA + j) * 2 + 1] = pos[2 * j + 1];
      o_tile[q * NA + j] = tile[j];
      o_blk[q * NA + j] = blk[j];
    }
  }
  __syncthreads();
  const long long out0 = env0 * a.A * NA;                                            // the group's first (pair, action)
  const int items = pairs * NA;
  if (a.target_pos) for (int i = tid; i < items * 2; i += nthr) a.target_pos[out0 * 2 + i] = o_pos[i];
  if (a.target_tile) for (int i = tid; i < items; i += nthr) a.target_tile[out0 + i] = o_tile[i];
  if (a.blocked) for (int i = tid; i < items; i += nthr) a.blocked[out0 + i] = o_blk[i];
}

#define SGW_WHATIF_CASES(M) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9)

__global__ __launch_bounds__(WHATIF_THREADS_MAX) void k_simulate_moves(WhatifArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t whatif_lds[];
  switch (a.n_actions) {                                                             // uniform
#define SGW_WHATIF_CASE(NA) case NA: simulate_moves_block<NA>(a, whatif_lds); break;
    SGW_WHATIF_CASES(SGW_WHATIF_CASE)
#undef SGW_WHATIF_CASE
    default: break;
  }
}

template <int NA>
__device__ __forceinline__ void fold_q_values_lane(const FoldArgs& a) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n * a.A * a.D) return;
  const long long pair = i / a.D;
  const int d = (int)(i - pair * a.D);
  whatif_fold<NA>(a.target_tile + pair * NA, a.q + pair * NA * a.D + d, a.D, a.tile_chars, a.L, a.table + pair * a.L * a.D + d,
                  a.seen ? a.seen + pair * a.L : nullptr, d == 0);
}

__global__ __launch_bounds__(WHATIF_THREADS_MAX) void k_fold_q_values(FoldArgs a) {
  switch (a.n_actions) {                                                             // uniform
#define SGW_WHATIF_CASE(NA) case NA: fold_q_values_lane<NA>(a); break;
    SGW_WHATIF_CASES(SGW_WHATIF_CASE)
#undef SGW_WHATIF_CASE
    default: break;
  }
}

}  // namespace sgw
