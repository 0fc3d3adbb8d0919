// sgw_learn.hpp -- sgw_policy_scores / sgw_policy_accumulate / sgw_policy_apply: what a table policy needs to LEARN on the device.
// The table is a Q-table that is linear in the one-hot observation (score[j] = Q(s, j)); with these three calls any rule of the
// form weights += lr * sum(coef * one-hot) is a chain of launches: rollout -> scores -> targets -> gradient sums -> update.
//
// The three element rules, each ONE __host__ __device__ function (tests/host_shim/learn_check.cpp compiles the same text for the
// host):
//   learn_scores_element   the score vector policy_choose computes (policy_score of sgw_policy.hpp: the same float32 additions in
//                          the same order), vmax = (double)score[first maximum], chosen = (double)score[j of the action played]
//   learn_quantise         x = coef * 2^frac_bits;  NaN -> 0;  |x| >= 2^31 - 1 -> +-(2^31 - 1);  else (int64)rint(x), ties to even
//   learn_apply_element    w = (float)((double)w + lr * ((double)acc * 2^-frac_bits)), every operation rounded on its own
//
// WHY FIXED POINT.  The gradient sums are INTEGERS: integer addition is associative, so every schedule of the 8 million additions
// into one bin (65 536 envs x 128 steps) gives the same bits, and two runs agree.  |q| < 2^31 and fewer than 2^32 transitions: no
// int64 sum wraps.  Float atomics would depend on the arrival order; a fixed float order would serialise the additions per bin.
//
// Work mapping of k_policy_accumulate.  A SLICE is (agent a, a range of R cells of its table); a workgroup belongs to one slice for
// its whole life and, with P == 1, keeps that slice's bins -- int64 [R][G][n_actions], and the agent's bias bins behind them -- in
// LDS.  The workgroups of a slice stride over the TILES (step t, group of E consecutive envs): the tile's observation rows are
// contiguous in O[t] and come into LDS as 16-byte loads exactly as k_policy_act stages them (no byte of a row n >= N is read); one
// lane per env of the tile quantises its coefficient and leaves (q, j, p) in LDS.  Then each WAVE walks transitions (wave w takes
// env w, w + waves, ...): q and j are uniform over the wave, lane l takes cells l, l + 64, ... of the range and adds q to bin
// (cell, code_of[o[cell]], j) with one LDS 64-bit integer add that returns nothing -- the 64 lanes of one instruction hit 64
// different bins (different cells), so nothing serialises on the wall code.  A transition with q == 0 costs one LDS read per wave.
// At the end the workgroup adds its NON-ZERO bins to the caller's accumulators with 64-bit integer global atomic adds, each
// workgroup starting at another bin so that the adds of one moment spread over the table.  Windows whose bins exceed the LDS
// budget (the 33 x 33 window of firemaker_ex_ma) are cut into several cell ranges: more slices, each re-reading the rows.
// P > 1 takes the simple path: the same walk, every add a global integer atomic on acc[p], no bins.
// LDS (dynamic): round16(E * row_bytes) | code_of [256] | q, j, p int32 [E] each | bins int64 [R * G * n_actions + n_actions].
#pragma once

#include <math.h>
#include <stdint.h>

#include "sgw_common.hpp"
#include "sgw_policy.hpp"

namespace sgw {

constexpr long long LEARN_Q_MAX = 2147483647LL;      // 2^31 - 1: the largest |q|

// ---- the element rules ----------------------------------------------------------------------------------------------------------
// known == false: the env's policy index is out of range -- +0.0 everywhere, no table is read.  j: the index of the action played
// (action - action_lo), anything outside 0 .. NA-1 (or no tape) gives chosen = +0.0.
template <int NA>
__host__ __device__ __forceinline__ void learn_scores_element(float (&score)[NA], double& vmax, double& chosen, const uint8_t* o, int C_a,
                                                              const uint8_t* code_of, bool known, const float* w, const float* b, int G, int j) {
  vmax = 0.0; chosen = 0.0;
  if (!known) {
#pragma unroll
    for (int k = 0; k < NA; ++k) score[k] = 0.0f;
    return;
  }
  policy_score<NA>(score, o, C_a, code_of, w, b, G);
  float top;
  policy_first_max<NA>(score, top);
  vmax = (double)top;
  float c = 0.0f;
#pragma unroll
  for (int k = 0; k < NA; ++k) c = j == k ? score[k] : c;                    // selects: the registers are never indexed at run time
  chosen = (double)c;
}

// scale = 2^frac_bits (exact): the product is exact unless it overflows to an infinity, which saturates
__host__ __device__ __forceinline__ long long learn_quantise(double coef, double scale) {
  const double x = coef * scale;
  if (x != x) return 0;
  if (x >= 2147483647.0) return LEARN_Q_MAX;
  if (x <= -2147483647.0) return -LEARN_Q_MAX;
  return (long long)rint(x);
}

// inv_scale = 2^-frac_bits (exact).  acc != 0 (an element with acc == 0 is not written at all: the caller checks)
__host__ __device__ __forceinline__ float learn_apply_element(float w, long long acc, double lr, double inv_scale) {
  const double g = (double)acc * inv_scale;
  const double step = lr * g;
  return (float)((double)w + step);
}

#ifndef SGW_LEARN_RULES_ONLY
// ---- sgw_policy_scores -----------------------------------------------------------------------------------------------------------
struct ScoreArgs {
  const uint8_t* obs0;           // O[0]: [>= n, row_bytes]
  const uint8_t* obs;            // O[1 .. T]: [T, obs_rows, row_bytes]
  const uint8_t* code_of;
  const float* weights;
  const float* bias;
  const int32_t* policy_of_env;
  const int8_t* actions;         // [T, n, A] or nullptr
  float* scores;                 // [T+1, n, A, n_actions] or nullptr
  double* vmax;                  // [T+1, n, A] or nullptr
  double* chosen;                // [T, n, A] or nullptr
  long long n, obs_rows, groups;
  int T, row_bytes, envs_per_block, A, P, G, C, n_actions, action_lo;
  int c_a[SGW_MAX_AGENTS], off_a[SGW_MAX_AGENTS];
};

// the rows of one (step, env group) into LDS: 16-byte chunks inside the rows n < N, then single bytes
__device__ __forceinline__ void learn_stage_rows(uint8_t* lds, const uint8_t* src, int nbytes, int tid, int nthr) {
  for (int i = tid * 16; i + 16 <= nbytes; i += nthr * 16)
    *reinterpret_cast<uint4*>(lds + i) = *reinterpret_cast<const uint4*>(src + i);
  for (int i = (nbytes & ~15) + tid; i < nbytes; i += nthr) lds[i] = src[i];
}

template <int NA>
__device__ __forceinline__ void policy_scores_block(const ScoreArgs& a, uint8_t* lds) {
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const long long s = (long long)blockIdx.x / a.groups, grp = (long long)blockIdx.x - s * a.groups;   // observation O[s], env group
  const long long env0 = grp * a.envs_per_block;
  const long long left = a.n - env0;
  const int nrow = left < a.envs_per_block ? (int)left : a.envs_per_block;
  const uint8_t* src = (s == 0 ? a.obs0 : a.obs + (s - 1) * a.obs_rows * a.row_bytes) + env0 * a.row_bytes;
  uint8_t* codes = lds + (a.envs_per_block * a.row_bytes + 15) / 16 * 16;
  learn_stage_rows(lds, src, nrow * a.row_bytes, tid, nthr);
  for (int i = tid; i < 256; i += nthr) codes[i] = a.code_of[i];
  __syncthreads();
  const bool played = a.chosen != nullptr && s < a.T;                                 // O[T] has no action
  for (int q = tid; q < nrow * a.A; q += nthr) {
    const int env = q / a.A, ag = q - env * a.A;
    const long long n = env0 + env;
    const int p = a.policy_of_env ? a.policy_of_env[n] : 0;
    const long long pair = (s * a.n + n) * a.A + ag;
    const float* w = nullptr;
    const float* b = nullptr;
    const bool known = p >= 0 && p < a.P;
    if (known) {
      const long long slice = (long long)p * a.A + ag;
      w = a.weights + slice * a.C * a.G * NA;
      b = a.bias ? a.bias + slice * NA : nullptr;
    }
    const int j = played ? (int)a.actions[pair] - a.action_lo : -1;
    float score[NA];
    double vmax, chosen;
    learn_scores_element<NA>(score, vmax, chosen, lds + env * a.row_bytes + policy_pick(a.off_a, ag), policy_pick(a.c_a, ag), codes, known, w, b, a.G, j);
    if (a.scores) {
#pragma unroll
      for (int k = 0; k < NA; ++k) a.scores[pair * NA + k] = score[k];
    }
    if (a.vmax) a.vmax[pair] = vmax;
    if (played) a.chosen[pair] = chosen;
  }
}

__global__ __launch_bounds__(POLICY_THREADS_MAX) void k_policy_scores(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t policy_lds[];
  switch (a.n_actions) {                                                             // uniform
#define SGW_SCORES_CASE(NA) case NA: policy_scores_block<NA>(a, policy_lds); break;
    SGW_SCORES_CASE(1) SGW_SCORES_CASE(2) SGW_SCORES_CASE(3) SGW_SCORES_CASE(4) SGW_SCORES_CASE(5) SGW_SCORES_CASE(6)
    SGW_SCORES_CASE(7) SGW_SCORES_CASE(8) SGW_SCORES_CASE(9) SGW_SCORES_CASE(10) SGW_SCORES_CASE(11) SGW_SCORES_CASE(12)
    SGW_SCORES_CASE(13) SGW_SCORES_CASE(14) SGW_SCORES_CASE(15) SGW_SCORES_CASE(16)
#undef SGW_SCORES_CASE
    default: break;
  }
}

// ---- sgw_policy_accumulate -------------------------------------------------------------------------------------------------------
constexpr int LEARN_THREADS = 256;
constexpr int LEARN_MAX_ROW_LDS = 32 * 1024;      // bytes of observation rows a workgroup stages
constexpr int LEARN_MAX_BIN_LDS = 24 * 1024;      // bytes of int64 bins a workgroup keeps (rows + bins + the rest < 64 KiB)
constexpr int LEARN_BLOCKS = 1024;                // workgroups of a launch, about: 4 per CU

struct AccArgs {
  const uint8_t* obs0;
  const uint8_t* obs;
  const uint8_t* code_of;
  const int32_t* policy_of_env;
  const int8_t* actions;               // [T, n, A]
  const double* coef;                  // [T, n, A]
  unsigned long long* acc_w;           // int64 [P, A, C, G, n_actions], added to as two's complement
  unsigned long long* acc_b;           // int64 [P, A, n_actions] or nullptr
  long long n, obs_rows, groups, tiles;
  double scale;                        // 2^frac_bits
  int row_bytes, envs_per_block, A, P, G, C, n_actions, action_lo;
  int R;                               // cells per slice
  int blocks_per_slice;
  int c_a[SGW_MAX_AGENTS], off_a[SGW_MAX_AGENTS];
  int slice0[SGW_MAX_AGENTS];          // the first slice of agent a
};

__device__ __forceinline__ void learn_lds_add(unsigned long long* bin, long long q) {
  __hip_atomic_fetch_add(bin, (unsigned long long)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void learn_global_add(unsigned long long* bin, unsigned long long q) {
  __hip_atomic_fetch_add(bin, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(LEARN_THREADS) void k_policy_accumulate(AccArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t learn_lds[];
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const int E = a.envs_per_block, NA = a.n_actions;
  uint8_t* codes = learn_lds + (E * a.row_bytes + 15) / 16 * 16;
  int32_t* qs = reinterpret_cast<int32_t*>(codes + 256);
  int32_t* js = qs + E;
  int32_t* ps = js + E;
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(ps + E);        // 8-byte aligned: E is a multiple of 16
  const int slice = (int)blockIdx.x / a.blocks_per_slice, first = (int)blockIdx.x - slice * a.blocks_per_slice;
  static_assert(SGW_MAX_AGENTS == 4, "the slice table is searched by three compares");
  const int ag = (a.A > 3 && slice >= a.slice0[3]) ? 3 : (a.A > 2 && slice >= a.slice0[2]) ? 2 : (a.A > 1 && slice >= a.slice0[1]) ? 1 : 0;
  const int chunk = slice - policy_pick(a.slice0, ag);
  const int C_a = policy_pick(a.c_a, ag), off = policy_pick(a.off_a, ag);
  const int c0 = chunk * a.R;
  const int cn = C_a - c0 < a.R ? (C_a - c0 > 0 ? C_a - c0 : 0) : a.R;               // cells of this slice (0: an agent without a window)
  const bool in_lds = a.P == 1;
  const bool with_bias = chunk == 0 && a.acc_b != nullptr;
  const int nbins = cn * a.G * NA;
  unsigned long long* bias_bins = bins + a.R * a.G * NA;
  if (in_lds)
    for (int i = tid; i < a.R * a.G * NA + NA; i += nthr) bins[i] = 0;
  for (int i = tid; i < 256; i += nthr) codes[i] = a.code_of[i];
  const int wave = tid >> 6, lane = tid & 63, waves = nthr >> 6;
  for (long long tile = first; tile < a.tiles; tile += a.blocks_per_slice) {
    const long long t = tile / a.groups, grp = tile - t * a.groups;
    const long long env0 = grp * E;
    const long long left = a.n - env0;
    const int nrow = left < E ? (int)left : E;
    const uint8_t* src = (t == 0 ? a.obs0 : a.obs + (t - 1) * a.obs_rows * a.row_bytes) + env0 * a.row_bytes;
    __syncthreads();                                                                 // the walk over the previous tile is over
    learn_stage_rows(learn_lds, src, nrow * a.row_bytes, tid, nthr);
    for (int i = tid; i < nrow; i += nthr) {
      const long long n = env0 + i, pair = (t * a.n + n) * a.A + ag;
      const int p = a.policy_of_env ? a.policy_of_env[n] : 0;
      const int j = (int)a.actions[pair] - a.action_lo;
      const long long q = learn_quantise(a.coef[pair], a.scale);
      const bool ok = p >= 0 && p < a.P && j >= 0 && j < NA;
      qs[i] = ok ? (int32_t)q : 0; js[i] = ok ? j : 0; ps[i] = ok ? p : 0;
    }
    __syncthreads();
    for (int i = wave; i < nrow; i += waves) {                                       // q, j, p: uniform over the wave
      const long long q = qs[i];
      if (q == 0) continue;
      const int j = js[i];
      const uint8_t* o = learn_lds + i * a.row_bytes + off + c0;
      if (in_lds) {
        if (with_bias && lane == 0) learn_lds_add(bias_bins + j, q);
        for (int c = lane; c < cn; c += 64) learn_lds_add(bins + (c * a.G + (int)codes[o[c]]) * NA + j, q);
      } else {
        const long long slice_p = (long long)ps[i] * a.A + ag;
        if (with_bias && lane == 0) learn_global_add(a.acc_b + slice_p * NA + j, (unsigned long long)q);
        unsigned long long* table = a.acc_w + (slice_p * a.C + c0) * a.G * NA;
        for (int c = lane; c < cn; c += 64) learn_global_add(table + (c * a.G + (int)codes[o[c]]) * NA + j, (unsigned long long)q);
      }
    }
  }
  if (!in_lds) return;                                                               // uniform
  __syncthreads();
  unsigned long long* table = a.acc_w + ((long long)ag * a.C + c0) * a.G * NA;       // p == 0
  int at = nbins > 0 ? (int)(((unsigned)first * 2039u + (unsigned)tid) % (unsigned)nbins) : 0;   // each workgroup starts at another bin
  const int stride = nthr % (nbins > 0 ? nbins : 1);
  for (int i = tid; i < nbins; i += nthr) {
    const unsigned long long v = bins[at];
    if (v != 0) learn_global_add(table + at, v);
    at += stride;
    if (at >= nbins) at -= nbins;
  }
  if (with_bias && tid < NA) {
    const unsigned long long v = bias_bins[tid];
    if (v != 0) learn_global_add(a.acc_b + (long long)ag * NA + tid, v);
  }
}

// ---- sgw_policy_apply ------------------------------------------------------------------------------------------------------------
struct ApplyArgs {
  float* weights;
  float* bias;
  long long* acc_w;
  long long* acc_b;
  long long n_w, n_b;                  // elements of weights; of bias (0: the bias is not updated)
  double lr, inv_scale;
  int clear;
};

__global__ __launch_bounds__(LEARN_THREADS) void k_policy_apply(ApplyArgs a) {
  const long long total = a.n_w + a.n_b, step = (long long)gridDim.x * LEARN_THREADS;
  for (long long i = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x; i < total; i += step) {
    const bool is_w = i < a.n_w;
    float* w = is_w ? a.weights + i : a.bias + (i - a.n_w);
    long long* acc = is_w ? a.acc_w + i : a.acc_b + (i - a.n_w);
    const long long v = *acc;
    if (v == 0) continue;                                                            // the element's bits stay
    *w = learn_apply_element(*w, v, a.lr, a.inv_scale);
    if (a.clear) *acc = 0;
  }
}
#endif  // SGW_LEARN_RULES_ONLY

}  // namespace sgw
