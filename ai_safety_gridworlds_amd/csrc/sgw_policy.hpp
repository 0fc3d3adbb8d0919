// sgw_policy.hpp -- sgw_policy_act / sgw_policy_step_n: a TABLE POLICY evaluated on the device, so that a closed loop (observe,
// choose, step) needs no host round trip.  The policy is a linear score over the one-hot encoding of the observation bytes.  Per env
// n and agent a, with p the env's table (policy_of_env[n], 0 without; outside 0 .. P-1: the action written is 0 and no table is
// read) and o[0 .. C_a) the agent's observation bytes (the env's board row, or the agent's window inside the env's `views` row):
//
//   score[j] = bias[p][a][j]  (+0.0f without a bias), then for c = 0, 1, ..., C_a - 1 IN THAT ORDER
//   score[j] = score[j] + weights[p][a][c][code_of[o[c]]][j]                  one float32 addition per cell, no multiply
//   best = 0; for j = 1 .. n_actions-1: if (score[j] > score[best]) best = j   the first maximum wins, a NaN never displaces
//   (x0, x1, _, _) = philox4x32_10(counter = (step, TAG_POLICY, a, env_id >> 32), key = (seed, env_id)), step = *step_dev + t
//   explore iff (uint64)x0 < explore_below: index = (x1 * n_actions) >> 32, else index = best
//   actions[n][a] = action_lo + index
//
// policy_choose below is that statement, ONE __host__ __device__ function: tests/host_shim/policy_check.cpp compiles the same
// text for the host.  The scan for the maximum is ordered (with a NaN in the row it is not a tree), and the additions of one
// (env, agent, action) are ordered, so one lane owns one (env, agent) and keeps its n_actions accumulators in registers: the
// function is instantiated per n_actions (a uniform switch over 1..16, as k_scalarise does for the reward dimensions), nothing
// is indexed at run time, no scratch.  Parallelism is envs x agents; the unrolled cell loop keeps n_actions x 4 independent
// gathers in flight per lane.  The table slice of a cell is n_actions contiguous floats; tables are read from global memory
// (they live in L2 / the vector L1 and may be rewritten in place between launches).
//
// Work mapping: a workgroup takes E consecutive envs (E = 64, or 32 / 16 for long rows; a multiple of 16 keeps its first byte
// 16-byte aligned).  Their rows are contiguous in global memory: they come into LDS as 16-byte loads (whole chunks inside the
// rows n < N, then single bytes: no byte of a row n >= N is read), with the 256-byte code_of behind them.  Lane q of the group then
// evaluates pair (env = q / A, agent = q % A) and stores one int8; the pairs' bytes are consecutive in `actions`.
// LDS (dynamic): round16(E * row_bytes) | code_of [256].
#pragma once

#include <stdint.h>

#include "sgw_common.hpp"

namespace sgw {

constexpr int POLICY_MAX_ACTIONS = 16;
constexpr int POLICY_MAX_ROW_LDS = 48 * 1024;     // bytes of observation rows a workgroup stages

struct PolicyArgs {
  const uint8_t* obs;            // [n_pad, row_bytes]
  const uint8_t* code_of;        // [256]
  const float* weights;          // [P, A, C, G, n_actions]
  const float* bias;             // [P, A, n_actions] or nullptr
  const int32_t* policy_of_env;  // [n] or nullptr
  const int64_t* step_dev;       // [1]
  int8_t* actions;               // [n, A]
  unsigned long long explore_below, seed;
  long long n, env_id_base, t;
  int row_bytes, envs_per_block, A, P, G, C, n_actions, action_lo;
  int c_a[SGW_MAX_AGENTS];       // cells agent a reads (H*W, or its window's h*w)
  int off_a[SGW_MAX_AGENTS];     // byte offset of agent a's cells in the env's row
};

// The score vector of one (env, agent): the bias, then one float32 addition per cell in cell order.  The one statement of the
// accumulation: policy_choose (the actor) and sgw_policy_scores (sgw_learn.hpp) both call it.
template <int NA>
__host__ __device__ __forceinline__ void policy_score(float (&score)[NA], const uint8_t* o, int C_a, const uint8_t* code_of, const float* w,
                                                      const float* b, int G) {
#pragma unroll
  for (int j = 0; j < NA; ++j) score[j] = b ? b[j] : 0.0f;
#pragma unroll 4
  for (int c = 0; c < C_a; ++c) {
    const float* cell = w + (c * G + (int)code_of[o[c]]) * NA;
#pragma unroll
    for (int j = 0; j < NA; ++j) score[j] = score[j] + cell[j];
  }
}

// the first maximum of a score vector (a NaN never displaces the incumbent); top: its score
template <int NA>
__host__ __device__ __forceinline__ int policy_first_max(const float (&score)[NA], float& top) {
  int best = 0;
  top = score[0];
#pragma unroll
  for (int j = 1; j < NA; ++j)
    if (score[j] > top) { top = score[j]; best = j; }
  return best;
}

// The action INDEX (0 .. NA-1) of one (env, agent).  o: the agent's C_a observation bytes; w: the agent's table
// [C][G][NA] of the env's policy; b: its bias [NA] or nullptr.
template <int NA>
__host__ __device__ inline int policy_choose(const uint8_t* o, int C_a, const uint8_t* code_of, const float* w, const float* b, int G,
                                             unsigned long long explore_below, unsigned long long seed, long long env_id,
                                             long long step, int agent) {
  float score[NA];
  policy_score<NA>(score, o, C_a, code_of, w, b, G);
  float top;
  int best = policy_first_max<NA>(score, top);
  if (explore_below != 0) {
    const U4 r = philox4x32_10((uint32_t)step, TAG_POLICY, (uint32_t)agent, (uint32_t)((uint64_t)env_id >> 32), (uint32_t)seed,
                               (uint32_t)env_id);
    if ((unsigned long long)r.x < explore_below) best = (int)(((uint64_t)r.y * (uint32_t)NA) >> 32);
  }
  return best;
}

constexpr int POLICY_THREADS_MAX = 256;

// v[i] of a kernel-argument array without indexing it at run time (an indexed kernarg array is copied to scratch)
__device__ __forceinline__ int policy_pick(const int (&v)[SGW_MAX_AGENTS], int i) {
  static_assert(SGW_MAX_AGENTS == 4, "policy_pick selects among four agents");
  return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
}

template <int NA>
__device__ __forceinline__ void policy_act_block(const PolicyArgs& a, uint8_t* lds) {
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const long long env0 = (long long)blockIdx.x * a.envs_per_block;
  const long long left = a.n - env0;
  const int nrow = left < a.envs_per_block ? (int)left : a.envs_per_block;          // a ragged last group takes only its own rows
  const int nbytes = nrow * a.row_bytes;
  const uint8_t* src = a.obs + env0 * a.row_bytes;                                   // 16-byte aligned: envs_per_block % 16 == 0
  uint8_t* codes = lds + (a.envs_per_block * a.row_bytes + 15) / 16 * 16;
  for (int i = tid * 16; i + 16 <= nbytes; i += nthr * 16)
    *reinterpret_cast<uint4*>(lds + i) = *reinterpret_cast<const uint4*>(src + i);
  for (int i = (nbytes & ~15) + tid; i < nbytes; i += nthr) lds[i] = src[i];
  for (int i = tid; i < 256; i += nthr) codes[i] = a.code_of[i];
  __syncthreads();
  const long long step = *a.step_dev + a.t;
  for (int q = tid; q < nrow * a.A; q += nthr) {
    const int env = q / a.A, ag = q - env * a.A;
    const long long n = env0 + env;
    const int p = a.policy_of_env ? a.policy_of_env[n] : 0;
    int action = 0;                                                                  // a table index out of range: 0, nothing is read
    if (p >= 0 && p < a.P) {
      const long long slice = (long long)p * a.A + ag;
      const float* w = a.weights + slice * a.C * a.G * NA;
      const float* b = a.bias ? a.bias + slice * NA : nullptr;
      action = a.action_lo + policy_choose<NA>(lds + env * a.row_bytes + policy_pick(a.off_a, ag), policy_pick(a.c_a, ag), codes, w, b, a.G, a.explore_below,
                                               a.seed, a.env_id_base + n, step, ag);
    }
    a.actions[n * a.A + ag] = (int8_t)action;
  }
}

__global__ __launch_bounds__(POLICY_THREADS_MAX) void k_policy_act(PolicyArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t policy_lds[];
  switch (a.n_actions) {                                                             // uniform
#define SGW_POLICY_CASE(NA) case NA: policy_act_block<NA>(a, policy_lds); break;
    SGW_POLICY_CASE(1) SGW_POLICY_CASE(2) SGW_POLICY_CASE(3) SGW_POLICY_CASE(4) SGW_POLICY_CASE(5) SGW_POLICY_CASE(6)
    SGW_POLICY_CASE(7) SGW_POLICY_CASE(8) SGW_POLICY_CASE(9) SGW_POLICY_CASE(10) SGW_POLICY_CASE(11) SGW_POLICY_CASE(12)
    SGW_POLICY_CASE(13) SGW_POLICY_CASE(14) SGW_POLICY_CASE(15) SGW_POLICY_CASE(16)
#undef SGW_POLICY_CASE
    default: break;
  }
}

// after the T steps of sgw_policy_step_n: the next call's Philox counters follow on
__global__ void k_policy_advance(int64_t* step_dev, long long T) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *step_dev += T;
}

}  // namespace sgw
