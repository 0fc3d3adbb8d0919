// sgw_softmax.hpp -- sgw_policy_sample / sgw_policy_sample_step_n / sgw_policy_probs / sgw_policy_accumulate_softmax: the SOFTMAX half of
// the table-policy stack.  The score vector, `best` and `top` of one (env, agent) are those of sgw_policy.hpp (policy_score,
// policy_first_max, unchanged); on top of them, with beta2 = inverse temperature * log2(e) (float32, finite, >= 0):
//
//   z_j   = (score[j] - top) * beta2            one float32 subtraction, then one float32 multiplication
//   w_j   = E(z_j)
//   E(z)  : if !(z >= -125.0f) -> +0.0f         (NaN included: a NaN or -inf score is never sampled)
//           k = rintf(z) (ties to even);  g = z - k          (exact, g in [-0.5, 0.5])
//           p = 1 + g*(c1 + g*(c2 + g*(c3 + g*(c4 + g*(c5 + g*c6)))))   Horner: every * and + one float32 operation, nothing fused
//           E = ldexpf(p, (int)k)               (exact: never subnormal)
//           c1..c6 = float32((ln 2)^i / i!) = 0x1.62e430p-1, 0x1.ebfbe0p-3, 0x1.c6b08ep-5, 0x1.3b2ab6p-7, 0x1.5d87fep-10, 0x1.430912p-13
//   total = 0.0; for j = 0..NA-1 in order: total = total + (double)w_j        one double addition each
//   degenerate iff !(total > 0.0)               (exactly when top is NaN or infinite)
//   pi_j  = (double)w_j / total                 one double division
//
// Each rule is ONE __host__ __device__ function (tests/host_shim/softmax_check.cpp compiles the same text for the host, and
// tests/softmax_ref.py restates it in numpy): softmax_exp2, softmax_weights, softmax_pick (the sampler), softmax_pi (the
// probabilities), softmax_grad (the NA fixed-point score-function terms of one transition).  Like policy_choose they are
// instantiated per n_actions = 1..16 and pick registers by selects: nothing is indexed at run time, no scratch.
//
// The kernels follow their greedy twins line for line: k_policy_sample stages as k_policy_act does, k_policy_probs as
// k_policy_scores; k_policy_accumulate_softmax has k_policy_accumulate's slices, tiles, LDS bins (P == 1) and global atomics
// (P > 1), with ONE difference: a transition adds to EVERY action's bin, so the staging phase leaves q[E][NA] (int32) instead of
// one q per env -- one lane per env of the tile evaluates the agent's whole score vector from the staged row (tables gathered from
// global memory, as k_policy_scores does) -- and the walk issues NA adds per cell, skipping each q_j == 0.
// LDS of k_policy_accumulate_softmax (softmax_acc_lds): round16(E * row_bytes) | code_of [256] | q int32 [E][NA] | p int32 [E]
// | bins int64 [R * G * NA + NA] (P == 1).
#pragma once

#include <math.h>
#include <stdint.h>

#include "sgw_common.hpp"
#include "sgw_policy.hpp"
#include "sgw_learn.hpp"

namespace sgw {

enum { TAG_SAMPLE = 3 };                             // the Philox stream of the softmax sampler (TAG_POLICY: the exploration draws)

// ---- the element rules ----------------------------------------------------------------------------------------------------------
// 2^z for z <= 0 in float32, +0.0f below -125 and for a NaN; every operation is rounded on its own (-ffp-contract=off)
__host__ __device__ __forceinline__ float softmax_exp2(float z) {
  if (!(z >= -125.0f)) return 0.0f;
  const float k = rintf(z);
  const float g = z - k;
  float p = g * 0x1.430912p-13f;
  p = 0x1.5d87fep-10f + p; p = g * p;
  p = 0x1.3b2ab6p-7f + p; p = g * p;
  p = 0x1.c6b08ep-5f + p; p = g * p;
  p = 0x1.ebfbe0p-3f + p; p = g * p;
  p = 0x1.62e430p-1f + p; p = g * p;
  p = 1.0f + p;
  return ldexpf(p, (int)k);
}

// w_j of a score vector and their ordered double sum
template <int NA>
__host__ __device__ __forceinline__ double softmax_weights(float (&w)[NA], const float (&score)[NA], float top, float beta2) {
  double total = 0.0;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const float d = score[j] - top;
    const float z = d * beta2;
    w[j] = softmax_exp2(z);
    total = total + (double)w[j];
  }
  return total;
}

// The sampled index among weights whose sum `total` is > 0: the first j with thr < cum_j.  cum ends on total bit for bit and
// thr < total, so it is always found (NA - 1 is only the initial value).
template <int NA>
__host__ __device__ __forceinline__ int softmax_pick(const float (&w)[NA], double total, uint32_t x0) {
  const double u = ((double)x0 + 0.5) * 0x1p-32;
  const double thr = u * total;
  double cum = 0.0;
  int index = NA - 1;
  bool found = false;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    cum = cum + (double)w[j];
    const bool hit = !found && thr < cum;
    index = hit ? j : index;
    found = found || hit;
  }
  return index;
}

// The action INDEX of one (env, agent) under the softmax policy; the arguments are policy_choose's, plus beta2.
template <int NA>
__host__ __device__ inline int softmax_choose(const uint8_t* o, int C_a, const uint8_t* code_of, const float* w, const float* b, int G,
                                              float beta2, unsigned long long explore_below, unsigned long long seed, long long env_id,
                                              long long step, int agent) {
  float score[NA];
  policy_score<NA>(score, o, C_a, code_of, w, b, G);
  float top;
  const int best = policy_first_max<NA>(score, top);
  if (explore_below != 0) {                                                          // explore first, exactly as policy_choose
    const U4 r = philox4x32_10((uint32_t)step, TAG_POLICY, (uint32_t)agent, (uint32_t)((uint64_t)env_id >> 32), (uint32_t)seed,
                               (uint32_t)env_id);
    if ((unsigned long long)r.x < explore_below) return (int)(((uint64_t)r.y * (uint32_t)NA) >> 32);
  }
  float wt[NA];
  const double total = softmax_weights<NA>(wt, score, top, beta2);
  if (!(total > 0.0)) return best;                                                   // degenerate: top is NaN or infinite
  const U4 r = philox4x32_10((uint32_t)step, TAG_SAMPLE, (uint32_t)agent, (uint32_t)((uint64_t)env_id >> 32), (uint32_t)seed,
                             (uint32_t)env_id);
  return softmax_pick<NA>(wt, total, r.x);
}

// pi of a score vector; false: the row is degenerate (pi is then 1.0 at best, +0.0 elsewhere)
template <int NA>
__host__ __device__ __forceinline__ bool softmax_pi(double (&pi)[NA], const float (&score)[NA], float beta2) {
  float top;
  const int best = policy_first_max<NA>(score, top);
  float wt[NA];
  const double total = softmax_weights<NA>(wt, score, top, beta2);
  const bool live = total > 0.0;
#pragma unroll
  for (int j = 0; j < NA; ++j) pi[j] = live ? (double)wt[j] / total : (j == best ? 1.0 : 0.0);
  return live;
}

// q_j = learn_quantise(coef * ((j == a ? 1.0 : 0.0) - pi_j), scale) for every j: the score-function terms of one transition
template <int NA>
__host__ __device__ __forceinline__ void softmax_grad(long long (&q)[NA], const double (&pi)[NA], int a, double coef, double scale) {
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const double d = (j == a ? 1.0 : 0.0) - pi[j];
    const double x = coef * d;
    q[j] = learn_quantise(x, scale);
  }
}

#ifndef SGW_LEARN_RULES_ONLY
// ---- sgw_policy_sample ----------------------------------------------------------------------------------------------------------
struct SampleArgs { PolicyArgs p; float beta2; };

template <int NA>
__device__ __forceinline__ void policy_sample_block(const SampleArgs& s, uint8_t* lds) {
  const PolicyArgs& a = s.p;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const long long env0 = (long long)blockIdx.x * a.envs_per_block;
  const long long left = a.n - env0;
  const int nrow = left < a.envs_per_block ? (int)left : a.envs_per_block;
  const uint8_t* src = a.obs + env0 * a.row_bytes;                                   // 16-byte aligned: envs_per_block % 16 == 0
  uint8_t* codes = lds + (a.envs_per_block * a.row_bytes + 15) / 16 * 16;
  learn_stage_rows(lds, src, nrow * a.row_bytes, tid, nthr);
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
      action = a.action_lo + softmax_choose<NA>(lds + env * a.row_bytes + policy_pick(a.off_a, ag), policy_pick(a.c_a, ag), codes, w, b, a.G,
                                                s.beta2, a.explore_below, a.seed, a.env_id_base + n, step, ag);
    }
    a.actions[n * a.A + ag] = (int8_t)action;
  }
}

__global__ __launch_bounds__(POLICY_THREADS_MAX) void k_policy_sample(SampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t policy_lds[];
  switch (a.p.n_actions) {                                                           // uniform
#define SGW_SAMPLE_CASE(NA) case NA: policy_sample_block<NA>(a, policy_lds); break;
    SGW_SAMPLE_CASE(1) SGW_SAMPLE_CASE(2) SGW_SAMPLE_CASE(3) SGW_SAMPLE_CASE(4) SGW_SAMPLE_CASE(5) SGW_SAMPLE_CASE(6)
    SGW_SAMPLE_CASE(7) SGW_SAMPLE_CASE(8) SGW_SAMPLE_CASE(9) SGW_SAMPLE_CASE(10) SGW_SAMPLE_CASE(11) SGW_SAMPLE_CASE(12)
    SGW_SAMPLE_CASE(13) SGW_SAMPLE_CASE(14) SGW_SAMPLE_CASE(15) SGW_SAMPLE_CASE(16)
#undef SGW_SAMPLE_CASE
    default: break;
  }
}

// ---- sgw_policy_probs -----------------------------------------------------------------------------------------------------------
struct ProbsArgs {
  const uint8_t* obs0;           // O[0]: [>= n, row_bytes]
  const uint8_t* obs;            // O[1 .. T]: [T, obs_rows, row_bytes]
  const uint8_t* code_of;
  const float* weights;
  const float* bias;
  const int32_t* policy_of_env;
  const int8_t* actions;         // [T, n, A] or nullptr
  float* probs;                  // [T+1, n, A, n_actions] or nullptr
  double* p_chosen;              // [T, n, A] or nullptr
  long long n, obs_rows, groups;
  float beta2;
  int T, row_bytes, envs_per_block, A, P, G, C, n_actions, action_lo;
  int c_a[SGW_MAX_AGENTS], off_a[SGW_MAX_AGENTS];
};

template <int NA>
__device__ __forceinline__ void policy_probs_block(const ProbsArgs& a, uint8_t* lds) {
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
  const bool played = a.p_chosen != nullptr && s < a.T;                               // O[T] has no action
  for (int q = tid; q < nrow * a.A; q += nthr) {
    const int env = q / a.A, ag = q - env * a.A;
    const long long n = env0 + env;
    const int p = a.policy_of_env ? a.policy_of_env[n] : 0;
    const long long pair = (s * a.n + n) * a.A + ag;
    double pi[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) pi[k] = 0.0;                                        // an unknown table: +0.0 everywhere, nothing is read
    if (p >= 0 && p < a.P) {
      const long long slice = (long long)p * a.A + ag;
      float score[NA];
      policy_score<NA>(score, lds + env * a.row_bytes + policy_pick(a.off_a, ag), policy_pick(a.c_a, ag), codes, a.weights + slice * a.C * a.G * NA,
                       a.bias ? a.bias + slice * NA : nullptr, a.G);
      softmax_pi<NA>(pi, score, a.beta2);
    }
    if (a.probs) {
#pragma unroll
      for (int k = 0; k < NA; ++k) a.probs[pair * NA + k] = (float)pi[k];
    }
    if (played) {
      const int j = (int)a.actions[pair] - a.action_lo;
      double c = 0.0;
#pragma unroll
      for (int k = 0; k < NA; ++k) c = j == k ? pi[k] : c;                           // selects: the registers are never indexed at run time
      a.p_chosen[pair] = c;
    }
  }
}

__global__ __launch_bounds__(POLICY_THREADS_MAX) void k_policy_probs(ProbsArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t policy_lds[];
  switch (a.n_actions) {                                                             // uniform
#define SGW_PROBS_CASE(NA) case NA: policy_probs_block<NA>(a, policy_lds); break;
    SGW_PROBS_CASE(1) SGW_PROBS_CASE(2) SGW_PROBS_CASE(3) SGW_PROBS_CASE(4) SGW_PROBS_CASE(5) SGW_PROBS_CASE(6)
    SGW_PROBS_CASE(7) SGW_PROBS_CASE(8) SGW_PROBS_CASE(9) SGW_PROBS_CASE(10) SGW_PROBS_CASE(11) SGW_PROBS_CASE(12)
    SGW_PROBS_CASE(13) SGW_PROBS_CASE(14) SGW_PROBS_CASE(15) SGW_PROBS_CASE(16)
#undef SGW_PROBS_CASE
    default: break;
  }
}

// ---- sgw_policy_accumulate_softmax ----------------------------------------------------------------------------------------------
struct SoftAccArgs {
  AccArgs a;                           // k_policy_accumulate's arguments: the same slices and tiles
  const float* weights;
  const float* bias;
  float beta2;
};

// The LDS layout, computed by the launcher (the bytes it requests) and by the kernel (the offsets it uses) from the same numbers
struct SoftAccLds { int codes, q, p, bins, total; };
__host__ __device__ __forceinline__ SoftAccLds softmax_acc_lds(int E, int row_bytes, int NA, int R, int G, bool in_lds) {
  SoftAccLds l;
  l.codes = (E * row_bytes + 15) / 16 * 16;
  l.q = l.codes + 256;
  l.p = l.q + E * NA * 4;
  l.bins = l.p + E * 4;                                                              // 8-byte aligned: E is a multiple of 16
  l.total = l.bins + (in_lds ? (R * G * NA + NA) * 8 : 0);
  return l;
}

// one env of a tile: q[0 .. NA) of its transition, all 0 for a transition that is skipped
template <int NA>
__device__ __forceinline__ void softmax_stage_env(const SoftAccArgs& s, int32_t* q_out, const uint8_t* o, int C_a, const uint8_t* codes, int p, int ag,
                                                  int j, double coef) {
  const AccArgs& a = s.a;
  long long q[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) q[k] = 0;
  if (p >= 0 && p < a.P && j >= 0 && j < NA) {
    const long long slice = (long long)p * a.A + ag;
    float score[NA];
    policy_score<NA>(score, o, C_a, codes, s.weights + slice * a.C * a.G * NA, s.bias ? s.bias + slice * NA : nullptr, a.G);
    double pi[NA];
    if (softmax_pi<NA>(pi, score, s.beta2)) softmax_grad<NA>(q, pi, j, coef, a.scale);
  }
#pragma unroll
  for (int k = 0; k < NA; ++k) q_out[k] = (int32_t)q[k];
}

__global__ __launch_bounds__(LEARN_THREADS) void k_policy_accumulate_softmax(SoftAccArgs s) {
  extern __shared__ __attribute__((aligned(16))) uint8_t learn_lds[];
  const AccArgs& a = s.a;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  const int E = a.envs_per_block, NA = a.n_actions;
  const bool in_lds = a.P == 1;
  const SoftAccLds l = softmax_acc_lds(E, a.row_bytes, NA, a.R, a.G, in_lds);
  uint8_t* codes = learn_lds + l.codes;
  int32_t* qs = reinterpret_cast<int32_t*>(learn_lds + l.q);
  int32_t* ps = reinterpret_cast<int32_t*>(learn_lds + l.p);
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(learn_lds + l.bins);
  const int slice = (int)blockIdx.x / a.blocks_per_slice, first = (int)blockIdx.x - slice * a.blocks_per_slice;
  static_assert(SGW_MAX_AGENTS == 4, "the slice table is searched by three compares");
  const int ag = (a.A > 3 && slice >= a.slice0[3]) ? 3 : (a.A > 2 && slice >= a.slice0[2]) ? 2 : (a.A > 1 && slice >= a.slice0[1]) ? 1 : 0;
  const int chunk = slice - policy_pick(a.slice0, ag);
  const int C_a = policy_pick(a.c_a, ag), off = policy_pick(a.off_a, ag);
  const int c0 = chunk * a.R;
  const int cn = C_a - c0 < a.R ? (C_a - c0 > 0 ? C_a - c0 : 0) : a.R;               // cells of this slice (0: an agent without a window)
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
    __syncthreads();                                                                 // the rows (and code_of) are there: the scores read them
    for (int i = tid; i < nrow; i += nthr) {
      const long long n = env0 + i, pair = (t * a.n + n) * a.A + ag;
      const int p = a.policy_of_env ? a.policy_of_env[n] : 0;
      const int j = (int)a.actions[pair] - a.action_lo;
      const double coef = a.coef[pair];
      const uint8_t* o = learn_lds + i * a.row_bytes + off;                          // the agent's WHOLE window, whatever cell range the slice has
      int32_t* q_out = qs + i * NA;
      switch (NA) {                                                                  // uniform
#define SGW_STAGE_CASE(K) case K: softmax_stage_env<K>(s, q_out, o, C_a, codes, p, ag, j, coef); break;
        SGW_STAGE_CASE(1) SGW_STAGE_CASE(2) SGW_STAGE_CASE(3) SGW_STAGE_CASE(4) SGW_STAGE_CASE(5) SGW_STAGE_CASE(6)
        SGW_STAGE_CASE(7) SGW_STAGE_CASE(8) SGW_STAGE_CASE(9) SGW_STAGE_CASE(10) SGW_STAGE_CASE(11) SGW_STAGE_CASE(12)
        SGW_STAGE_CASE(13) SGW_STAGE_CASE(14) SGW_STAGE_CASE(15) SGW_STAGE_CASE(16)
#undef SGW_STAGE_CASE
        default: break;
      }
      ps[i] = p >= 0 && p < a.P ? p : 0;
    }
    __syncthreads();
    for (int i = wave; i < nrow; i += waves) {                                       // q[0 .. NA), p: uniform over the wave
      const int32_t* q = qs + i * NA;
      bool any = false;
      for (int k = 0; k < NA; ++k) any = any || q[k] != 0;
      if (!any) continue;
      const uint8_t* o = learn_lds + i * a.row_bytes + off + c0;
      if (in_lds) {
        if (with_bias && lane < NA) {
          const long long v = q[lane];
          if (v != 0) learn_lds_add(bias_bins + lane, v);
        }
        for (int c = lane; c < cn; c += 64) {
          unsigned long long* cell = bins + (c * a.G + (int)codes[o[c]]) * NA;
          for (int k = 0; k < NA; ++k) {
            const long long v = q[k];
            if (v != 0) learn_lds_add(cell + k, v);
          }
        }
      } else {
        const long long slice_p = (long long)ps[i] * a.A + ag;
        if (with_bias && lane < NA) {
          const long long v = q[lane];
          if (v != 0) learn_global_add(a.acc_b + slice_p * NA + lane, (unsigned long long)v);
        }
        unsigned long long* table = a.acc_w + (slice_p * a.C + c0) * a.G * NA;
        for (int c = lane; c < cn; c += 64) {
          unsigned long long* cell = table + (c * a.G + (int)codes[o[c]]) * NA;
          for (int k = 0; k < NA; ++k) {
            const long long v = q[k];
            if (v != 0) learn_global_add(cell + k, (unsigned long long)v);
          }
        }
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
#endif  // SGW_LEARN_RULES_ONLY

}  // namespace sgw
