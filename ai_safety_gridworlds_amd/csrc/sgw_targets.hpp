// sgw_targets.hpp -- sgw_td_targets: the discounted return-to-go and the GAE-lambda advantage of a rollout buffer, the backward
// recursion over T that every learner runs first on the [T, N_pad, ...] `reward` / `step_type` / `term_reason` buffers of a
// write_every call, cut at episode ends by the REFERENCE'S conventions (not Gym's): an auto-reset consumes a step slot (that row is
// FIRST: no action was played, its reward is 0); `terminated` is reported at max-steps too and only `term_reason` tells the two
// apart; in the per-agent families an agent goes LAST -> DEAD while the others play on.
//
// The rule of one element (env n < N, agent a < A, column c < C), td_element below, ONE __host__ __device__ function
// (tests/host_shim/targets_check.cpp compiles the same text for the host).  g = gamma[c], gl = g * lambda (one multiplication);
// every `*`, `+`, `-` is one IEEE double operation rounded on its own (the build carries -ffp-contract=off and no fast-math flag):
//
//   carry_ret = value ? value[T-1] : 0.0;  carry_adv = 0.0               -- what lies beyond the buffer
//   for t = T-1 .. 0:
//     st = step_type[t, n, a];  r = reward[t, n, a, c]
//     MID:   cont = 1
//     LAST:  cont = 2 if BOOTSTRAP_TRUNCATED and term_reason[t, n, min(a, R-1)] == SGW_MAX_STEPS, else 0
//     FIRST, DEAD, any other byte:  ret[t] = adv[t] = +0.0, valid[t] = 0, both carries = +0.0, next row
//     valid[t] = 1;  v = value ? value[t] : 0.0;  vprev = t > 0 ? value[t-1] : value0        (vprev is read for adv only)
//     cont 1: ret[t] = r + g * carry_ret;  adv[t] = ((r + g * v) - vprev) + gl * carry_adv
//     cont 2: ret[t] = r + g * v;          adv[t] = (r + g * v) - vprev      -- truncated: bootstraps from its own row
//     cont 0: ret[t] = r;                  adv[t] = r - vprev                -- terminated: r itself (a -0.0 stays -0.0)
//     carry_ret = ret[t];  carry_adv = adv[t]
//
// Work mapping of k_td_targets: one lane per element i = (n * A + a) * C + c < N A C, walking t from T-1 down to 0.  Element i of
// step t sits at t * rows * A C + i, so the 64 lanes of a wave read and write 512 contiguous bytes of every double array per step;
// the step_type byte of an agent is one address for its C lanes; `valid` is written by the lane c == 0.  The recurrence is serial,
// the loads are not: the rows come in groups of TD_DEPTH, and the loads of the NEXT group (reward, value, step_type, term_reason
// of TD_DEPTH rows: up to 4 TD_DEPTH loads per lane in flight) are issued before the arithmetic of the current one, so the HBM
// latency is paid once per group.  The groups are unrolled: every row of a group is a named register, nothing is indexed at
// run time, no scratch, no LDS.  gamma arrives in the kernel arguments; a lane picks its entry once with a chain of selects.
// What a call reads (values, term_reason) and writes (adv) selects one of six instantiations of the loop, so a group's loads stand
// in a row with no branch between them.  Rows n >= N of every array are neither read nor written.
#pragma once

#include <stdint.h>

#include "sgw_common.hpp"

namespace sgw {

constexpr int TD_DEPTH = 4;          // rows per group: 2 groups x (2 doubles + 2 bytes) x TD_DEPTH registers hold the loads in flight
                                     // (83 VGPRs; 8 rows: 131 VGPRs, fewer resident waves, 10 % slower -- DESIGN.md 4.8)
constexpr int TD_THREADS = 256;

struct TdArgs {
  const double* reward;              // [T, src_rows, A, C]
  const uint8_t* step_type;          // [T, src_rows, A]
  const uint8_t* term_reason;        // [T, src_rows, R]; read only with bootstrap
  const double* value;               // [T, dst_rows, A, C] or nullptr
  const double* value0;              // [dst_rows, A, C]; read only when adv is written
  double* ret;                       // [T, dst_rows, A, C] each, or nullptr
  double* adv;
  uint8_t* valid;                    // [T, dst_rows, A] or nullptr
  long long src_rows, dst_rows;
  long long n_elems;                 // N * A * C
  int T, A, C, R;
  int bootstrap;                     // SGW_TD_BOOTSTRAP_TRUNCATED set
  double lambda;
  double gamma[SGW_MAX_K];           // [C]
};

// the loads of TD_DEPTH rows of one element, row t0 - j in slot j.  A row below 0 (the ragged last group) re-reads row 0, whose
// lines the group has just asked for: the loads of a group are the same on every path, nothing branches between them
struct TdRows {
  double r[TD_DEPTH], v[TD_DEPTH];
  uint8_t st[TD_DEPTH], tr[TD_DEPTH];
};

template <bool VALUE, bool BOOT>
__host__ __device__ __forceinline__ void td_load(TdRows& g, const TdArgs& a, int t0, long long i, long long pair, long long reason) {
  const long long AC = (long long)a.A * a.C;
#pragma unroll
  for (int j = 0; j < TD_DEPTH; ++j) {
    const long long t = t0 - j > 0 ? t0 - j : 0;                             // uniform
    g.r[j] = a.reward[t * a.src_rows * AC + i];
    g.st[j] = a.step_type[t * a.src_rows * a.A + pair];
    g.tr[j] = BOOT ? a.term_reason[t * a.src_rows * a.R + reason] : (uint8_t)SGW_TERM_NONE;
    g.v[j] = VALUE ? a.value[t * a.dst_rows * AC + i] : 0.0;
  }
}

// one element's backward loop: i = (n * A + a) * C + c, i < a.n_elems.  VALUE: a.value is given; BOOT: SGW_TD_BOOTSTRAP_TRUNCATED;
// ADV: a.adv is written (needs VALUE and a.value0)
template <bool VALUE, bool BOOT, bool ADV>
__host__ __device__ __forceinline__ void td_element(const TdArgs& a, long long i) {
  static_assert(VALUE || !ADV, "the advantages need the values");
  const long long pair = i / a.C;                                            // n * A + a
  const int c = (int)(i - pair * a.C);
  const long long n = pair / a.A;
  const int ag = (int)(pair - n * a.A);
  const long long reason = n * a.R + (ag < a.R ? ag : a.R - 1);
  double g = a.gamma[0];
#pragma unroll
  for (int k = 1; k < SGW_MAX_K; ++k) g = c == k ? a.gamma[k] : g;           // constant indices: the argument block is never indexed at run time
  const double gl = g * a.lambda;
  const bool want_ret = a.ret != nullptr, want_valid = a.valid != nullptr && c == 0;
  const long long AC = (long long)a.A * a.C;

  TdRows cur, nxt;
  td_load<VALUE, BOOT>(cur, a, a.T - 1, i, pair, reason);
  double v0 = 0.0;                                                           // the vprev of row 0
  if (ADV) v0 = a.value0[i];
  double carry_ret = cur.v[0];                                               // value[T-1], or 0.0 without values
  double carry_adv = 0.0;
  for (int t0 = a.T - 1; t0 >= 0; t0 -= TD_DEPTH) {
    td_load<VALUE, BOOT>(nxt, a, t0 - TD_DEPTH, i, pair, reason);            // in flight while this group is computed
#pragma unroll
    for (int j = 0; j < TD_DEPTH; ++j) {
      const int t = t0 - j;                                                  // uniform
      if (t < 0) break;
      const int st = cur.st[j];
      const double r = cur.r[j], v = cur.v[j];
      const double below = j + 1 < TD_DEPTH ? cur.v[j + 1] : nxt.v[0];
      const double vprev = t > 0 ? below : v0;
      double ret = 0.0, adv = 0.0;
      uint8_t valid = 0;
      if (st == SGW_MID || st == SGW_LAST) {
        const int cont = st == SGW_MID ? 1 : (BOOT && cur.tr[j] == SGW_MAX_STEPS) ? 2 : 0;
        valid = 1;
        const double boot = r + g * v;
        if (cont == 1) {
          ret = r + g * carry_ret;
          if (ADV) adv = (boot - vprev) + gl * carry_adv;
        } else if (cont == 2) {
          ret = boot;
          if (ADV) adv = boot - vprev;
        } else {
          ret = r;
          if (ADV) adv = r - vprev;
        }
      }
      carry_ret = ret; carry_adv = adv;
      const long long o = t * a.dst_rows * AC + i;
      if (want_ret) a.ret[o] = ret;
      if (ADV) a.adv[o] = adv;
      if (want_valid) a.valid[t * a.dst_rows * a.A + pair] = valid;
    }
    cur = nxt;
  }
}

// the instantiation a call needs, from what its argument block holds (uniform)
__host__ __device__ __forceinline__ void td_element_any(const TdArgs& a, long long i) {
  const bool value = a.value != nullptr, boot = a.bootstrap != 0, adv = a.adv != nullptr;
  if (adv) { if (boot) td_element<true, true, true>(a, i); else td_element<true, false, true>(a, i); }
  else if (value) { if (boot) td_element<true, true, false>(a, i); else td_element<true, false, false>(a, i); }
  else { if (boot) td_element<false, true, false>(a, i); else td_element<false, false, false>(a, i); }
}

__global__ __launch_bounds__(TD_THREADS) void k_td_targets(TdArgs a) {
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i >= a.n_elems) return;                                                // lanes past N A C do nothing
  td_element_any(a, i);
}

}  // namespace sgw
