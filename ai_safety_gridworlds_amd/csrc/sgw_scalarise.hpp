// sgw_scalarise.hpp -- sgw_scalarise: the scalarise=True branch of _process_timestep (safety_game_mo.py:1027-1066,
// safety_game_moma.py:1253-1321) for a whole batch of output rows in ONE launch.  Per env and agent, over the agent's k enabled
// reward dimensions in the order of the output columns:
//
//   scalar_reward     = sum(reward[0 .. k))
//   scalar_cumulative = sum(cumulative[0 .. k))
//   scalar_average    = sum(cumulative[i] / (frame + 1) for i in 0 .. k)        -- the sum of k quotients, not the quotient of the sum
//
// where sum() is the reference's Python sum() over a list of floats as CPython <= 3.11 computes it: an accumulator that starts
// at +0.0, then one IEEE double addition per column, column 0 first (so a row of -0.0 sums to +0.0, and (1e16, 1, -1e16, 1)
// to 1).  Every addition and division below is written in that order and unrolled for the agent's k (a wave-uniform switch
// over 1..16, as the derived statistics do): the column index is a constant, nothing is indexed at run time, no scratch.  The
// translation unit is built without fast-math flags; a reassociating flag would break the contract.
//
// Work mapping: one wave per 64 envs of one step t.  The wave's 64 x A rows of `reward` and `cumulative` are contiguous in
// global memory (each row is K doubles; a lane walking its own row would read at a stride of 8 K bytes): they come in as 16-byte
// loads and are transposed through LDS as [agent * K + dimension][lane], so a lane then reads its own vector conflict-free
// (the staging of derived_stats_wave, sgw_observe.hpp).  Only the rows n < N of a step's N_pad block are read or written.
// LDS (dynamic): R [A * K][64] | C [A * K][64] doubles = 1 KiB per column pair, at most 64 KiB.
#pragma once

#include <stdint.h>

#include "sgw_common.hpp"

namespace sgw {

struct ScalariseArgs {
  const double* reward;        // [T, n_pad, A, K] or nullptr (not needed)
  const double* cumulative;    // [T, n_pad, A, K] or nullptr
  const int32_t* frame;        // [T, n_pad] or nullptr
  double* scalar_reward;       // [T, n_pad, A] each, or nullptr
  double* scalar_cumulative;
  double* scalar_average;
  long long n, n_pad;
  unsigned chunks;             // waves per step: ceil(n / 64)
  int A, K;
  int recip_AK;                // ceil(2^18 / (A K)): (e * recip_AK) >> 18 == e / (A K) for e < 64 * 64
  int k[SGW_MAX_AGENTS];       // reward dimensions of each agent, 0 .. K
};

// The wave's nel = rows * A * K doubles at g (16-byte aligned: a wave's block starts on a multiple of 64 rows) -> L[column][row]
__device__ inline void scalarise_stage(double* L, const double* g, int nel, int AK, int recip_AK, int lane) {
  for (int e0 = 2 * lane; e0 < nel; e0 += 2 * WAVE) {
    const bool two = e0 + 1 < nel;
    double v0, v1 = 0.0;
    if (two) {
      const double2 v = *reinterpret_cast<const double2*>(g + e0);
      v0 = v.x; v1 = v.y;
    } else {
      v0 = g[e0];
    }
    int row = (e0 * recip_AK) >> 18, col = e0 - row * AK;
    L[col * WAVE + row] = v0;
    if (two) {
      row = ((e0 + 1) * recip_AK) >> 18; col = e0 + 1 - row * AK;
      L[col * WAVE + row] = v1;
    }
  }
}

// One agent of this lane's env: Rv / Cv are the agent's columns [dimension][lane]
template <int KK>
__device__ __forceinline__ void scalarise_agent(const double* Rv, const double* Cv, int lane, double denom, bool want_r, bool want_c,
                                                bool want_a, double& sr, double& sc, double& sa) {
  if (want_r) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < KK; ++i) s = s + Rv[i * WAVE + lane];
    sr = s;
  }
  if (want_c || want_a) {
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < KK; ++i) {
      const double c = Cv[i * WAVE + lane];
      s = s + c;
      if (want_a) q = q + c / denom;
    }
    sc = s; sa = q;
  }
}

__global__ __launch_bounds__(WAVE) void k_scalarise(ScalariseArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sc_lds[];
  const int lane = (int)threadIdx.x;
  const unsigned t = blockIdx.x / a.chunks, chunk = blockIdx.x - t * a.chunks;          // uniform
  const long long env0 = (long long)chunk * WAVE;
  const long long rows_left = a.n - env0;
  const int nrow = rows_left < WAVE ? (int)rows_left : WAVE;                             // a ragged last wave takes only its own rows
  const long long row0 = (long long)t * a.n_pad + env0;
  const int A = a.A, K = a.K, AK = A * K;
  double* R = reinterpret_cast<double*>(sc_lds);
  double* Cm = R + AK * WAVE;
  const bool want_r = a.scalar_reward != nullptr, want_c = a.scalar_cumulative != nullptr, want_a = a.scalar_average != nullptr;
  if (want_r) scalarise_stage(R, a.reward + row0 * AK, nrow * AK, AK, a.recip_AK, lane);
  if (want_c || want_a) scalarise_stage(Cm, a.cumulative + row0 * AK, nrow * AK, AK, a.recip_AK, lane);
  double denom = 1.0;
  if (want_a && lane < nrow) denom = (double)(a.frame[row0 + lane] + 1);
  lds_wave_sync();
  if (lane >= nrow) return;
  for (int ag = 0; ag < A; ++ag) {
    const double* Rv = R + ag * K * WAVE;
    const double* Cv = Cm + ag * K * WAVE;
    double sr = 0.0, sc = 0.0, sa = 0.0;                            // an agent without reward dimensions: sum([]) = 0
    switch (a.k[ag]) {                                              // uniform
#define SGW_SC_CASE(KK) case KK: scalarise_agent<KK>(Rv, Cv, lane, denom, want_r, want_c, want_a, sr, sc, sa); break;
      SGW_SC_CASE(1) SGW_SC_CASE(2) SGW_SC_CASE(3) SGW_SC_CASE(4) SGW_SC_CASE(5) SGW_SC_CASE(6) SGW_SC_CASE(7) SGW_SC_CASE(8)
      SGW_SC_CASE(9) SGW_SC_CASE(10) SGW_SC_CASE(11) SGW_SC_CASE(12) SGW_SC_CASE(13) SGW_SC_CASE(14) SGW_SC_CASE(15) SGW_SC_CASE(16)
#undef SGW_SC_CASE
      default: break;
    }
    const long long o = (row0 + lane) * A + ag;
    if (want_r) a.scalar_reward[o] = sr;
    if (want_c) a.scalar_cumulative[o] = sc;
    if (want_a) a.scalar_average[o] = sa;
  }
}

}  // namespace sgw
