// sgw_episodes.hpp -- the episode log: one record per episode that ends in a batch of output rows, appended to a caller-owned
// log in (t, n) order (the reference's _episodic_performances.append at every LAST timestep, safety_game.py:253-263,
// safety_game_mo.py:1015-1016 -- for the whole batch, with the env, the step, the length, the termination reason, the return
// vector, the hidden performance and the metrics of the row).  A stream compaction with a deterministic order, in three launches
// on the caller's stream; no launch waits on another workgroup, nothing is allocated, nothing is read back.
//
// Unit of work: a TILE = the 64 consecutive envs of one t, one wave (N_pad is a multiple of 64; tile = t * N_pad / 64 + n / 64).
//   k_episode_count  a lane reads its env's A step-type bytes; one __ballot and a population count are the tile's number of
//                    ended episodes -> scratch.
//   k_episode_scan   ONE workgroup: exclusive prefix of the tile numbers (a thread sums a contiguous run of tiles, a shuffle scan
//                    per wave, the sixteen wave totals through LDS), written over them; *count is saved to the scratch as the
//                    call's base and advanced by the total -- one thread, plain loads and stores, no atomics.
//   k_episode_write  the same ballot; the set lanes below a lane (v_mbcnt) are its rank, so a wave's records are ONE contiguous
//                    span of the log at base + prefix[tile].  The small fields go out one store per set lane.  The return and
//                    metric rows are copied by the whole wave: element j of the span is column j % C of record j / C, whose
//                    source lane is the (j / C)-th set bit of the ballot (one ds_permute hands every rank its lane) -- coalesced
//                    stores whose number follows the episodes, not N.  Records at index >= cap are not stored.
// Rows n >= N never count.  The predicate is episode_ended (sgw_common.hpp), the one of sgw_track_performance; it inherits that
// predicate's repeat on idle rounds of the per-agent families (every agent already DEAD, no reset: the row counts again).
#pragma once
#include "sgw_common.hpp"       // episode_ended, div_recip

namespace sgw {

constexpr int EPISODE_SCAN_THREADS = 1024;

struct EpisodeScratch {            // the head of sgw_episodes.scratch; the uint32 tile numbers / prefixes follow
  long long base;                  // *count when the call's scan ran: where the call's records start
  long long pad_;
};

struct EpisodeArgs {
  // source rows [T, N_pad, ...]
  const uint8_t* step_type; const uint8_t* term_reason; const int* frame;
  const unsigned long long* cumulative; const unsigned long long* hidden; const unsigned long long* metrics;    // doubles, copied as bits
  long long n, n_pad, step_base;
  unsigned tiles, tiles_per_t;
  int A, per_agent, R, C, M, recip_C, recip_M;
  // destination
  long long cap;
  int* env; long long* step; int* length; uint8_t* reason;
  unsigned long long* ret; unsigned long long* hid; unsigned long long* met;
  EpisodeScratch* head; unsigned* tile_num;
};

__device__ __forceinline__ int episode_popc_below(uint64_t m) {      // set bits of m in the lanes below this one
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// the ballot of one tile: bit l = env (tile % tiles_per_t) * 64 + l of row t = tile / tiles_per_t ends an episode
__device__ __forceinline__ uint64_t episode_tile_ballot(const uint8_t* step_type, unsigned tile, unsigned tiles_per_t, long long n, long long n_pad,
                                                        int A, int per_agent, int lane, long long& row, bool& ended) {
  const unsigned t = tile / tiles_per_t, w = tile - t * tiles_per_t;
  const long long env = (long long)w * WAVE + lane;
  row = (long long)t * n_pad + env;
  ended = env < n && episode_ended(step_type + row * A, A, per_agent);
  return __ballot(ended);
}

__global__ __launch_bounds__(256) void k_episode_count(const uint8_t* step_type, unsigned tiles, unsigned tiles_per_t, long long n, long long n_pad,
                                                       int A, int per_agent, unsigned* tile_num) {
  const int lane = threadIdx.x & (WAVE - 1);
  const unsigned tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (tile >= tiles) return;                                          // uniform per wave
  long long row; bool ended;
  const uint64_t b = episode_tile_ballot(step_type, tile, tiles_per_t, n, n_pad, A, per_agent, lane, row, ended);
  if (lane == 0) tile_num[tile] = (unsigned)__popcll(b);
}

__global__ __launch_bounds__(EPISODE_SCAN_THREADS) void k_episode_scan(unsigned* tile_num, unsigned tiles, EpisodeScratch* head, long long* count) {
  __shared__ unsigned wave_total[EPISODE_SCAN_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
  const unsigned per = (tiles + EPISODE_SCAN_THREADS - 1) / EPISODE_SCAN_THREADS;
  const unsigned lo = threadIdx.x * per < tiles ? threadIdx.x * per : tiles, hi = lo + per < tiles ? lo + per : tiles;
  unsigned mine = 0;
  for (unsigned i = lo; i < hi; ++i) mine += tile_num[i];
  unsigned incl = mine;
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const unsigned v = (unsigned)__shfl_up((int)incl, d);
    if (lane >= d) incl += v;
  }
  if (lane == WAVE - 1) wave_total[wave] = incl;
  __syncthreads();
  unsigned before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < EPISODE_SCAN_THREADS / WAVE; ++w) {
    const unsigned v = wave_total[w];
    before += w < wave ? v : 0u;
    total += v;
  }
  unsigned run = before + incl - mine;
  for (unsigned i = lo; i < hi; ++i) {
    const unsigned c = tile_num[i];
    tile_num[i] = run;
    run += c;
  }
  if (threadIdx.x == 0) {
    const long long base = *count;
    head->base = base;
    *count = base + (long long)total;
  }
}

// copy the C-column rows of the wave's records: element j of the span = column j % C of record j / C
__device__ __forceinline__ void episode_copy_rows(const unsigned long long* src, unsigned long long* dst, int C, uint32_t recip, long long tile_row0,
                                                  long long first, long long cap, int n_rec, int lane_of_rank, int lane) {
  const int span = n_rec * C;
  for (int j0 = 0; j0 < span; j0 += WAVE) {                           // uniform per wave: every lane reaches the shuffle
    const int j = j0 + lane;
    const int rec = (int)div_recip((uint32_t)j, recip), col = j - rec * C;
    const int src_lane = __shfl(lane_of_rank, rec & (WAVE - 1));
    if (j < span && first + rec < cap) dst[(first + rec) * C + col] = src[(tile_row0 + src_lane) * C + col];
  }
}

__global__ __launch_bounds__(256) void k_episode_write(const EpisodeArgs x) {
  const int lane = threadIdx.x & (WAVE - 1);
  const unsigned tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (tile >= x.tiles) return;                                        // uniform per wave
  long long row; bool ended;
  const uint64_t b = episode_tile_ballot(x.step_type, tile, x.tiles_per_t, x.n, x.n_pad, x.A, x.per_agent, lane, row, ended);
  if (b == 0) return;
  const long long first = x.head->base + (long long)x.tile_num[tile];      // the wave's span of the log starts here
  if (first < 0 || first >= x.cap) return;                            // (a counter the caller never zeroed stores nothing)
  const int n_rec = __popcll(b), rank = episode_popc_below(b);
  const long long at = first + rank;
  if (ended && at < x.cap) {
    const unsigned t = tile / x.tiles_per_t;
    if (x.env) x.env[at] = (int)(row - (long long)t * x.n_pad);
    if (x.step) x.step[at] = x.step_base + t;
    if (x.length) x.length[at] = x.frame[row];
    if (x.hid) x.hid[at] = x.hidden[row];
    if (x.reason)
      for (int r = 0; r < x.R; ++r) x.reason[at * x.R + r] = x.term_reason[row * x.R + r];
  }
  if (x.ret || x.met) {
    // a permutation of the lanes: the set lanes go to their ranks, the others behind them -- lane r < n_rec receives the r-th set lane
    const int to = ended ? rank : n_rec + (lane - rank);
    const int lane_of_rank = __builtin_amdgcn_ds_permute(to << 2, lane);
    const long long tile_row0 = row - lane;
    if (x.ret) episode_copy_rows(x.cumulative, x.ret, x.C, (uint32_t)x.recip_C, tile_row0, first, x.cap, n_rec, lane_of_rank, lane);
    if (x.met) episode_copy_rows(x.metrics, x.met, x.M, (uint32_t)x.recip_M, tile_row0, first, x.cap, n_rec, lane_of_rank, lane);
  }
}

}  // namespace sgw
