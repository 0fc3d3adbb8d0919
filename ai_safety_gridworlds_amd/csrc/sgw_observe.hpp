// sgw_observe.hpp -- the derived-observation kernels: what the wrappers compute from a step's outputs, as launches of their own
// (k_engine uses none of them): derived statistics, RGB / layer planes, k_step_extras, agent views, agent layer views.
#pragma once

#include "sgw_kernels.hpp"      // view_unrotate

namespace sgw {

// ---- derived statistics (safety_game_mo.py:1027-1084) in numpy's summation order -----------------------------
// numpy pairwise_sum for a contiguous double array (umath loops): n < 8 sequential from 0.0; n <= 128 eight accumulators
// over blocks of 8, tree-combined, remainder added sequentially; larger n split once (n2 = n/2 rounded down to a
// multiple of 8: both halves <= 128 for n <= 256 = K * K outer differences, K <= 16).  Everything is unrolled at compile time
// for the agent's number of dimensions K (a switch over 1..16): the element index is a constant, so the vectors stay in
// registers and a sum over |d_i - d_j| needs no array of the K * K differences (round 2 kept one per thread: 2.6 KB of scratch
// per lane; a version that streamed the vectors from LDS at run-time indices was bound by serial LDS round trips, 23 us).
template <int T0, int N, class Get> __device__ __forceinline__ double np_block_c(Get& get) {
  if constexpr (N < 8) {
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) r += get(T0 + i);
    return r;
  } else {
    double r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = get(T0 + u);
#pragma unroll
    for (int i = 8; i < N - (N % 8); i += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] += get(T0 + i + u);
    }
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
    for (int i = N - (N % 8); i < N; ++i) res += get(T0 + i);
    return res;
  }
}
template <int N, class Get> __device__ __forceinline__ double np_sum_c(Get get) {
  if constexpr (N <= 128) return np_block_c<0, N>(get);
  else {
    constexpr int n2 = (N / 2) - ((N / 2) % 8);
    const double lo = np_block_c<0, n2>(get);
    return lo + np_block_c<n2, N - n2>(get);
  }
}
template <int K> __device__ __forceinline__ double np_gini100_c(const double (&v)[K]) {      // gini_coefficient(...) * 100 (1645-1681)
  double mn = v[0];
#pragma unroll
  for (int i = 1; i < K; ++i) mn = v[i] < mn ? v[i] : mn;                                   // python min()
  double d[K];
#pragma unroll
  for (int i = 0; i < K; ++i) d[i] = v[i] - mn;
  const double mad = np_sum_c<K * K>([&](int t) { return fabs(d[t / K] - d[t % K]); }) / (double)(K * K);
  const double rel = mad / (np_sum_c<K>([&](int i) { return d[i]; }) / (double)K + 2.220446049250313e-16);
  return 0.5 * rel * 100.0;
}
template <int K> __device__ __forceinline__ double np_var_c(const double (&v)[K]) {          // np.var(list, ddof=0)
  const double mean = np_sum_c<K>([&](int i) { return v[i]; }) / (double)K;
  double x[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { const double y = v[i] - mean; x[i] = y * y; }
  return np_sum_c<K>([&](int i) { return x[i]; }) / (double)K;
}
struct AgentK { int k[SGW_MAX_AGENTS]; };
// one agent's statistics for this lane's env: vectors from the transposed LDS rows into registers, results into the lane's
// output row in LDS
template <int K> __device__ __noinline__ void derived_agent(const double* Rv, const double* Cv, double denom, double* o, int Kout, int lane) {
  double r[K], c[K], avg[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { r[i] = Rv[i * WAVE + lane]; c[i] = Cv[i * WAVE + lane]; }
#pragma unroll
  for (int i = 0; i < K; ++i) avg[i] = c[i] / denom;
  o[0] = np_gini100_c<K>(r);
  o[1] = np_gini100_c<K>(c);
  o[2] = np_var_c<K>(r);
  o[3] = np_var_c<K>(c);
  o[4] = np_var_c<K>(avg);
#pragma unroll
  for (int j = 0; j < K; ++j) o[5 + j] = avg[j];
  for (int j = K; j < Kout; ++j) o[5 + j] = 0.0;
}
// One wave per 64 envs.  The wave's 64 x A rows of `reward` and `cumulative` are contiguous in global memory: they come in as
// 16-byte loads and are transposed through LDS as [agent][dimension][lane] (a lane then reads its own vector conflict-free);
// the wave's 64 x A x (5 + K) results are staged in LDS and leave as 16-byte stores.
// LDS (dynamic): R [A][K][64] | C [A][K][64] | O [64 * A * (5 + K)] doubles.
__device__ inline void derived_stats_wave(uint8_t* ds_lds, int lane, long long env0, int rows, const double* reward, const double* cumulative, const int* frame,
                                          long long n, int A, int K, const AgentK& ak, int recip_K, double* stats) {
  const long long env = env0 + lane;
  const int AK = A * K, S = 5 + K;
  double* R = reinterpret_cast<double*>(ds_lds);
  double* Cm = R + AK * WAVE;
  double* O = Cm + AK * WAVE;
  // ---- rows in: element e of the wave's block (row-major [64][A][K]) -> [agent * K + dim][lane]
  const long long rows_left = n - env0;
  const int nrow = rows_left < rows ? (int)rows_left : rows;        // a ragged last wave reads only its own rows (rows <= 64 per wave)
  const int nel = nrow * AK;
  const double* gr = reward + env0 * AK;
  const double* gc = cumulative + env0 * AK;
  for (int e0 = 2 * lane; e0 < WAVE * AK; e0 += 2 * WAVE) {
    double r0 = 0.0, r1 = 0.0, c0 = 0.0, c1 = 0.0;
    if (e0 + 1 < nel) {
      const double2 rv = *reinterpret_cast<const double2*>(gr + e0), cv = *reinterpret_cast<const double2*>(gc + e0);
      r0 = rv.x; r1 = rv.y; c0 = cv.x; c1 = cv.y;
    } else if (e0 < nel) { r0 = gr[e0]; c0 = gc[e0]; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = e0 + h;
      const int row = (e * recip_K) >> 18;                          // e / (A * K): exact for e < 64 * 64 (host-computed ceil(2^18 / (A K)))
      const int col = e - row * AK;
      R[col * WAVE + row] = h ? r1 : r0;
      Cm[col * WAVE + row] = h ? c1 : c0;
    }
  }
  const double denom = (double)(((env < n && lane < nrow) ? frame[env] : 0) + 1);
  lds_wave_sync();
  for (int ag = 0; ag < A; ++ag) {
    const double* Rv = R + ag * K * WAVE;
    const double* Cv = Cm + ag * K * WAVE;
    double* o = O + (lane * A + ag) * S;
    switch (ak.k[ag]) {                                             // uniform
#define SGW_DS_CASE(KK) case KK: derived_agent<KK>(Rv, Cv, denom, o, K, lane); break;
      SGW_DS_CASE(1) SGW_DS_CASE(2) SGW_DS_CASE(3) SGW_DS_CASE(4) SGW_DS_CASE(5) SGW_DS_CASE(6) SGW_DS_CASE(7) SGW_DS_CASE(8)
      SGW_DS_CASE(9) SGW_DS_CASE(10) SGW_DS_CASE(11) SGW_DS_CASE(12) SGW_DS_CASE(13) SGW_DS_CASE(14) SGW_DS_CASE(15) SGW_DS_CASE(16)
#undef SGW_DS_CASE
      default: {                                                    // an agent without reward dimensions (an absent slot)
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        o[0] = 0.0; o[1] = 0.0; o[2] = nan; o[3] = nan; o[4] = nan;
        for (int j = 0; j < K; ++j) o[5 + j] = 0.0;
      }
    }
  }
  lds_wave_sync();
  // ---- results out: the wave's nrow * A * S doubles are contiguous
  const int nout = nrow * A * S;
  double* g = stats + env0 * A * S;
  for (int e0 = 2 * lane; e0 < nout; e0 += 2 * WAVE) {
    if (e0 + 1 < nout) *reinterpret_cast<double2*>(g + e0) = *reinterpret_cast<const double2*>(O + e0);
    else g[e0] = O[e0];
  }
}
__global__ __launch_bounds__(WAVE) void k_derived_stats(const double* reward, const double* cumulative, const int* frame, long long n, int A, int K,
                                                        AgentK ak, int recip_K, double* stats) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ds_lds[];
  derived_stats_wave(ds_lds, (int)threadIdx.x, (long long)blockIdx.x * WAVE, WAVE, reward, cumulative, frame, n, A, K, ak, recip_K, stats);
}

// ---- per-character planes of a rendered board: RGB, occluded layers, unoccluded layers ---------------------------------------
// Every one of these outputs is [N][P planes][H*W] bytes with byte (e, p, c) a function of plane p and of what is at cell c of
// env e.  A workgroup takes 64 envs: their board rows (contiguous) come in as 16-byte loads into LDS, phase 1 reduces a cell to
// a CODE (the ascii code, or the bit mask of the layers that are on there), and phase 2 writes the block's 64 * P * HW
// contiguous output bytes 16 at a time -- a lane walks (env, plane, cell) forward by one from the chunk's first byte, whose
// coordinates come from two reciprocal multiplies, instead of dividing per byte.  (Round 2: one thread per cell, an integer
// division each, P one-byte stores at a stride of HW.)
constexpr int PLANES_THREADS = 256, PLANES_ENVS = 64;      // (PLANES_ENVS: the most envs a workgroup takes; 16 for boards whose staging would crowd the CU's LDS)
struct PlaneGeom { int HW, P, recip_HW, recip_Q; };       // recip_x = ceil(2^32 / x) as uint32: (f * recip) >> 32 == f / x for f < 64 x; Q = ceil(HW / 4)
// phase 2: a lane takes FOUR consecutive cells of an env, fetches their codes once and writes one dword per plane
// -- consecutive lanes write consecutive dwords of a row.  When H*W is not a multiple of 4 the rows do not start on dwords: the
// stores are then unaligned dword stores (global memory takes them; the bytes of a wave's instruction are contiguous all the
// same) and the last, partial group of a row leaves as single bytes.  dword4(e, c, nvalid, put): put(p, the 4 output bytes)
typedef uint32_t __attribute__((aligned(1))) sgw_u32_unaligned;
template <class Dword4>
__device__ inline void planes_expand4(uint8_t* out_block, const PlaneGeom& g, int n_env, Dword4 dword4) {
  const int HW = g.HW, q = (HW + 3) >> 2, items = n_env * q;
  for (int i = threadIdx.x; i < items; i += PLANES_THREADS) {
    const int e = (int)div_recip((uint32_t)i, (uint32_t)g.recip_Q), c = 4 * (i - e * q);
    const int nvalid = HW - c < 4 ? HW - c : 4;
    uint8_t* row = out_block + (size_t)e * g.P * HW + c;
    dword4(e, c, nvalid, [&](int p, uint32_t v) {
      uint8_t* d = row + (size_t)p * HW;
      if (nvalid == 4) {
#if defined(__HIP_DEVICE_COMPILE__)
        // ONE dword store at a byte address (the compiler splits a store it cannot prove aligned into four byte stores; the memory
        // pipeline takes unaligned dwords: the tests compare every byte with the fixtures)
        asm volatile("global_store_dword %0, %1, off" : : "v"(d), "v"(v) : "memory");
#else
        *reinterpret_cast<sgw_u32_unaligned*>(d) = v;
#endif
      } else for (int b = 0; b < nvalid; ++b) d[b] = (uint8_t)(v >> (8 * b));
    });
  }
}
// four consecutive LDS bytes at any alignment (cells past the row's end read the row's last cell: their output is dropped)
__device__ inline uint32_t lds_bytes4(const uint8_t* base, int at, int nvalid) {
  const int i1 = nvalid > 1 ? 1 : 0, i2 = nvalid > 2 ? 2 : i1, i3 = nvalid > 3 ? 3 : i2;
  return (uint32_t)base[at] | ((uint32_t)base[at + i1] << 8) | ((uint32_t)base[at + i2] << 16) | ((uint32_t)base[at + i3] << 24);
}
// the block's board rows -> LDS (16-byte loads; 64 * HW is a multiple of 16 and the block starts on one)
__device__ inline void planes_load_boards(const uint8_t* board, long long env0, int n_env, int HW, uint8_t* lds_board) {
  const uint4* src = reinterpret_cast<const uint4*>(board + env0 * HW);
  const int bytes = n_env * HW, n16 = (reinterpret_cast<uintptr_t>(board) & 15) ? 0 : bytes >> 4;      // a caller's unaligned slice: bytes
  for (int j = threadIdx.x; j < n16; j += PLANES_THREADS) reinterpret_cast<uint4*>(lds_board)[j] = src[j];
  for (int j = (n16 << 4) + threadIdx.x; j < bytes; j += PLANES_THREADS) lds_board[j] = board[env0 * HW + j];     // ragged last block
}

// the RGB planes of a block's boards (in LDS) through the colour table tab[plane][char] (in LDS)
__device__ inline void observe_rgb_expand(const uint8_t* bl, const uint8_t* tab, uint8_t* rgb_block, const PlaneGeom& g_rgb, int n_env) {
  const int HW = g_rgb.HW;
  planes_expand4(rgb_block, g_rgb, n_env, [&](int e, int c, int nvalid, auto put) {
    const uint32_t b4 = (HW & 3) == 0 ? *reinterpret_cast<const uint32_t*>(bl + e * HW + c) : lds_bytes4(bl, e * HW + c, nvalid);
    const uint32_t c0 = b4 & 0x7f, c1 = (b4 >> 8) & 0x7f, c2 = (b4 >> 16) & 0x7f, c3 = (b4 >> 24) & 0x7f;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const uint8_t* t = tab + p * 128;
      put(p, (uint32_t)t[c0] | ((uint32_t)t[c1] << 8) | ((uint32_t)t[c2] << 16) | ((uint32_t)t[c3] << 24));
    }
  });
}

// observation distiller extras from an ascii board (observation_distiller.py:30-91, rendering.py:69-185): RGB planes via the
// colour LUT and OCCLUDED per-character layers (board == char).  LDS: boards [64 * HW] | table [P][128]
__global__ __launch_bounds__(PLANES_THREADS) void k_observe(const uint8_t* board, long long n, int epb, PlaneGeom g_rgb, const uint8_t* rgb_lut, uint8_t* rgb,
                                                            PlaneGeom g_lay, const uint8_t* layer_chars, uint8_t* layers) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pl_lds[];
  const int HW = g_rgb.HW;
  const long long env0 = (long long)blockIdx.x * epb;              // epb envs per workgroup: 64, or 16 for large boards (LDS per workgroup)
  const int n_env = n - env0 < epb ? (int)(n - env0) : epb;
  uint8_t* bl = pl_lds;
  uint8_t* tab = pl_lds + ((epb * HW + 15) & ~15);
  planes_load_boards(board, env0, n_env, HW, bl);
  if (rgb) {
    for (int i = threadIdx.x; i < 3 * 128; i += PLANES_THREADS) tab[i] = rgb_lut[(i & 127) * 3 + (i >> 7)];        // [plane][char]
    __syncthreads();
    observe_rgb_expand(bl, tab, rgb + env0 * 3 * HW, g_rgb, n_env);
  }
  if (layers) {
    __syncthreads();
    for (int i = threadIdx.x; i < g_lay.P; i += PLANES_THREADS) tab[i] = layer_chars[i];
    __syncthreads();
    planes_expand4(layers + env0 * g_lay.P * HW, g_lay, n_env, [&](int e, int c, int nvalid, auto put) {
      const uint32_t b4 = ((HW & 3) == 0 ? *reinterpret_cast<const uint32_t*>(bl + e * HW + c) : lds_bytes4(bl, e * HW + c, nvalid)) & 0x7f7f7f7fu;
      for (int p = 0; p < g_lay.P; ++p) put(p, bytes_equal_mask(b4, 0x01010101u * tab[p]) & 0x01010101u);
    });
  }
}

// unoccluded layers + gap correction (rendering.py:188-302, observation_distiller_ex.py:164-178).  Phase 1 reduces cell (e, c)
// to the bit mask of the layers that are on there: a dynamic layer (stat 2: sprite / moving drape) where the board shows its
// character, a static curtain (stat 1) always, the hidden drape under an agent that covers it (firemaker's fire), and the
// what_lies_beneath layer only where every other layer is blank.  LDS: boards [64 * HW] | masks u32 [64 * HW] | per-cell tables
// dyn u32 [HW], on u32 [HW] | per-char table u32 [128]
__device__ inline void observe_layers_block(uint8_t* pl_lds, long long env0, int epb, bool boards_loaded, const uint8_t* board, long long n, PlaneGeom g, int W,
                                            const uint8_t* chars, const uint8_t* stat, int gap, const uint8_t* pos, const uint8_t* flags, int A,
                                            int hidden, uint8_t* layers) {
  const int HW = g.HW, L = g.P;
  const int n_env = n - env0 < epb ? (int)(n - env0) : epb;
  uint8_t* bl = pl_lds;
  uint32_t* mask = reinterpret_cast<uint32_t*>(pl_lds + ((epb * HW + 15) & ~15));
  uint32_t* dyn = mask + epb * HW;
  uint32_t* on = dyn + HW;
  uint32_t* chm = on + HW;
  if (!boards_loaded) planes_load_boards(board, env0, n_env, HW, bl);
  for (int c = threadIdx.x; c < HW; c += PLANES_THREADS) {
    uint32_t d = 0u, o = 0u;
    for (int k = 0; k < L; ++k) { const uint8_t st = stat[k * HW + c]; d |= (st == 2 ? 1u : 0u) << k; o |= ((st != 0 && st != 2) ? 1u : 0u) << k; }
    dyn[c] = d; on[c] = o;
  }
  for (int ch = threadIdx.x; ch < 128; ch += PLANES_THREADS) {
    uint32_t m = 0u;
    for (int k = 0; k < L; ++k) m |= (chars[k] == ch ? 1u : 0u) << k;
    chm[ch] = m;
  }
  __syncthreads();
  const uint32_t gapbit = gap >= 0 ? 1u << gap : 0u;
  for (int i = threadIdx.x; i < n_env * HW; i += PLANES_THREADS) {
    const int e = (int)div_recip((uint32_t)i, (uint32_t)g.recip_HW), c = i - e * HW;
    mask[i] = ((chm[bl[i] & 0x7f] & dyn[c]) | on[c]) & ~gapbit;      // the gap layer is decided below
  }
  __syncthreads();
  if (pos && hidden >= 0) {                                           // the hidden drape under an agent's sprite
    for (int i = threadIdx.x; i < n_env * A; i += PLANES_THREADS) {
      const long long ea = env0 * A + i;
      const int e = i / A;
      if (flags[ea] & 1) atomicOr(&mask[e * HW + (int)pos[ea * 2] * W + (int)pos[ea * 2 + 1]], 1u << hidden);
    }
    __syncthreads();
  }
  if (gap >= 0) {
    for (int i = threadIdx.x; i < n_env * HW; i += PLANES_THREADS) {
      const int e = (int)div_recip((uint32_t)i, (uint32_t)g.recip_HW), c = i - e * HW;
      const uint32_t m = mask[i];
      const bool gap_static = ((on[c] | dyn[c]) & gapbit) != 0u;              // the layer's curtain entry is not 0
      if (gap_static && (m & ~gapbit) == 0u) mask[i] = m | gapbit;
    }
    __syncthreads();
  }
  planes_expand4(layers + env0 * L * HW, g, n_env, [&](int e, int c, int nvalid, auto put) {
    uint4 m;                                                         // the four cells' layer masks
    if ((HW & 3) == 0) m = *reinterpret_cast<const uint4*>(mask + e * HW + c);      // one 16-byte LDS read
    else {
      const uint32_t* mp = mask + e * HW + c;
      m = make_uint4(mp[0], mp[nvalid > 1 ? 1 : 0], mp[nvalid > 2 ? 2 : 0], mp[nvalid > 3 ? 3 : 0]);
    }
    for (int p = 0; p < L; ++p)
      put(p, ((m.x >> p) & 1u) | (((m.y >> p) & 1u) << 8) | (((m.z >> p) & 1u) << 16) | (((m.w >> p) & 1u) << 24));
  });
}
__global__ __launch_bounds__(PLANES_THREADS) void k_observe_layers(const uint8_t* board, long long n, int epb, PlaneGeom g, int W, const uint8_t* chars,
                                                                   const uint8_t* stat, int gap, const uint8_t* pos, const uint8_t* flags, int A,
                                                                   int hidden, uint8_t* layers) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pl_lds[];
  observe_layers_block(pl_lds, (long long)blockIdx.x * epb, epb, false, board, n, g, W, chars, stat, gap, pos, flags, A, hidden, layers);
}

// ---- sgw_step_full's board-derived outputs in ONE launch: a workgroup takes `epb` envs of the step that just ran and produces, from
// their boards (loaded into LDS once), the RGB planes and the unoccluded layers, then the performance bookkeeping and the `done`
// flags of those envs: one kernel boundary and one graph node instead of three.
struct ExtrasArgs {
  const uint8_t* board; long long n; int epb, HW, W, A, K;
  PlaneGeom g_rgb; const uint8_t* rgb_lut; uint8_t* rgb;
  PlaneGeom g_lay; const uint8_t* chars; const uint8_t* stat; int gap, hidden; const uint8_t* pos; const uint8_t* flags; uint8_t* layers;
  const double* reward; const double* cumulative; const int* frame; AgentK ak; int recip_K; double* stats;
  const double* perf; int perf_cols, per_agent; const uint8_t* step_type; double* last; double* sum; long long* count; uint8_t* done;
  int lds_planes;                                   // bytes of the planes region (the statistics' rows follow it)
};
// _episodic_performances bookkeeping per env (safety_game.py:194-263): at a LAST timestep (episode_ended, sgw_common.hpp) the
// episode's performance becomes the env's last performance and joins its running sum and count
__device__ inline void track_performance_item(long long i, const double* perf, int C, const uint8_t* step_type, int A, int per_agent, double* last,
                                              double* sum, long long* count, uint8_t* done_out) {
  const long long e = i / C;
  const bool done = episode_ended(step_type + e * A, A, per_agent);
  if (done_out && i == e * C) done_out[e] = done ? 1 : 0;
  if (!done) return;
  const double v = perf[i];
  if (last) last[i] = v;
  if (sum) sum[i] += v;
  if (count && i == e * C) count[e] += 1;
}
__global__ void k_track_performance(const double* perf, int C, const uint8_t* step_type, int A, int per_agent, long long n, double* last,
                                    double* sum, long long* count, uint8_t* done_out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * C) track_performance_item(i, perf, C, step_type, A, per_agent, last, sum, count, done_out);
}
__global__ __launch_bounds__(PLANES_THREADS) void k_step_extras(const ExtrasArgs x) {
  extern __shared__ __attribute__((aligned(16))) uint8_t pl_lds[];
  const long long env0 = (long long)blockIdx.x * x.epb;
  const int n_env = x.n - env0 < x.epb ? (int)(x.n - env0) : x.epb;
  const bool planes = x.rgb != nullptr || x.layers != nullptr;
  if (planes) planes_load_boards(x.board, env0, n_env, x.HW, pl_lds);
  if (x.rgb) {
    uint8_t* tab = pl_lds + x.lds_planes - 3 * 128;               // the colour table sits at the end of the planes region
    for (int i = threadIdx.x; i < 3 * 128; i += PLANES_THREADS) tab[i] = x.rgb_lut[(i & 127) * 3 + (i >> 7)];
    __syncthreads();
    observe_rgb_expand(pl_lds, tab, x.rgb + env0 * 3 * x.HW, x.g_rgb, n_env);
  }
  if (x.layers) {
    __syncthreads();
    observe_layers_block(pl_lds, env0, x.epb, true, x.board, x.n, x.g_lay, x.W, x.chars, x.stat, x.gap, x.pos, x.flags, x.A, x.hidden, x.layers);
  }
  // (the derived statistics stay a launch of their own: their unrolled K = 16 body needs ~290 registers, and compiled into this
  // kernel that budget applied to every wave -- one workgroup per CU, 83 instead of 54 us per full step)
  if (x.perf) {
    for (long long i = env0 * x.perf_cols + (int)threadIdx.x; i < (env0 + n_env) * x.perf_cols; i += PLANES_THREADS)
      track_performance_item(i, x.perf, x.perf_cols, x.step_type, x.A, x.per_agent, x.last, x.sum, x.count, x.done);
  }
}

// agent-centric windows of the rendered board (safety_game_moma.py:1996-2101), one thread per output byte
struct ViewSpec { int A, H, W, total; int off[SGW_MAX_AGENTS], up[SGW_MAX_AGENTS], left[SGW_MAX_AGENTS], vh[SGW_MAX_AGENTS], vw[SGW_MAX_AGENTS]; };
// (view_unrotate: above, with the in-kernel windows)
// One WAVE produces one agent's window of one env.  The lanes cover whole window rows (64 / vw rows per pass, one byte per lane) and
// read contiguous board cells (a board row, or a column when the window is rotated); the window is assembled in LDS at the same
// 16-byte phase as its place in the output and leaves as 16-byte stores (head and tail bytes singly): window bytes are not
// aligned to anything (1 139 bytes per firemaker env), and byte-masked partial-line writes were what the earlier versions
// were waiting for.  History (16 384 firemaker envs x 1 139 window bytes): one thread per output byte with its own divisions,
// 46 us; one thread per window row, 49 us; one wave per window with byte stores, 42-44 us.
__device__ inline void view_wave(const uint8_t* src, uint8_t* dst, uint8_t* lds, int H, int W, int vh, int vw, int pr, int pc, int dir,
                                 bool rotate, uint8_t pad, int lane) {
  const int len = vh * vw;
  const int phase = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
  uint8_t* stage = lds + phase;                                   // stage[j] and dst[j] share their 16-byte alignment
  if (len > H * W && vw <= 255) {
    // a window LARGER than the board (firemaker's supervisor: 33 x 33 around a 17 x 17 board) is mostly padding: fill the stage
    // with the pad byte (16-byte LDS stores), then walk the BOARD cells once and drop each where it lands in the window
    const uint32_t p4 = 0x01010101u * pad;
    const uint4 fill = make_uint4(p4, p4, p4, p4);
    for (int k = lane; k < (phase + len + 15) >> 4; k += WAVE) reinterpret_cast<uint4*>(lds)[k] = fill;
    lds_wave_sync();
    const int cells = H * W;
    for (int k0 = 0; k0 < cells; k0 += 4 * WAVE) {                 // four loads in flight
      uint8_t val[4]; int at[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + q * WAVE + lane;
        const bool in_board = k < cells;
        val[q] = src[in_board ? k : 0];
        const int r = k / W, c = k - r * W;
        const int cr = r - pr, cc = c - pc;                       // crop coordinates
        int vr = cr, vc = cc;                                     // inverse of view_unrotate
        if (rotate) {
          if (dir == 3) { vr = vw - 1 - cr; vc = vw - 1 - cc; }
          else if (dir == 0) { vr = cc; vc = vw - 1 - cr; }
          else if (dir == 1) { vr = vw - 1 - cc; vc = cr; }
        }
        at[q] = (in_board && cr >= 0 && cr < vh && cc >= 0 && cc < vw) ? vr * vw + vc : -1;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) if (at[q] >= 0) stage[at[q]] = val[q];
    }
  } else if (vw > WAVE) {                                         // wider than a wave: plain column chunks (no reference env is)
    for (int vr = 0; vr < vh; ++vr)
      for (int vc = lane; vc < vw; vc += WAVE) {
        int r = vr, c = vc;
        if (rotate) view_unrotate(dir, vw, r, c);
        r += pr; c += pc;
        stage[vr * vw + vc] = (r < 0 || r >= H || c < 0 || c >= W) ? pad : src[r * W + c];
      }
  } else {
    const int rpg = WAVE / vw;                                    // window rows per pass
    const int lr = lane / vw, lc = lane - lr * vw;
    const bool lane_on = lr < rpg;
    for (int vr0 = 0; vr0 < vh; vr0 += 4 * rpg) {                 // four passes in flight: loads first, LDS writes after
      uint8_t val[4]; bool on[4]; int at[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int vr = vr0 + k * rpg + lr;
        on[k] = lane_on && vr < vh;
        int r = on[k] ? vr : 0, c = lc;
        if (rotate) view_unrotate(dir, vw, r, c);
        r += pr; c += pc;
        const bool inside = !(r < 0 || r >= H || c < 0 || c >= W);
        const uint8_t got = src[inside ? r * W + c : 0];           // unconditional load (index clamped), selected afterwards
        val[k] = inside ? got : pad;
        at[k] = vr * vw + lc;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) if (on[k]) stage[at[k]] = val[k];
    }
  }
  lds_wave_sync();
  const int head = (16 - phase) & 15;                             // bytes up to the first 16-byte boundary of the output
  const int nh = head < len ? head : len;
  if (lane < nh) dst[lane] = stage[lane];
  const int body = (len - nh) >> 4;                               // whole 16-byte chunks
  for (int k = lane; k < body; k += WAVE)
    *reinterpret_cast<uint4*>(dst + nh + 16 * k) = *reinterpret_cast<const uint4*>(stage + nh + 16 * k);
  const int done = nh + 16 * body;
  if (lane < len - done) dst[done + lane] = stage[done + lane];
  lds_wave_sync();                                                // the next window of this wave reuses the stage
}
__global__ void k_agent_views(const uint8_t* board, const uint8_t* pos, const uint8_t* flags, long long n, ViewSpec v,
                              uint8_t outside, uint8_t* views, int lds_per_wave) {
  extern __shared__ __attribute__((aligned(16))) uint8_t view_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  uint8_t* lds = view_lds + (threadIdx.x >> 6) * lds_per_wave;
  const long long stride = ((long long)gridDim.x * blockDim.x) >> 6, windows = n * v.A;
  for (long long wv = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < windows; wv += stride) {
    const long long e = wv / v.A;
    const int ag = (int)(wv - e * v.A);
    if (v.vh[ag] * v.vw[ag] == 0) continue;                      // an agent without a window (absent firemaker agents)
    const int pr = (int)pos[wv * 2] - v.up[ag], pc = (int)pos[wv * 2 + 1] - v.left[ag];
    const int dir = flags ? (flags[wv] >> 3) & 3 : 2;
    view_wave(board + e * (long long)(v.H * v.W), views + e * v.total + v.off[ag], lds, v.H, v.W, v.vh[ag], v.vw[ag], pr, pc, dir,
              flags != nullptr, outside, lane);
  }
}

// Small windows (every window <= 64 cells, e.g. the 5 x 5 windows of island_navigation_ex_ma): a wave per window would leave most
// lanes idle (131 072 waves for 65 536 two-agent envs); one thread per output byte keeps the stores contiguous across lanes
// and costs ~60 instructions per 64 bytes.  `per_env` = bytes per env (window bytes x layers for the layer variant).
__device__ inline uint8_t small_view_byte(const uint8_t* src_env, const uint8_t* pos, const uint8_t* flags, const ViewSpec& v,
                                          uint8_t pad, long long e, int ag, int cellidx) {
  const int vw = v.vw[ag];
  int vr = cellidx / vw, vc = cellidx - vr * vw;
  const long long ea = e * v.A + ag;
  if (flags) view_unrotate((flags[ea] >> 3) & 3, vw, vr, vc);
  const int r = (int)pos[ea * 2] - v.up[ag] + vr, c = (int)pos[ea * 2 + 1] - v.left[ag] + vc;
  return (r < 0 || r >= v.H || c < 0 || c >= v.W) ? pad : src_env[r * v.W + c];
}
__global__ void k_agent_views_small(const uint8_t* board, const uint8_t* pos, const uint8_t* flags, long long n, ViewSpec v,
                                    uint8_t outside, uint8_t* views) {
  const long long total = n * v.total;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i / v.total;
    int b = (int)(i - e * v.total), ag = 0;
#pragma unroll
    for (int k = 1; k < SGW_MAX_AGENTS; ++k) if (k < v.A && b >= v.off[k]) ag = k;
    views[i] = small_view_byte(board + e * (long long)(v.H * v.W), pos, flags, v, outside, e, ag, b - v.off[ag]);
  }
}
__global__ void k_agent_layer_views_small(const uint8_t* layers, const uint8_t* pos, const uint8_t* flags, long long n, ViewSpec v,
                                          const uint8_t* chars, int L, uint8_t outside, uint8_t* out) {
  const long long per_env = (long long)v.total * L, total = n * per_env;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long e = i / per_env;
    int b = (int)(i - e * per_env), ag = 0;
#pragma unroll
    for (int k = 1; k < SGW_MAX_AGENTS; ++k) if (k < v.A && b >= v.off[k] * L) ag = k;
    b -= v.off[ag] * L;
    const int cells = v.vh[ag] * v.vw[ag];
    const int li = b / cells;
    out[i] = small_view_byte(layers + (e * L + li) * (long long)(v.H * v.W), pos, flags, v, (uint8_t)(chars[li] == outside), e, ag,
                             b - li * cells);
  }
}

// per-layer agent windows, windows larger than 64 cells (firemaker's 33 x 33, savanna's 21 x 21): a WORKGROUP takes G envs at a
// time.  Their L layer planes come into LDS, each of the A x L windows of an env is assembled in an LDS image of the env's whole
// output row by one wave (a window larger than the plane: pad fill, then the plane's cells dropped where they land; else a
// gather), and the rows leave as dword stores at their byte address (rows of L * view_bytes bytes are not aligned to anything).
// Why G envs at once: an env is a chain of dependent waits -- planes and positions from global memory, the LDS passes, and the
// next env's loads queue behind this env's stores (vmcnt counts both) -- about 8 us per env whatever its size; with one env per
// wave (the L = 1 form: sgw_agent_views) a CU had 32 such chains in flight and 16 384 firemaker envs took 17.5 us, 65 536
// savanna envs 60 us.  G envs share every wait of the chain.  Round 2's kernel below -- one wave per window, every cell a byte
// load from global memory -- took 208 us for 16 384 firemaker envs' layer cubes (0.13 of HBM).
template <int G>
__global__ __launch_bounds__(256) void k_agent_layer_views_lds(const uint8_t* layers, const uint8_t* pos, const uint8_t* flags, long long n, ViewSpec v,
                                                               const uint8_t* chars, int L, uint8_t outside, uint8_t* out, int lay_bytes, int img_bytes,
                                                               int pad_is_char) {
  // pad_is_char: the planes are ascii boards (L = 1: sgw_agent_views) and cells outside the board read `outside` itself; otherwise
  // they are layer planes and read 1 on the outside character's own layer (agent_perspectives_with_layers)
  // LDS: [ per-agent table: off, up, left, vh, vw x 4 | per-env words of the group: row | col << 8 | flags << 16, x G x 4 |
  //        G x ( [L][H*W] planes | the env's output row [agent][layer][vh][vw] at its 16-byte phase ) ]
  // What a loop indexes at run time (the agent's window, the env's position) is READ from LDS: as members of the kernel
  // argument / as register arrays they became select chains over every agent and env -- 2 200 scalar and 420 spill
  // instructions, 400 branches in the first G-env version, and the kernel was bound by exactly that (75 us for savanna's
  // 65 536 envs, 26 of them with loads, assembly and stores all switched off).
  extern __shared__ __attribute__((aligned(16))) uint8_t view_lds[];
  int* tab = reinterpret_cast<int*>(view_lds);
  uint32_t* ppos = reinterpret_cast<uint32_t*>(view_lds + 128);
  uint8_t* envs = view_lds + 128 + 16 * G;
  const int env_lds = lay_bytes + img_bytes;
  const int HW = v.H * v.W, H = v.H, W = v.W, A = v.A, lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int row_bytes = v.total * L;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < SGW_MAX_AGENTS; ++k) { tab[k] = v.off[k] * L; tab[4 + k] = v.up[k]; tab[8 + k] = v.left[k]; tab[12 + k] = v.vh[k]; tab[16 + k] = v.vw[k]; }
  }
  // lane constants, once per kernel (no division inside the env loop): the plane cells this lane drops into a large window
  // (cell k = lane + 64 j: row, column)
  constexpr int NP = (SGW_MAX_CELLS + WAVE - 1) / WAVE;
  int prr[NP], pcc[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) { const int k = lane + WAVE * j; prr[j] = k / W; pcc[j] = k - prr[j] * W; }
  bool inb[NP];                                             // plane cell lane + 64 j exists
#pragma unroll
  for (int j = 0; j < NP; ++j) inb[j] = lane + WAVE * j < HW;
  uint8_t* const trash = view_lds + 124;                    // where the scatter's out-of-window cells land (no exec juggling per store)
  constexpr int PF = G > 1 ? 5 : 12;                        // plane bytes per thread held in registers between the load and the LDS write
  const int nbytes = L * HW;
  const bool in_regs = nbytes <= PF * (int)blockDim.x;
  for (long long e0 = (long long)blockIdx.x * G; e0 < n; e0 += (long long)gridDim.x * G) {
    // ---- every load of the G envs first: planes (into registers), positions and flags (a lane per (env, agent))
    uint32_t pl[G][PF];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const long long e = e0 + g < n ? e0 + g : n - 1;       // (a ragged last group re-reads the last env; nothing of it is stored)
      const uint8_t* src = layers + e * (long long)nbytes;
      if (in_regs) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          const int idx = (int)threadIdx.x + j * (int)blockDim.x;
          pl[g][j] = idx < nbytes ? src[idx] : 0u;
        }
      }
    }
    if ((int)threadIdx.x < 4 * G) {
      const int g = threadIdx.x >> 2, ag = threadIdx.x & 3;
      const long long e = e0 + g < n ? e0 + g : n - 1;
      uint32_t w = 16u << 16;                                  // (no flags: observation direction UP)
      if (ag < A) {
        const long long ea = e * A + ag;
        w = (uint32_t)*reinterpret_cast<const uint16_t*>(pos + ea * 2) | ((flags ? (uint32_t)flags[ea] : 16u) << 16);
      }
      ppos[threadIdx.x] = w;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      uint8_t* lay = envs + g * env_lds;
      if (pad_is_char) {                                       // ascii planes: one pad character for every window of the row -- the whole
        uint32_t* im4 = reinterpret_cast<uint32_t*>(lay + lay_bytes);      // image (its phase slack included) is filled here, once
        for (int k = threadIdx.x; k < (img_bytes >> 2); k += blockDim.x) im4[k] = 0x01010101u * outside;
      }
      if (in_regs) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
          const int idx = (int)threadIdx.x + j * (int)blockDim.x;
          if (idx < nbytes) lay[idx] = (uint8_t)pl[g][j];
        }
      } else {
        const long long e = e0 + g < n ? e0 + g : n - 1;
        const uint8_t* src = layers + e * (long long)nbytes;
        for (int i = threadIdx.x; i < nbytes; i += blockDim.x) lay[i] = src[i];
      }
    }
    __syncthreads();
    // ---- the windows of the G envs into their LDS images: agent by agent, so that what only depends on the agent's window
    // (the landing constants of the plane cells) is worked out once for the G envs
    for (int ag = 0; ag < A; ++ag) {                           // scalar loops: agent, env of the group, then this wave's layers
      const int vh = __builtin_amdgcn_readfirstlane(tab[12 + ag]), vw = __builtin_amdgcn_readfirstlane(tab[16 + ag]), cells = vh * vw;
      if (cells == 0) continue;
      const int up = __builtin_amdgcn_readfirstlane(tab[4 + ag]), left = __builtin_amdgcn_readfirstlane(tab[8 + ag]);
      const int off = __builtin_amdgcn_readfirstlane(tab[ag]), n1 = vw - 1;
      const bool big = cells > HW;
      const bool covers = up >= H - 1 && vh - 1 - up >= H - 1 && left >= W - 1 && vw - 1 - left >= W - 1;
      int P[NP], Q[NP];                                        // landing offset of plane cell (r, c): +-(r * n + c) or +-(c * n - r) plus an env scalar
#pragma unroll
      for (int j = 0; j < NP; ++j) { P[j] = prr[j] * vw + pcc[j]; Q[j] = pcc[j] * vw - prr[j]; }
#pragma nounroll
      for (int g = 0; g < G; ++g) {
        const uint8_t* lay = envs + g * env_lds;
        // the image sits at the 16-byte phase of its row in global memory, so that the row's aligned 16-byte chunks are aligned in
        // LDS too (img_bytes has 16 bytes of slack for it)
        const long long eg = e0 + g < n ? e0 + g : n - 1;
        uint8_t* img = envs + g * env_lds + lay_bytes + (int)(reinterpret_cast<uintptr_t>(out + eg * (long long)row_bytes) & 15);
        const uint32_t pw = (uint32_t)__builtin_amdgcn_readfirstlane((int)ppos[g * 4 + ag]);
        const int pr = (int)(pw & 0xffu) - up, pc = (int)((pw >> 8) & 0xffu) - left;
        const int dir = (int)((pw >> 19) & 3u);
        if (big) {
          const int base = dir == 2 ? -(pr * vw + pc) : (dir == 3 ? (n1 + pr) * vw + n1 + pc : (dir == 0 ? n1 + pr - pc * vw : (n1 + pc) * vw - pr));
          const bool useQ = dir < 2, neg = dir == 3 || dir == 1;
          int at[NP]; bool ok[NP];
#pragma unroll
          for (int j = 0; j < NP; ++j) {
            const int t = useQ ? Q[j] : P[j];
            at[j] = (neg ? -t : t) + base;
            ok[j] = inb[j];
            if (!covers) ok[j] = ok[j] && (unsigned)(prr[j] - pr) < (unsigned)vh && (unsigned)(pcc[j] - pc) < (unsigned)vw;
          }
          for (int l = wave; l < L; l += nwave) {
            const uint32_t pad = pad_is_char ? 0x01010101u * outside : (chars[l] == outside ? 0x01010101u : 0u);
            const uint8_t* plane = lay + l * HW;
            uint8_t* dst = img + off + l * cells;
            if (!pad_is_char) {
              // pad fill: bytes up to the first dword boundary, dwords, tail bytes (dst is byte-aligned only)
              const int head = (int)((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3), nh = head < cells ? head : cells;
              if (lane < nh) dst[lane] = (uint8_t)pad;
              uint32_t* d4 = reinterpret_cast<uint32_t*>(dst + nh);
              const int nd = (cells - nh) >> 2;
              for (int k = lane; k < nd; k += WAVE) d4[k] = pad;
              const int done = nh + 4 * nd;
              if (lane < cells - done) dst[done + lane] = (uint8_t)pad;
              lds_wave_sync();
            }
            uint8_t val[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) val[j] = plane[ok[j] ? lane + WAVE * j : 0];
#pragma unroll
            for (int j = 0; j < NP; ++j) *(ok[j] ? dst + at[j] : trash) = val[j];
          }
        } else {
          for (int l = wave; l < L; l += nwave) {
            const uint8_t pad = pad_is_char ? outside : (uint8_t)(chars[l] == outside);
            const uint8_t* plane = lay + l * HW;
            uint8_t* dst = img + off + l * cells;
            for (int k = lane; k < cells; k += WAVE) {
              int vr = k / vw, vc = k - vr * vw;
              view_unrotate(dir, vw, vr, vc);
              const int r = vr + pr, c = vc + pc;
              dst[k] = ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) ? plane[r * W + c] : pad;
            }
          }
        }
      }
    }
    __syncthreads();
    // ---- the G rows out
#pragma nounroll
    for (int g = 0; g < G; ++g) {
      if (e0 + g < n) {
        uint8_t* gp = out + (e0 + g) * (long long)row_bytes;
        const int phase = (int)(reinterpret_cast<uintptr_t>(gp) & 15);
        const uint8_t* img = envs + g * env_lds + lay_bytes + phase;
        // head bytes up to the first 16-byte boundary, aligned 16-byte chunks, tail bytes
        const int head = ((16 - phase) & 15) < row_bytes ? ((16 - phase) & 15) : row_bytes;
        const int nq = (row_bytes - head) >> 4, done = head + 16 * nq;
        if ((int)threadIdx.x < head) gp[threadIdx.x] = img[threadIdx.x];
        for (int q = threadIdx.x; q < nq; q += blockDim.x)
          *reinterpret_cast<uint4*>(gp + head + 16 * q) = *reinterpret_cast<const uint4*>(img + head + 16 * q);
        if ((int)threadIdx.x < row_bytes - done) gp[done + threadIdx.x] = img[done + threadIdx.x];
      }
    }
    __syncthreads();                                         // the next group reuses the planes and the images
  }
}

// per-layer agent windows: out[e][agent][layer][vr][vc]; one wave per (env, agent, layer)
__global__ void k_agent_layer_views(const uint8_t* layers, const uint8_t* pos, const uint8_t* flags, long long n, ViewSpec v,
                                    const uint8_t* chars, int L, uint8_t outside, uint8_t* out, int lds_per_wave) {
  extern __shared__ __attribute__((aligned(16))) uint8_t view_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  uint8_t* lds = view_lds + (threadIdx.x >> 6) * lds_per_wave;
  const long long stride = ((long long)gridDim.x * blockDim.x) >> 6, windows = n * v.A * L;
  for (long long wv = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wv < windows; wv += stride) {
    const long long ea = wv / L;                                 // env * A + agent
    const int li = (int)(wv - ea * L);
    const long long e = ea / v.A;
    const int ag = (int)(ea - e * v.A);
    if (v.vh[ag] * v.vw[ag] == 0) continue;
    const int pr = (int)pos[ea * 2] - v.up[ag], pc = (int)pos[ea * 2 + 1] - v.left[ag];
    const int dir = flags ? (flags[ea] >> 3) & 3 : 2;
    const int cells = v.vh[ag] * v.vw[ag];
    view_wave(layers + (e * L + li) * (long long)(v.H * v.W), out + e * ((long long)v.total * L) + (long long)v.off[ag] * L + (long long)li * cells,
              lds, v.H, v.W, v.vh[ag], v.vw[ag], pr, pc, dir, flags != nullptr, (uint8_t)(chars[li] == outside), lane);
  }
}

}  // namespace sgw
