// sgw_kernels.hpp -- the generic batched engine kernels, templated on a game family F.
//
// k_engine<F> covers sgw_reset (mode RESET), sgw_step (T = 1) and sgw_rollout (T > 1, state kept
// in registers across steps).  Restates, for 64 envs per wave in lockstep:
//   Environment.step auto-reset + max_iterations   pycolab_interface{,_mo}.py:147-192 / 157-196, 292-319
//   _process_timestep: episode return, termination reason default   safety_game.py:265-304,
//                                                                    safety_game_mo.py:971-1066
#pragma once

#include <cstddef>
#include <type_traits>

#include "sgw_common.hpp"
#include "sgw_pcg64.hpp"
#include "sgw_pow.hpp"

namespace sgw {

constexpr int TERM_NONE4 = 15;   // 4-bit in-state encoding of "termination_reason key absent"

template <class F, class = void> struct has_idle_round : std::false_type {};
template <class F> struct has_idle_round<F, std::void_t<decltype(&F::idle_round)>> : std::true_type {};
template <class F, class = void> struct has_safety2 : std::false_type {};     // environment_data['safety2_<agent>'] (aintelope_savanna)
template <class F> struct has_safety2<F, std::void_t<decltype(&F::agent_safety2)>> : std::true_type {};
// families that work out every agent's safety value in one pass
template <class F, class = void> struct has_safety_all : std::false_type {};
template <class F> struct has_safety_all<F, std::void_t<decltype(&F::agent_safety_all)>> : std::true_type {};
template <class F>
__device__ inline void agent_safeties(const typename F::State& s, const KSpec& sp, const Lds& l, int (&out)[F::NA]) {
  if constexpr (has_safety_all<F>::value) {
    F::agent_safety_all(s, sp, l, out);
  } else {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) out[ag] = F::agent_safety(s, ag, sp);
  }
}
template <class F, class = void> struct has_init_issue : std::false_type {};
template <class F> struct has_init_issue<F, std::void_t<decltype(&F::init_issue)>> : std::true_type {};
// fused rollout: the COMPUTING wave re-reads the kernel arguments every step (see the loop) unless the family opts out
// (`ROLLOUT_KEEPS_ARGS`: measured faster and inside the register budget)
// one-step kernel: re-read the arguments AFTER the rules for the output phase, so that what only the outputs need (a dozen
// pointers, the LDS plan) is not held in SGPRs across play() -- for the families whose step kernel spills SGPRs (`STEP_REREADS_ARGS`)
template <class F, class = void> struct step_rereads : std::false_type {};
template <class F> struct step_rereads<F, std::void_t<decltype(F::STEP_REREADS_ARGS)>> : std::integral_constant<bool, F::STEP_REREADS_ARGS> {};
template <class F, class = void> struct rollout_rereads : std::true_type {};
template <class F> struct rollout_rereads<F, std::void_t<decltype(F::ROLLOUT_KEEPS_ARGS)>> : std::integral_constant<bool, !F::ROLLOUT_KEEPS_ARGS> {};
// families whose cumulative reward vector (NU doubles per lane: 52 VGPRs in aintelope_savanna) is PARKED IN LDS while the rules
// run: nothing in the rules reads it, so its registers are free for them (`static constexpr bool CUM_IN_LDS = true`)
template <class F, class = void> struct cum_in_lds : std::false_type {};
template <class F> struct cum_in_lds<F, std::void_t<decltype(F::CUM_IN_LDS)>> : std::integral_constant<bool, F::CUM_IN_LDS> {};
// (rows of the stash: one per enabled output column, A * K)
template <class F> __host__ __device__ inline int cum_stash_rows(int A, int K) { return cum_in_lds<F>::value ? A * K : 0; }
template <class F, class = void> struct has_init_args : std::false_type {};
template <class F> struct has_init_args<F, std::void_t<decltype(&F::init_args)>> : std::true_type {};
// families that write their row of the rendered board into the wave's LDS image themselves
template <class F, class = void> struct has_board_stage : std::false_type {};
template <class F> struct has_board_stage<F, std::void_t<decltype(&F::stage_board)>> : std::true_type {};

// ---- a step's outputs: stage (the computing wave, from registers into its LDS buffer) and drain (LDS -> global) ----------
template <class F> constexpr int per_agent_cols(const KSpec& sp) { return F::PER_AGENT ? sp.A : 1; }

// Every requested output of one step is written into the wave's staging buffer in the byte order of the env-major global
// arrays (the wave's 64 rows are contiguous there).  `finished` / `real`: the returns staging of the accumulators.
template <class F, bool SMALL = true, bool BOARD = true>
__device__ inline void emit_stage(const typename F::State& s, const double (&r)[F::NU], double discount, const KArgs& a,
                                  const Lds& l, int lane) {
  const sgw_out& o = a.out;
  const KSpec& sp = a.sp;
  const int nd = a.need;
  const int HW = sp.HW, K = sp.A * sp.K, M = sp.M;   // reward rows hold all agents' vectors: [A][K]
  if (BOARD && (nd & (LN_BOARD | LN_OBS | LN_VIEWS | LN_OBSVIEWS))) {
    if constexpr (has_board_stage<F>::value) {            // boards with dynamic content: the family writes its row itself
      F::stage_board(l, s, sp, lane);
    } else {
      static_assert(!F::CUSTOM_BOARD, "a family with a custom board provides stage_board()");
      int cells[F::NSPRITE]; uint8_t chars[F::NSPRITE];
      const uint8_t* base = F::board_layers(s, sp, l, cells, chars);
      lds_write_board_row<F::NSPRITE>(l.board, HW, lane, base, cells, chars);
    }
  }
  SGW_STAMP(a, 9);
  if (nd & LN_REWARD) {
    const StageRow row_r(l.vec_r, l.trash, lane, K);
#pragma unroll
    for (int u = 0; u < F::NU; ++u) *row_r.cell(F::slot(sp, u)) = r[u];
  }
  if (nd & LN_CUMULATIVE) {
    const StageRow row_c(l.vec_c, l.trash, lane, K);
#pragma unroll
    for (int u = 0; u < F::NU; ++u) *row_c.cell(F::slot(sp, u)) = s.cum[u];
  }
  if ((nd & LN_METRICS) && o.metrics && M > 0) {
#pragma unroll
    for (int id = 0; id < F::NMETRIC; ++id) *stage_cell(l.vec_m, l.trash, lane, M, sp.metric_slot[id]) = F::metric(s, id);
  }
  SGW_STAMP(a, 10);
  if constexpr (SMALL) {
  if (nd & LN_ST) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) {
      if constexpr (F::PER_AGENT) l.st[lane * F::NA + ag] = (uint8_t)F::agent_step_type(s, ag);
      else l.st[lane * F::NA + ag] = (uint8_t)s.step_type;
    }
  }
  if (nd & LN_TR) {
    if constexpr (F::PER_AGENT) {
#pragma unroll
      for (int ag = 0; ag < F::NA; ++ag) l.tr[lane * F::NA + ag] = (uint8_t)F::agent_term(s, ag);
    } else {
      l.tr[lane] = (s.step_type == ST_LAST) ? (uint8_t)s.term : (uint8_t)SGW_TERM_NONE;
    }
  }
  if (nd & LN_ACT) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) l.act[lane * F::NA + ag] = (int8_t)F::actual(s, ag);
  }
  if (nd & LN_POS) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) {
      int pr, pc; F::agent_pos(s, ag, pr, pc);
      l.pos[(lane * F::NA + ag) * 2] = (uint8_t)pr; l.pos[(lane * F::NA + ag) * 2 + 1] = (uint8_t)pc;
    }
  }
  if (nd & LN_FLG) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) l.flg[lane * F::NA + ag] = (uint8_t)F::agent_flags(s, ag);
  }
  if (nd & LN_DISC) l.disc[lane] = discount;
  if (nd & LN_HID) l.hid[lane] = F::hidden(s);
  if (nd & LN_SAF) {
    if constexpr (F::PER_AGENT) {
      int saf_all[F::NA];
      agent_safeties<F>(s, sp, l, saf_all);
#pragma unroll
      for (int ag = 0; ag < F::NA; ++ag) l.saf[lane * F::NA + ag] = (int32_t)saf_all[ag];
    } else {
      l.saf[lane] = F::safety(s);
    }
  }
  if (nd & LN_FRM) l.frm[lane] = s.frame;
  }
}

// The wave streams its 64 contiguous rows of every requested output from LDS, 16 B per lane per instruction, no waits in
// between.  coop == false (masked reset): each ACTIVE lane copies only its own rows.
template <class F, bool SMALL = true, bool BOARD = true>
__device__ inline void emit_drain(const KArgs& a, const Lds& l, long long env0, int lane, long long toff, bool coop,
                                  bool lane_active) {
  const sgw_out& o = a.out;
  const KSpec& sp = a.sp;
  const int nd = a.need;
  const int HW = sp.HW, K = sp.A * sp.K, M = sp.M, A = F::NA, PA = F::PER_AGENT ? F::NA : 1;
  const long long env = env0 + lane;
  auto rows = [&](void* base, long long row_bytes, const void* src) {     // base = the output array at time slice toff
    uint8_t* dst = reinterpret_cast<uint8_t*>(base) + toff * row_bytes;
    if (coop) coop_store(dst, env0, (int)row_bytes, src, lane);
    else if (lane_active) lane_store(dst, env, (int)row_bytes, src, lane);
  };
  if (BOARD && (nd & LN_BOARD)) rows(o.board, HW, l.board);
  if (BOARD && (nd & LN_OBS)) {                          // value_mapping LUT (rendering.py:491-549)
    float* dst = o.obs_board + (toff + env0) * HW;
    const uint8_t* img = reinterpret_cast<const uint8_t*>(l.board);
    if (coop) {
      float4* d4 = reinterpret_cast<float4*>(dst);
      for (int c = lane; c < 16 * HW; c += WAVE) {       // 64*HW cells, 4 per lane-iteration
        uint32_t q = l.board[c];
        d4[c] = make_float4(l.value_map[q & 0x7f], l.value_map[(q >> 8) & 0x7f],
                            l.value_map[(q >> 16) & 0x7f], l.value_map[(q >> 24) & 0x7f]);
      }
    } else if (lane_active) {
      for (int i = 0; i < HW; ++i) dst[(long long)lane * HW + i] = l.value_map[img[lane * HW + i] & 0x7f];
    }
  }
  if (nd & LN_REWARD) rows(o.reward, K * 8, l.vec_r);
  if (nd & LN_CUMULATIVE) rows(o.cumulative, K * 8, l.vec_c);
  if ((nd & LN_METRICS) && o.metrics && M > 0) rows(o.metrics, M * 8, l.vec_m);
  if constexpr (SMALL) {
  if (nd & LN_ST) rows(o.step_type, A, l.st);
  if (nd & LN_TR) rows(o.term_reason, PA, l.tr);
  if (nd & LN_ACT) rows(o.actual_action, A, l.act);
  if (nd & LN_POS) rows(o.agent_pos, 2 * A, l.pos);
  if (nd & LN_FLG) rows(o.agent_flags, A, l.flg);
  if (nd & LN_DISC) rows(o.discount, 8, l.disc);
  if (nd & LN_HID) rows(o.hidden, 8, l.hid);
  if (nd & LN_SAF) rows(o.safety, 4 * PA, l.saf);
  if (nd & LN_FRM) rows(o.frame, 4, l.frm);
  }
}

// The per-env scalar outputs straight from registers (one narrow store per lane each): the wave that computed the step
// also drains it, so the LDS round trip of the pipelined rollout would only add instructions here.
template <class F>
__device__ inline void emit_small_direct(const typename F::State& s, double discount, const KArgs& a, const Lds& l, long long env0, int lane,
                                         long long toff, bool active) {
  if (!active) return;
  const sgw_out& o = a.out;
  const KSpec& sp = a.sp;
  const int nd = a.need;
  const long long row = toff + env0 + lane;
  if (nd & LN_ST) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) {
      if constexpr (F::PER_AGENT) store_wt(o.step_type + row * F::NA + ag, (uint8_t)F::agent_step_type(s, ag));
      else store_wt(o.step_type + row * F::NA + ag, (uint8_t)s.step_type);
    }
  }
  if (nd & LN_TR) {
    if constexpr (F::PER_AGENT) {
#pragma unroll
      for (int ag = 0; ag < F::NA; ++ag) store_wt(o.term_reason + row * F::NA + ag, (uint8_t)F::agent_term(s, ag));
    } else {
      store_wt(o.term_reason + row, (s.step_type == ST_LAST) ? (uint8_t)s.term : (uint8_t)SGW_TERM_NONE);
    }
  }
  if (nd & LN_ACT) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) store_wt(o.actual_action + row * F::NA + ag, (int8_t)F::actual(s, ag));
  }
  if (nd & LN_POS) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) {
      int pr, pc; F::agent_pos(s, ag, pr, pc);
      store_wt(o.agent_pos + (row * F::NA + ag) * 2, (uint8_t)pr); store_wt(o.agent_pos + (row * F::NA + ag) * 2 + 1, (uint8_t)pc);
    }
  }
  if (nd & LN_FLG) {
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) store_wt(o.agent_flags + row * F::NA + ag, (uint8_t)F::agent_flags(s, ag));
  }
  if (nd & LN_DISC) store_wt(o.discount + row, discount);
  if (nd & LN_HID) store_wt(o.hidden + row, F::hidden(s));
  if (nd & LN_SAF) {
    if constexpr (F::PER_AGENT) {
      int saf_all[F::NA];
      agent_safeties<F>(s, sp, l, saf_all);
#pragma unroll
      for (int ag = 0; ag < F::NA; ++ag) store_wt(o.safety + row * F::NA + ag, (int32_t)saf_all[ag]);
    } else {
      store_wt(o.safety + row, F::safety(s));
    }
  }
  if constexpr (has_safety2<F>::value) {
    if (nd & LN_SAF2) {
#pragma unroll
      for (int ag = 0; ag < F::NA; ++ag) store_wt(o.safety2 + row * F::NA + ag, (int32_t)F::agent_safety2(s, ag, sp));
    }
  }
  if (nd & LN_FRM) store_wt(o.frame + row, s.frame);
}

// sgw_out.done / obs_dir / act_dir: what the wrappers compute from step_type and agent_flags every step, written by the wave that
// holds the state (one byte per lane and agent: a handful of narrow stores per wave, no staging).  The three pointers are read
// from the kernarg segment HERE, through a pointer the compiler cannot see through, and only when asked for: as ordinary
// members of the argument block they were six more SGPRs live across the rules of every step kernel (boat_race_ex: 2 -> 6 SGPR
// spills, 7.07 -> 7.40 us per launch at the mixed suite's shard size) whether or not a launch wanted them.
template <class F>
__device__ inline void emit_decodes_direct(const typename F::State& s, const KArgs& a, long long env0, int lane, long long toff, bool active,
                                           int kargs_off) {
  const int nd = a.need;
  if (!(nd & (LN_DONE | LN_ODIR | LN_ADIR)) || !active) return;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const sgw_out __attribute__((address_space(4))) * OutSeg;
  OutSeg seg = (OutSeg)((const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + kargs_off + (int)offsetof(KArgs, out));
  asm volatile("" : "+s"(seg) : : "memory");
  struct { uint8_t *done, *obs_dir, *act_dir; } o = {seg->done, seg->obs_dir, seg->act_dir};
#else
  const sgw_out& o = a.out;
#endif
  const long long row = toff + env0 + lane;
#pragma unroll
  for (int ag = 0; ag < F::NA; ++ag) {
    int st;
    if constexpr (F::PER_AGENT) st = F::agent_step_type(s, ag); else st = s.step_type;
    if (nd & LN_DONE) store_wt(o.done + row * F::NA + ag, (uint8_t)(st >= ST_LAST ? 1 : 0));
    if (nd & (LN_ODIR | LN_ADIR)) {
      const int fl = F::agent_flags(s, ag);
      if (nd & LN_ODIR) store_wt(o.obs_dir + row * F::NA + ag, (uint8_t)((fl >> 3) & 3));
      if (nd & LN_ADIR) store_wt(o.act_dir + row * F::NA + ag, (uint8_t)((fl >> 1) & 3));
    }
  }
}

// workgroup barrier that orders LDS only: __syncthreads() also drains the wave's global stores (s_waitcnt vmcnt(0)),
// which is exactly what the draining wave of the pipelined rollout must not wait for
__device__ inline void lds_workgroup_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- agent-centric windows inside the step launch (sgw_out.views / obs_views; get_agent_perspective, safety_game_moma.py:1996-2101) ----
// The wave's 64 rendered board rows are in LDS already (emit_stage); the windows are assembled next to them in an LDS image laid
// out exactly like the wave's 64 rows of the [N, view_total] output and leave as plain 16-byte-per-lane stores: no second
// launch, no re-read of the board from HBM, no byte-granular global stores.
template <class F, class = void> struct has_views : std::false_type {};
template <class F> struct has_views<F, std::void_t<decltype(F::VIEWS)>> : std::integral_constant<bool, F::VIEWS> {};
template <class F, class = void> struct has_view_dir : std::false_type {};
template <class F> struct has_view_dir<F, std::void_t<decltype(&F::view_dir)>> : std::true_type {};

// rot90 by the agent's observation direction (Directions LEFT=0 RIGHT=1 UP=2 DOWN=3): first crop, then rotate
// (safety_game_moma.py:2085-2096).  (vr, vc) of the OUTPUT -> (row, col) of the crop; square windows only.
__device__ inline void view_unrotate(int dir, int n, int& vr, int& vc) {
  const int r = vr, c = vc;
  if (dir == 3) { vr = n - 1 - r; vc = n - 1 - c; }          // DOWN: rot90 k=2
  else if (dir == 0) { vr = n - 1 - c; vc = r; }             // LEFT: rot90 k=-1 (clockwise)
  else if (dir == 1) { vr = c; vc = n - 1 - r; }             // RIGHT: rot90 k=1 (counter-clockwise)
}
// the inverse: (cr, cc) of the crop -> (vr, vc) of the output
__device__ inline void view_rotate(int dir, int n, int& cr, int& cc) {
  const int r = cr, c = cc;
  if (dir == 3) { cr = n - 1 - r; cc = n - 1 - c; }
  else if (dir == 0) { cr = c; cc = n - 1 - r; }
  else if (dir == 1) { cr = n - 1 - c; cc = r; }
}

// ONE wave assembles the windows of envs [e_lo, e_hi) of its env-wave, an env at a time with all 64 lanes.  Everything that
// does not depend on the env is worked out once per agent, outside the env loop:
//   * a window no larger than the board is gathered (a lane per output byte): the lane's window coordinates are constants,
//     an env adds its agent's position (v_readlane of lane e's registers -> scalars);
//   * a window LARGER than the board (firemaker's supervisor: 33 x 33 around 17 x 17) is mostly padding: the block is filled
//     with the pad byte first and the BOARD's cells are dropped where they land.  The landing offset of board cell (r, c) is
//     (r - pr) * n + (c - pc) unrotated and, rot90-ed by the observation direction, one of +-(r * n + c), +-(c * n - r) plus a
//     term that only depends on the env -- so a lane keeps two constants per cell and an env costs one scalar and one add
//     per cell.  When the window covers the board wherever the agent stands (radius >= board size - 1: the reference's
//     `None` radius) no cell can fall outside and the bounds test is skipped.
// ROT: the env has observation directions (a scalar property of the spec; the caller branches once): without them every `dir`
// below is the constant UP and the rotation arithmetic folds away (firemaker's default mode: 86 instead of 89 us per round).
// `e_img0`: the env whose row is row 0 of the image at l.views (0: the image holds the env-wave's 64 rows; the chunked phase of
// the one-wavefront families hands over e_lo: its image holds rows [e_lo, e_hi) only).
template <class F, bool ROT>
__device__ inline void views_stage_wave_per_env(const typename F::State& s, const KSpec& sp, const Lds& l, int e_lo, int e_hi, int lane,
                                                int e_img0 = 0) {
  const int VB = sp.view_total, HW = sp.HW, W = sp.W, H = sp.H;
  const uint32_t pad = (uint32_t)sp.view_pad & 0xffu;
  uint8_t* img = l.views;
  const uint8_t* boards = reinterpret_cast<const uint8_t*>(l.board);
  if (sp.view_prefill) {                                     // (e_hi - e_lo) * VB is a multiple of 8 for blocks of 8 envs
    const uint64_t p8 = 0x0101010101010101ull * pad;
    uint64_t* blk = reinterpret_cast<uint64_t*>(img + (e_lo - e_img0) * VB);
    const int n8 = ((e_hi - e_lo) * VB) >> 3;
    for (int i = lane; i < n8; i += WAVE) blk[i] = p8;
  }
  lds_wave_sync();
#pragma unroll
  for (int ag = 0; ag < F::NA; ++ag) {
    const int vh = sp.view_h[ag], vw = sp.view_w[ag], len = vh * vw;
    if (len == 0) continue;                                  // scalar: an agent without a window (absent firemaker agents)
    int prow, pcol, pdir = 2;
    F::agent_pos(s, ag, prow, pcol);
    if constexpr (ROT) pdir = F::view_dir(s, ag);
    const int up = sp.view_up[ag], left = sp.view_left[ag], off = sp.view_off[ag];
    if (len > HW) {
      // board cells k = lane + 64 j, j < 5 (H * W <= 320): row / column and the two rotation constants, once
      constexpr int NP = (SGW_MAX_CELLS + WAVE - 1) / WAVE;
      int rr[NP], cc[NP], P[NP], Q[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int k = lane + WAVE * j;
        rr[j] = (k * sp.recip_W) >> 16; cc[j] = k - rr[j] * W;
        P[j] = rr[j] * vw + cc[j]; Q[j] = cc[j] * vw - rr[j];
      }
      const bool covers = up >= H - 1 && vh - 1 - up >= H - 1 && left >= W - 1 && vw - 1 - left >= W - 1;
      const int npass = (HW + WAVE - 1) / WAVE;
      for (int e = e_lo; e < e_hi; ++e) {
        const int pr = __builtin_amdgcn_readlane(prow, e) - up, pc = __builtin_amdgcn_readlane(pcol, e) - left;
        const int dir = ROT ? __builtin_amdgcn_readlane(pdir, e) : 2;
        // at = sgn * (rotated ? Q : P) + base   (scalars per env)
        const int n1 = vw - 1;
        const int base = dir == 2 ? -(pr * vw + pc) : (dir == 3 ? (n1 + pr) * vw + n1 + pc : (dir == 0 ? n1 + pr - pc * vw : (n1 + pc) * vw - pr));
        const bool useQ = dir < 2, neg = dir == 3 || dir == 1;
        const uint8_t* src = boards + e * HW;
        uint8_t* dst = img + (e - e_img0) * VB + off + base;
        uint8_t val[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) if (j < npass) val[j] = src[lane + WAVE * j < HW ? lane + WAVE * j : 0];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          if (j < npass) {
            const int t = useQ ? Q[j] : P[j];
            const int at = neg ? -t : t;
            bool ok = lane + WAVE * j < HW;
            if (!covers) { const int cr = rr[j] - pr, c2 = cc[j] - pc; ok = ok && cr >= 0 && cr < vh && c2 >= 0 && c2 < vw; }
            if (ok) dst[at] = val[j];
          }
        }
      }
    } else {
      // output bytes k = lane + 64 j of the window: the lane's window coordinates, once
      constexpr int NP = (SGW_MAX_CELLS + WAVE - 1) / WAVE;
      const int npass = (len + WAVE - 1) / WAVE;
      int wr[NP], wc[NP];
#pragma unroll
      for (int j = 0; j < NP; ++j) { const int k = lane + WAVE * j; wr[j] = (k * (int)sp.view_recip[ag]) >> 16; wc[j] = k - wr[j] * vw; }
      for (int e = e_lo; e < e_hi; ++e) {
        const int pr = __builtin_amdgcn_readlane(prow, e) - up, pc = __builtin_amdgcn_readlane(pcol, e) - left;
        const int dir = ROT ? __builtin_amdgcn_readlane(pdir, e) : 2;
        const uint8_t* src = boards + e * HW;
        uint8_t* dst = img + (e - e_img0) * VB + off;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          if (j < npass) {
            int vr = wr[j], vc = wc[j];
            view_unrotate(dir, vw, vr, vc);                   // dir is a scalar: uniform branches
            const int r = vr + pr, c = vc + pc;
            const bool inside = r >= 0 && r < H && c >= 0 && c < W;
            const uint32_t got = src[inside ? r * W + c : 0];
            if (lane + WAVE * j < len) dst[lane + WAVE * j] = (uint8_t)(inside ? got : pad);
          }
        }
      }
    }
  }
}

// Families whose env-waves are single wavefronts (island_navigation_ex_ma, aintelope_savanna): a LANE assembles its own env's
// windows -- 64 envs x 2 small windows would be 128 serial wave passes the other way.  The window cell index is uniform over
// the wave (scalar row / column); only the agent's position and, where the env has observation directions, the rot90 are per
// lane.  Specs without a window larger than the board only (with one, views_chunked walks the envs with the whole wave).
template <class F>
__device__ inline void views_stage_lane_per_env(const typename F::State& s, const KSpec& sp, const Lds& l, int lane) {
  const int VB = sp.view_total, HW = sp.HW, W = sp.W, H = sp.H;
  const uint32_t pad = (uint32_t)sp.view_pad & 0xffu;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(l.board) + lane * HW;
  uint8_t* row = l.views + lane * VB;
#pragma unroll
  for (int ag = 0; ag < F::NA; ++ag) {
    const int vh = sp.view_h[ag], vw = sp.view_w[ag], len = vh * vw;
    if (len == 0) continue;
    int prow, pcol, dir = 2;
    F::agent_pos(s, ag, prow, pcol);
    if constexpr (has_view_dir<F>::value) dir = sp.view_rotates ? F::view_dir(s, ag) : 2;
    const int pr = prow - (int)sp.view_up[ag], pc = pcol - (int)sp.view_left[ag], n1 = vw - 1;
    uint8_t* dst = row + sp.view_off[ag];
    // Board cell of output cell (vr, vc), rot90 by the lane's direction (view_unrotate): LINEAR in the scalar window coordinates,
    //   r = r0 + vr * drr + vc * drv,  c = c0 + vr * dcr + vc * dcv
    // with per-lane constants worked out once per agent -- a cell then costs three multiply-adds, the bounds test and the two LDS
    // accesses (a lone wave per SIMD issues a dependent VALU instruction every ~8 cycles: the select chains of the first version,
    // ~25 instructions per cell, made 50 window bytes cost 11 of island_navigation_ex_ma's 28.6 us)
    const int r0 = pr + ((dir == 3 || dir == 0) ? n1 : 0), c0 = pc + ((dir == 3 || dir == 1) ? n1 : 0);
    const int drv = dir == 0 ? -1 : (dir == 1 ? 1 : 0), dcv = dir == 2 ? 1 : (dir == 3 ? -1 : 0);
    const int drr = dir == 2 ? 1 : (dir == 3 ? -1 : 0), dcr = dir == 0 ? 1 : (dir == 1 ? -1 : 0);
    int vr = 0, vc = 0;                                       // scalar window coordinates of cell k
    constexpr int NB = 8;                                     // cells per batch: eight independent LDS reads in flight, then the eight writes
    for (int k = 0; k < len; k += NB) {
      uint32_t got[NB]; bool inside[NB];
#pragma unroll
      for (int h = 0; h < NB; ++h) {
        const int r = r0 + vr * drr + vc * drv, c = c0 + vr * dcr + vc * dcv;
        inside[h] = (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W;
        got[h] = src[inside[h] ? r * W + c : 0];
        if (++vc == vw) { vc = 0; ++vr; }                     // (past the window's end the coordinates run on harmlessly: reads are clamped)
      }
#pragma unroll
      for (int h = 0; h < NB; ++h) if (k + h < len) dst[k + h] = (uint8_t)(inside[h] ? got[h] : pad);
    }
  }
}

// LDS view image -> global: `nthr` threads (thread `tid` of them) copy the env-wave's 64 contiguous rows, 16 bytes per lane and
// instruction; the float variant maps four window bytes to four floats per store (value_mapping LUT, rendering.py:491-549)
__device__ inline void views_drain(const KArgs& a, const Lds& l, long long env0, long long toff, int tid, int nthr) {
  const int VB = a.sp.view_total;
  if (a.need & LN_VIEWS) {
    uint4* g = reinterpret_cast<uint4*>(a.out.views + (toff + env0) * VB);
    const uint4* src = reinterpret_cast<const uint4*>(l.views);
    const int n = 4 * VB;
    int j = tid;
    for (; j + 3 * nthr < n; j += 4 * nthr) {                // four LDS reads in flight, then the four stores
      const uint4 v0 = src[j], v1 = src[j + nthr], v2 = src[j + 2 * nthr], v3 = src[j + 3 * nthr];
      store16_wt(g + j, v0); store16_wt(g + j + nthr, v1); store16_wt(g + j + 2 * nthr, v2); store16_wt(g + j + 3 * nthr, v3);
    }
    for (; j < n; j += nthr) store16_wt(g + j, src[j]);
  }
  if (a.need & LN_OBSVIEWS) {
    uint4* g = reinterpret_cast<uint4*>(a.out.obs_views + (toff + env0) * VB);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(l.views);
    const int n = 16 * VB;
    for (int j = tid; j < n; j += nthr) {
      const uint32_t q = src[j];
      const float f0 = l.value_map[q & 0x7f], f1 = l.value_map[(q >> 8) & 0x7f], f2 = l.value_map[(q >> 16) & 0x7f], f3 = l.value_map[(q >> 24) & 0x7f];
      store16_wt(g + j, make_uint4(__float_as_uint(f0), __float_as_uint(f1), __float_as_uint(f2), __float_as_uint(f3)));
    }
  }
}
// masked reset: only the rows of the envs that were reset, a wave per env (slow path)
__device__ inline void views_drain_env(const KArgs& a, const Lds& l, long long env0, int e, int lane) {
  const int VB = a.sp.view_total;
  const uint8_t* src = l.views + e * VB;
  if (a.need & LN_VIEWS) { uint8_t* g = a.out.views + (env0 + e) * VB; for (int k = lane; k < VB; k += WAVE) g[k] = src[k]; }
  if (a.need & LN_OBSVIEWS) { float* g = a.out.obs_views + (env0 + e) * VB; for (int k = lane; k < VB; k += WAVE) g[k] = l.value_map[src[k] & 0x7f]; }
}

// ---- windows LARGER than the board in the one-wavefront families (island_navigation_ex_ma, aintelope_savanna) ----------------
// The env-wave's whole image is 64 x view_total bytes (aintelope_savanna's default two 21 x 21 windows: 56 448 B), which would
// cost the family resident workgroups.  The wave therefore assembles and drains G envs at a time through ONE region of
// G x view_total bytes (G = LdsPlan::views_g, chosen by the launcher with G * view_total a multiple of 16): pad-prefill, drop
// the board's cells (views_stage_wave_per_env), 16-byte write-through stores of the chunk's contiguous rows, next chunk.  The
// wave's LDS instructions execute in order, so a chunk's reads are done before the next chunk's prefill overwrites them.
// Masked reset: chunks without a reset env are skipped and the others leave row by row.
// The path is a family VARIANT of its own (`static constexpr bool VIEWS_CHUNKED = true`: SavannaBigViews, IslandMaBigViews,
// IslandMaWideBigViews), launched only when a spec with such a window asks for `views` / `obs_views`: as a runtime branch of the
// families' own kernels its scalar-heavy env loop raised their SGPR spills (island_navigation_ex_ma's step kernel: 143 -> 215,
// and with the spill lanes 230 -> 261 VGPR + 5 AGPR), whether or not a launch wanted windows.
template <class F, class = void> struct has_chunked_views : std::false_type {};
template <class F> struct has_chunked_views<F, std::void_t<decltype(F::VIEWS_CHUNKED)>> : std::integral_constant<bool, F::VIEWS_CHUNKED> {};
__device__ inline void views_drain_chunk(const KArgs& a, const Lds& l, long long row0, int nbytes, int lane) {
  const int VB = a.sp.view_total;
  if (a.need & LN_VIEWS) {
    uint4* g = reinterpret_cast<uint4*>(a.out.views + row0 * VB);
    const uint4* src = reinterpret_cast<const uint4*>(l.views);
    const int n = nbytes >> 4;
    int j = lane;
    for (; j + 3 * WAVE < n; j += 4 * WAVE) {                // four LDS reads in flight, then the four stores
      const uint4 v0 = src[j], v1 = src[j + WAVE], v2 = src[j + 2 * WAVE], v3 = src[j + 3 * WAVE];
      store16_wt(g + j, v0); store16_wt(g + j + WAVE, v1); store16_wt(g + j + 2 * WAVE, v2); store16_wt(g + j + 3 * WAVE, v3);
    }
    for (; j < n; j += WAVE) store16_wt(g + j, src[j]);
  }
  if (a.need & LN_OBSVIEWS) {
    uint4* g = reinterpret_cast<uint4*>(a.out.obs_views + row0 * VB);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(l.views);
    const int n = nbytes >> 2;
    for (int j = lane; j < n; j += WAVE) {
      const uint32_t q = src[j];
      const float f0 = l.value_map[q & 0x7f], f1 = l.value_map[(q >> 8) & 0x7f], f2 = l.value_map[(q >> 16) & 0x7f], f3 = l.value_map[(q >> 24) & 0x7f];
      store16_wt(g + j, make_uint4(__float_as_uint(f0), __float_as_uint(f1), __float_as_uint(f2), __float_as_uint(f3)));
    }
  }
}
template <class F>
__device__ inline void views_chunked(const typename F::State& s, const KArgs& a, const Lds& l, long long env0, long long toff, int lane,
                                     bool mask_on, bool lane_active) {
  const int G = a.lp.views_g, VB = a.sp.view_total;
  const unsigned long long on = mask_on ? __ballot(lane_active) : ~0ull;
  const unsigned long long chunk_bits = G >= WAVE ? ~0ull : ((1ull << G) - 1ull);
  const bool rot = has_view_dir<F>::value && a.sp.view_rotates;
  for (int e0 = 0; e0 < WAVE; e0 += G) {
    if (((on >> e0) & chunk_bits) == 0ull) continue;         // scalar
    if (rot) views_stage_wave_per_env<F, has_view_dir<F>::value>(s, a.sp, l, e0, e0 + G, lane, e0);
    else views_stage_wave_per_env<F, false>(s, a.sp, l, e0, e0 + G, lane, e0);
    lds_wave_sync();
    if (!mask_on) {
      views_drain_chunk(a, l, toff + env0 + e0, G * VB, lane);
    } else {
      for (int e = e0; e < e0 + G; ++e) {
        if (!((on >> e) & 1ull)) continue;
        const uint8_t* src = l.views + (e - e0) * VB;
        if (a.need & LN_VIEWS) { uint8_t* g = a.out.views + (env0 + e) * VB; for (int k = lane; k < VB; k += WAVE) g[k] = src[k]; }
        if (a.need & LN_OBSVIEWS) { float* g = a.out.obs_views + (env0 + e) * VB; for (int k = lane; k < VB; k += WAVE) g[k] = l.value_map[src[k] & 0x7f]; }
      }
    }
    lds_wave_sync();
  }
}

// families whose workgroup's waves write the board rows together (cooperative families: every wave holds the same envs)
template <class F, class = void> struct has_board_part : std::false_type {};
template <class F> struct has_board_part<F, std::void_t<decltype(&F::stage_board_part)>> : std::true_type {};
// the env-wave's 64 board rows (and their value-mapped float twins) LDS -> global by `nthr` threads
__device__ inline void board_drain_wg(const KArgs& a, const Lds& l, long long env0, long long toff, int tid, int nthr) {
  const int HW = a.sp.HW;
  if (a.need & LN_BOARD) {
    uint4* g = reinterpret_cast<uint4*>(a.out.board + (toff + env0) * HW);
    const uint4* src = reinterpret_cast<const uint4*>(l.board);
    const int n = 4 * HW;
    int j = tid;
    for (; j + nthr < n; j += 2 * nthr) {
      const uint4 v0 = src[j], v1 = src[j + nthr];
      store16_wt(g + j, v0); store16_wt(g + j + nthr, v1);
    }
    if (j < n) store16_wt(g + j, src[j]);
  }
  if (a.need & LN_OBS) {
    uint4* g = reinterpret_cast<uint4*>(a.out.obs_board + (toff + env0) * HW);
    const int n = 16 * HW;
    for (int j = tid; j < n; j += nthr) {
      const uint32_t q = l.board[j];
      const float f0 = l.value_map[q & 0x7f], f1 = l.value_map[(q >> 8) & 0x7f], f2 = l.value_map[(q >> 16) & 0x7f], f3 = l.value_map[(q >> 24) & 0x7f];
      store16_wt(g + j, make_uint4(__float_as_uint(f0), __float_as_uint(f1), __float_as_uint(f2), __float_as_uint(f3)));
    }
  }
}

// The windows of one step, after the board rows are staged: cooperative families split the env-wave's 64 envs over the
// workgroup's F::WAVES waves (every wave holds the same state; two workgroup barriers: the leader's board rows are visible,
// the image is complete), the others do it within the wave.  `mask_on`: masked reset -- only the rows of the envs whose lane
// has `lane_active` are written.
template <class F, bool BOARD_DRAIN = false>
__device__ inline void views_phase(const typename F::State& s, const KArgs& a_in, uint8_t* smem, int slot, long long env0, int lane, long long t,
                                   bool mask_on, bool lane_active, unsigned kargs_off) {
  // the phase reads its arguments (window geometry, output pointers, LDS plan) from the kernarg segment itself, through a
  // pointer the compiler cannot see through: nothing of it is held in SGPRs across the rules
#if defined(__HIP_DEVICE_COMPILE__)
  KArgs a_seg;
  {
    typedef const KArgs __attribute__((address_space(4))) * KArgsSeg;
    KArgsSeg seg = (KArgsSeg)((const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + kargs_off);
    asm volatile("" : "+s"(seg) : : "memory");
    a_seg = *seg;
  }
  const KArgs& a = a_seg;
#else
  const KArgs& a = a_in;
#endif
  const Lds l = lds_carve(smem, a.lp, F::LDS_EXTRA, slot);
  const long long toff = a.write_every != 0 ? t * a.n_pad : 0;
  constexpr int NW = F::WAVES, EPW = WAVE / NW;
  static_assert(NW == 1 || (EPW % 8) == 0, "a wave's block of the view image must be 8-byte aligned");
  const int w = NW > 1 ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
  if constexpr (NW > 1) lds_workgroup_barrier(); else lds_wave_sync();
  // BOARD_DRAIN: the board rows also leave by the whole workgroup (their stores are in flight while the windows are assembled)
  if constexpr (BOARD_DRAIN) board_drain_wg(a, l, env0, toff, (int)threadIdx.x, NW * WAVE);
  if (!(a.need & (LN_VIEWS | LN_OBSVIEWS))) return;
  if constexpr (has_chunked_views<F>::value) {
    // a spec with a window larger than the board: G envs at a time through the plan's chunk region (stages AND drains)
    static_assert(NW == 1, "");
    views_chunked<F>(s, a, l, env0, toff, lane, mask_on, lane_active);
    return;
  }
  if (NW == 1) views_stage_lane_per_env<F>(s, a.sp, l, lane);
  else if (has_view_dir<F>::value && a.sp.view_rotates) views_stage_wave_per_env<F, has_view_dir<F>::value>(s, a.sp, l, w * EPW, (w + 1) * EPW, lane);
  else views_stage_wave_per_env<F, false>(s, a.sp, l, w * EPW, (w + 1) * EPW, lane);
  if (!mask_on) {
    if constexpr (NW > 1) lds_workgroup_barrier(); else lds_wave_sync();
    views_drain(a, l, env0, toff, NW > 1 ? (int)threadIdx.x : lane, NW * WAVE);
  } else {
    lds_wave_sync();
    const unsigned long long on = __ballot(lane_active);
    for (int e = w * EPW; e < (w + 1) * EPW; ++e) if ((on >> e) & 1ull) views_drain_env(a, l, env0, e, lane);
  }
}

// The wave's accumulator row is updated with no-return f64 atomic adds executed at the memory side: nothing is loaded, so
// the wave never waits for the row (a load + store pair put a memory round trip on the critical path, and its pending
// load made the compiler drain vmcnt in the middle of the output staging).  Only this wave touches the row and it does so
// once per step, in program order: the sums are as deterministic as with plain stores.
__device__ inline void atomic_add_f64_noret(double* p, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  (void)__builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double*)p, v);
#else
  *p += v;
#endif
}

// Episodic-return accumulators (end-of-batch all-reduce buffer).  Lanes whose episode just ended have staged their return
// vector in l.vec_a (zeros otherwise).  lane = part * 16 + column: each lane sums one column over its part's 16 rows (reads
// batched, a fixed add tree) and adds the sum to the part's own accumulator row -- four rows per env-wave, no exchange between
// lanes; 16 columns per pass (one pass for C <= 16: every single-agent family and firemaker; island_navigation_ex_ma has
// 2K + 1 = 17..25).  Deterministic: every accumulator cell has one writer per launch and launches are ordered.  Traffic: one
// 8-byte RMW per column per 16 envs.
// Every one of the wave's 64 rows is staged -- a lane that is not a real env (the ragged end of the batch: it steps and ends
// episodes like any other) stages exact zeros -- so the reads need no per-row guard: one address per lane and pass, the 16 rows
// at fixed strides from it.  A lane past the last column reads the last column instead (inside vec_a) and adds nothing.
__device__ inline void accumulate_returns(const KArgs& a, const Lds& l, long long wave_id, int lane) {
  const int C = a.sp.A * a.sp.K + 1;
  const int part = lane >> 4;
  for (int c0 = 0; c0 < C; c0 += 16) {
    const int col = c0 + (lane & 15);
    const double* src = l.vec_a + part * 16 * C + (col < C ? col : C - 1);
    double v[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = src[j * C];
    // a fixed tree over the part's 16 rows (four add levels instead of a chain of sixteen); the four parts keep their own
    // accumulator rows -- no cross-lane exchange -- and k_read_returns adds the rows up in a fixed order
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1) {
#pragma unroll
      for (int j = 0; j < w; ++j) v[j] += v[j + w];
    }
    if (col < C) atomic_add_f64_noret(&a.ep_acc[(wave_id * SGW_ACC_PARTS + part) * C + col], v[0]);
  }
}

// KIND: K_STEP = exactly one step (sgw_step / sgw_step_n), K_ROLLOUT = a.T fused steps, K_RESET = sgw_reset.
// Separate instantiations keep the single-step kernel free of loop-carried scalar state.
enum { K_STEP = 0, K_ROLLOUT = 1, K_RESET = 2 };

// F::WAVES > 1 (cooperative families, firemaker): the workgroup's 64 envs are REPLICATED in every wave -- each wave
// runs the same lane-per-env code on the same state, so control flow (and every s_barrier) is identical across
// the waves -- and the family splits its wave-cooperative phase (one env at a time, one lane per board cell) over
// the waves.  Only wave 0 ("leader") writes outputs, accumulators and state.
//
// Non-cooperative families: the workgroup holds ENV_WAVES independent env-waves (64 envs each, one per SIMD) that share ONE
// LDS copy of the level tables and of the family's read-only tables.  A family may lower the count
// (`static constexpr int ENV_WAVES_MAX`) when four waves' worth of output staging would not fit the CU's 160 KiB of LDS
// with every output requested (island_navigation_ex_ma: 2, aintelope_savanna: 1).
//
// PIPELINED fused rollout (K_ROLLOUT, non-cooperative): every env-wave is a PAIR of wavefronts.  The computing wave keeps
// the state in registers, plays step t and stages its outputs into LDS buffer t & 1; the draining wave copies buffer t & 1
// to global memory and folds the finished episodes into the accumulators while the computing wave is already playing
// step t + 1.  One LDS-only workgroup barrier per step hands a buffer over.  A lone wave issues one instruction per ~4
// cycles whatever it does, and rules and output copy are about as many instructions each: two waves overlap them.
template <class F, class = void> struct family_env_waves { static constexpr int value = ENV_WAVES; };
template <class F> struct family_env_waves<F, std::void_t<decltype(F::ENV_WAVES_MAX)>> { static constexpr int value = F::ENV_WAVES_MAX; };
template <class F, class = void> struct family_pipelines : std::true_type {};
template <class F> struct family_pipelines<F, std::void_t<decltype(F::ROLLOUT_PIPELINED)>> : std::integral_constant<bool, F::ROLLOUT_PIPELINED> {};
// (K_STEP as a pair of wavefronts was measured too: 7.9 us instead of 6.8 at 65 536 envs, 0.53 instead of 0.66 of the roofline at
// 1 M -- the second wave's start-up and the hand-over barrier cost more than the store issue it takes off the first)
template <class F, int KIND> constexpr bool pipelined() { return KIND == K_ROLLOUT && !F::COOPERATIVE && family_pipelines<F>::value; }
// a pipelined workgroup holds at most two env-waves = four wavefronts, one per SIMD, each with the full register file
template <class F, int KIND> constexpr int env_waves() {
  return F::COOPERATIVE ? 1 : (pipelined<F, KIND>() ? (family_env_waves<F>::value < 2 ? family_env_waves<F>::value : 2) : family_env_waves<F>::value);
}
template <class F, int KIND> constexpr int lds_buffers() { return pipelined<F, KIND>() ? 2 : 1; }
template <class F, int KIND> constexpr int wg_threads() { return F::WAVES * env_waves<F, KIND>() * WAVE * (pipelined<F, KIND>() ? 2 : 1); }

// Warm the scalar cache with the launch's whole argument block while the prologue's global loads are in flight.  The bodies
// read their arguments in several batches, each at its first use and each followed by a wait (SGPR pressure keeps the compiler
// from hoisting them), and a launch's kernarg segment is cold: every batch that starts a new 64-byte line is a serial miss on a
// lone wave's critical path, most of them after the staging barrier.  One load per line, all issued at once behind the global
// loads, then one wait that the state's round trip covers; the later reads hit.  The values are discarded (one scratch SGPR).
// Bytes [0, END) of the segment: a load every 64 bytes and the last dword, so every line is touched whatever the segment's
// alignment, and nothing past the last argument byte is read.
//
// Two statements: `issue` holds the loads, `settle` the wait, and the engine puts `settle` just ahead of the staging barrier.  The
// scalar misses then overlap the vector loads' round trip instead of standing between the loads issued before the touch and
// whatever follows it.  Sound because (a) the scratch SGPR is an operand of both statements, so it stays allocated to this
// value from the first to the second and no late-returning load can land in a register that holds something else; (b) the
// loads the compiler does not know of only ADD to lgkmcnt: a counted wait of its own (LDS returns in order) can only wait
// longer than it needs, never too briefly, and its waits for scalar loads are always lgkmcnt(0).  tests/test_prologue_order.py
// reads both from the assembly of every k_engine kernel, whatever its family.
template <int END>
__device__ __forceinline__ uint32_t kernarg_touch_issue() {
  uint32_t t = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int LAST = END - 4, N = (LAST + 63) / 64;          // strided loads at 0, 64, ..., (N - 1) * 64 < LAST, then LAST
  static_assert(END % 4 == 0 && LAST >= 0 && (N - 1) * 64 + 4 <= END && LAST + 4 <= END && LAST - (N - 1) * 64 <= 64,
                "the touch loads cover every line of the argument block and stay inside it");
  asm volatile(".set sgw_touch_off, 0\n\t.rept %c2\n\ts_load_dword %0, %1, sgw_touch_off\n\t.set sgw_touch_off, sgw_touch_off + 64\n\t.endr\n\t"
               "s_load_dword %0, %1, %c3"
               : "=&s"(t) : "s"(__builtin_amdgcn_kernarg_segment_ptr()), "i"(N), "i"(LAST) : "memory");
#endif
  return t;
}
__device__ __forceinline__ void kernarg_touch_settle([[maybe_unused]] uint32_t t) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(0) ; kernarg touch settled, %0 free" : "+s"(t) : : "memory");
#endif
}
// `a` = a fresh copy of the KArgs block that sits `kargs_off` bytes into the kernarg segment (why: see the rollout loop of engine_body).
// Filled in place: returned by value, the copy cost aintelope_savanna's step kernel three instructions.
__device__ __forceinline__ void kargs_reread(KArgs& a, const unsigned kargs_off) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const KArgs __attribute__((address_space(4))) * KArgsSeg;
  KArgsSeg seg = (KArgsSeg)((const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr() + kargs_off);
  asm volatile("" : "+s"(seg) : : "memory");
  a = *seg;
#endif
}

#ifdef SGW_WAVES_PER_EU     // experiment: force an occupancy target (registers beyond it go to scratch)
#define SGW_OCC __attribute__((amdgpu_waves_per_eu(SGW_WAVES_PER_EU, SGW_WAVES_PER_EU)))
#else
#define SGW_OCC
#endif
// The engine's body: workgroup `block` of a launch whose KArgs block sits `kargs_off` bytes into the kernarg segment (the
// re-reading paths below go back to it there).  k_engine is this and nothing else; k_engine_group runs it for the member of a
// heterogeneous launch that the workgroup belongs to.
// TOUCH_END > 0: the launch's argument block is bytes [0, TOUCH_END) of the kernarg segment and nobody has read it yet
// (k_engine; k_engine_group has touched its member's block before it gets here).
template <class F, int KIND, int TOUCH_END = 0>
__device__ __forceinline__ void engine_body(const KArgs& a, const long long block, const unsigned kargs_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int EW = env_waves<F, KIND>();
  constexpr bool PIPE = pipelined<F, KIND>();
  constexpr int NB = lds_buffers<F, KIND>();
  constexpr int NT = wg_threads<F, KIND>();
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_in_wg = (F::COOPERATIVE || (EW == 1 && !PIPE)) ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wv = PIPE ? (wave_in_wg >= EW ? wave_in_wg - EW : wave_in_wg) : wave_in_wg;       // env-wave within the workgroup
  const bool drainer = PIPE && wave_in_wg >= EW;
  const bool leader = F::WAVES == 1 || threadIdx.x < WAVE;
  const long long wave_id = block * EW + wv;
  const long long env0 = wave_id * WAVE;
  const long long env = env0 + lane;
  const long long env_id = a.env_id_base + env;
  const bool real = env < a.n_envs;
  const bool wave_live = env0 < a.n_pad;                 // the last workgroup may hold fewer than EW env-waves

  SGW_STAMP_RT(a, 6);
  SGW_STAMP(a, 0);
  // every global load of the prologue is ISSUED before anything waits (level tables, the family's tables, the env's state,
  // the first actions: one memory round trip, not four); LDS is written afterwards.  The source order alone does not give
  // that: see sgw_pow_stage_issue and kernarg_touch_issue, and tests/test_prologue_order.py, which reads it off the assembly.
  TableStage ts;
  lds_tables_issue<NT>(ts, a.tables);
  const Lds l = lds_carve(smem, a.lp, F::LDS_EXTRA, wv * NB);
  typename F::Ctx cx;
  // no control flow up to the barrier: a dead env-wave (past n_pad in the last workgroup) loads env-wave 0's state and the
  // first table bytes instead of branching around its loads, so the compiler keeps every load of the prologue in one block
  typename F::State s;
  F::load(s, a, wave_live ? env : (long long)lane);
  int action0[F::NA];
#pragma unroll
  for (int ag = 0; ag < F::NA; ++ag) {
    const bool have = KIND != K_RESET && a.actions != nullptr && real;
    const int8_t* ap = have ? a.actions + env * F::NA + ag : reinterpret_cast<const int8_t*>(a.tables);
    const int v = (int)*ap;
    action0[ag] = have ? v : 0;
  }
  // the family's tables LAST: every wave of the launch reads the same 5 KB of pow tables, and loads return in order -- issued
  // ahead of the state they held the state back (measured: 5.54 us per headline launch instead of 5.18)
  if constexpr (has_init_issue<F>::value) F::init_issue(cx);
  [[maybe_unused]] uint32_t touch = 0;
  if constexpr (TOUCH_END > 0) touch = kernarg_touch_issue<TOUCH_END>();
  lds_tables_commit<NT>(ts, smem);
  F::init_ctx(cx, l);
  if constexpr (has_init_args<F>::value) F::init_args(cx, l, a);
  // pipelined rollout with synthetic actions: the Philox stream (~100 instructions per agent and step) is the draining wave's
  // work -- it writes step t + 2's actions into buffer t & 1's inbox while the computing wave plays step t + 1
  if constexpr (PIPE && KIND == K_ROLLOUT) {
    if (drainer && a.actions == nullptr) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const Lds lb = lds_carve(smem, a.lp, F::LDS_EXTRA, wv * NB + b);
#pragma unroll
        for (int ag = 0; ag < F::NA; ++ag)
          lb.ain[ag * WAVE + lane] = (int8_t)synth_action(a.seed, env_id, a.step0 + b, ag, a.sp.action_lo, a.sp.n_actions);
      }
    }
  }
  if constexpr (TOUCH_END > 0) kernarg_touch_settle(touch);
  __syncthreads();
  const int TT = (KIND == K_STEP) ? 1 : a.T;
  if constexpr (PIPE) {
    if (!wave_live || drainer) {
      // the draining wave (and a dead pair, which only keeps the barrier count): one barrier per step hands over buffer t & 1
      for (int t = 0; t < TT; ++t) {
        lds_workgroup_barrier();
        if (!wave_live) continue;
        KArgs a_step;
        kargs_reread(a_step, kargs_off);
        const Lds lb = lds_carve(smem, a_step.lp, F::LDS_EXTRA, wv * NB + (NB > 1 ? (t & 1) : 0));
        if (a_step.write_every != 0 || t == TT - 1)
          emit_drain<F>(a_step, lb, env0, lane, a_step.write_every != 0 ? (long long)t * a_step.n_pad : 0, true, true);
        if ((a_step.need & LN_RETURNS) && lb.flag[0] != 0u) accumulate_returns(a_step, lb, wave_id, lane);
        if (a_step.actions == nullptr && t + 2 < TT) {      // the computing wave read this inbox before the barrier above
#pragma unroll
          for (int ag = 0; ag < F::NA; ++ag)
            lb.ain[ag * WAVE + lane] = (int8_t)synth_action(a_step.seed, a_step.env_id_base + env, a_step.step0 + t + 2, ag,
                                                            a_step.sp.action_lo, a_step.sp.n_actions);
        }
      }
      return;
    }
  } else {
    if (!wave_live) return;
  }
  SGW_STAMP(a, 1);

  if (KIND == K_RESET) {
    const bool m = a.mask ? (real && a.mask[env] != 0) : true;
    double r[F::NU];
#pragma unroll
    for (int u = 0; u < F::NU; ++u) r[u] = 0.0;
    if (m) { F::begin_episode(s, a, l, env, env_id); if (leader) F::store(s, a, env); }
    if (leader) {
      lds_wave_sync();
      emit_stage<F, false>(s, r, __longlong_as_double(0x7ff8000000000000LL), a, l, lane);
    }
    if constexpr (has_views<F>::value) {
      if (a.need & (LN_VIEWS | LN_OBSVIEWS)) views_phase<F>(s, a, smem, wv * NB, env0, lane, 0, a.mask != nullptr, m, kargs_off);
    }
    if (leader) {
      lds_wave_sync();
      emit_drain<F, false>(a, l, env0, lane, 0, a.mask == nullptr, m);
      emit_small_direct<F>(s, __longlong_as_double(0x7ff8000000000000LL), a, l, env0, lane, 0, a.mask == nullptr || m);
      emit_decodes_direct<F>(s, a, env0, lane, 0, a.mask == nullptr || m, kargs_off);
    }
    return;
  }

  const KArgs& a_launch = a;
  const Lds& l_launch = l;
  for (int t = 0; t < TT; ++t) {
    // Fused rollout: nothing of the ARGUMENTS may stay live across the back-edge.  The loop would otherwise keep the whole
    // kernarg block (110 dwords) and everything derived from it in SGPRs -- every K_ROLLOUT instantiation sat at the 106-SGPR
    // ceiling with 200-630 SGPR spills -- so each step re-reads what it needs from the kernarg segment through a pointer the
    // compiler cannot see through (scalar loads, scalar cache hits).  The memory clobber does the same for loop-invariant
    // LDS reads (the family constants: 76 VGPRs in island_navigation_ex_ma).
    KArgs a_step;
    if constexpr (KIND == K_ROLLOUT && rollout_rereads<F>::value) kargs_reread(a_step, kargs_off);
    else if constexpr (KIND == K_ROLLOUT) asm volatile("" ::: "memory");
    const KArgs& a = (KIND == K_ROLLOUT && rollout_rereads<F>::value) ? a_step : a_launch;
    // ... and the LDS carve (a dozen region addresses) is re-derived from this step's arguments for the same reason
    const Lds l_step = lds_carve(smem, a.lp, F::LDS_EXTRA, wv * NB + (NB > 1 ? (t & 1) : 0));
    const Lds& l = KIND == K_ROLLOUT ? l_step : l_launch;   // (K_ROLLOUT: also selects the buffer t & 1)
    double r[F::NU];
#pragma unroll
    for (int u = 0; u < F::NU; ++u) r[u] = 0.0;
    double discount = __longlong_as_double(0x7ff8000000000000LL);   // None at FIRST
    bool over_now = false;
    if constexpr (cum_in_lds<F>::value) {                           // park the cumulative vector (re-read below, on every path)
#pragma unroll
      for (int u = 0; u < F::NU; ++u) { const int q = F::slot(a.sp, u); if (q >= 0) l.cstash[q * WAVE + lane] = s.cum[u]; }   // (a dimension that is not enabled stays 0)
    }
    [[maybe_unused]] const bool resetting = s.step_type >= ST_LAST;       // (the cooperative branch: lanes that auto-reset this step)
    // the actions this step plays: sgw_step / sgw_step_n always the caller's first row (loaded in the prologue), a rollout the
    // caller's buffer or, without one, the synthetic stream
    int action[F::NA];
#pragma unroll
    for (int ag = 0; ag < F::NA; ++ag) {
      if constexpr (KIND == K_STEP) action[ag] = action0[ag];
      else if (a.actions) action[ag] = (t == 0) ? action0[ag]
                                                : (real ? (int)a.actions[((long long)t * a.n_envs + env) * F::NA + ag] : 0);
      else if constexpr (PIPE) action[ag] = (int)l.ain[ag * WAVE + lane];     // the draining wave's Philox (see the prologue; never a cooperative family)
      else action[ag] = synth_action(a.seed, env_id, a.step0 + t, ag, a.sp.action_lo, a.sp.n_actions);
    }
    if constexpr (!F::COOPERATIVE) {
      bool idle = false;
      if constexpr (has_idle_round<F>::value) idle = s.step_type >= ST_LAST && !F::reset_requested(s, a, action);
      if (idle) {
        // multi-agent adapter, finished episode, no eligible agent in the submitted dict (PM:173-246: the play loop does not
        // run, so nothing resets): only the per-agent states move on (LAST -> DEAD); rewards are the default zeros
        if constexpr (has_idle_round<F>::value) discount = F::idle_round(s);
        if constexpr (cum_in_lds<F>::value) {
#pragma unroll
          for (int u = 0; u < F::NU; ++u) { const int q = F::slot(a.sp, u); s.cum[u] = q >= 0 ? l.cstash[q * WAVE + lane] : 0.0; }
        }
      } else if (s.step_type >= ST_LAST) {
        // step after LAST (or before any reset): new episode, action discarded (pycolab_interface_mo.py:175-178); the
        // multi-agent adapters still shuffle the discarded actions when more than one was submitted
        F::pre_autoreset(s, a, action);
        F::begin_episode(s, a, l, env, env_id);
      } else {
        discount = F::play(s, action, a, l, r, env);
        const bool over = (discount == 0.0) || (s.frame >= a.sp.max_iterations);   // pycolab_interface.py:292-303
        s.step_type = over ? ST_LAST : ST_MID;
        if (over && s.term == TERM_NONE4) s.term = SGW_MAX_STEPS;                   // safety_game.py:294-296
#pragma unroll
        for (int u = 0; u < F::NU; ++u) {                                          // safety_game_mo.py:996-997
          if constexpr (cum_in_lds<F>::value) { const int q = F::slot(a.sp, u); s.cum[u] = (q >= 0 ? l.cstash[q * WAVE + lane] : 0.0) + r[u]; }
          else s.cum[u] += r[u];
        }
        over_now = over;
      }
    } else {
      // cooperative families run play() with every lane active (their wave-wide phases need full EXEC and every wave
      // must reach the same barriers); lanes that auto-reset this step pass live = false and change nothing
      if (resetting) { F::pre_autoreset(s, a, action); F::begin_episode(s, a, l, env, env_id); }
      const double d = F::play(s, action, a, l, r, env, !resetting, cx);
      if (!resetting) {
        discount = d;
        const bool over = (discount == 0.0) || (s.frame >= a.sp.max_iterations);
        s.step_type = over ? ST_LAST : ST_MID;
        if (over && s.term == TERM_NONE4) s.term = SGW_MAX_STEPS;
#pragma unroll
        for (int u = 0; u < F::NU; ++u) s.cum[u] += r[u];
        over_now = over;
      }
    }
    SGW_STAMP(a, 2);
    // ---- this step's outputs and finished-episode returns go into the wave's staging buffer ...
    KArgs a_out;
    if constexpr (KIND == K_STEP && step_rereads<F>::value) kargs_reread(a_out, kargs_off);
    const KArgs& ae = (KIND == K_STEP && step_rereads<F>::value) ? a_out : a;
    const Lds l_out = lds_carve(smem, ae.lp, F::LDS_EXTRA, wv * NB + (NB > 1 ? (t & 1) : 0));
    const Lds& le = (KIND == K_STEP && step_rereads<F>::value) ? l_out : l;
    const int C = ae.sp.A * ae.sp.K + 1;
    const bool last_t = (t == TT - 1);
    const bool writes = ae.write_every != 0 || last_t;
    bool acc_any = false;
    if (leader) {
      if constexpr (!PIPE) lds_wave_sync();                 // the previous step's cooperative reads are done (program order)
      if (ae.need & LN_RETURNS) {
        acc_any = __ballot(over_now && real) != 0ull;       // wave-uniform
        if (acc_any) {
          const StageRow row_a(le.vec_a, le.trash, lane, C);
#pragma unroll
          for (int u = 0; u < F::NU; ++u) *row_a.cell(F::slot(ae.sp, u)) = (over_now && real) ? s.cum[u] : 0.0;
          le.vec_a[lane * C + C - 1] = (over_now && real) ? 1.0 : 0.0;       // a padded lane's row: zeros (accumulate_returns)
        }
        if constexpr (PIPE) { if (lane == 0) le.flag[0] = acc_any ? 1u : 0u; }
      }
      SGW_STAMP(ae, 8);
      if (writes) {
        emit_stage<F, PIPE, !has_board_part<F>::value>(s, r, discount, ae, le, lane);
        emit_decodes_direct<F>(s, ae, env0, lane, ae.write_every != 0 ? (long long)t * ae.n_pad : 0, true, kargs_off);
      }
    }
    if constexpr (has_board_part<F>::value) {
      // cooperative family: the WORKGROUP produces the step's big outputs -- every wave writes a slice of the board rows, then
      // (one barrier) a share of the board's and (a second barrier) of the windows' stores; the leader keeps the rest
      static_assert(!PIPE && has_views<F>::value && F::COOPERATIVE, "");
      if (writes && (ae.need & (LN_BOARD | LN_OBS | LN_VIEWS | LN_OBSVIEWS))) {
        F::stage_board_part(le, s, ae.sp, lane, __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
        views_phase<F, true>(s, ae, smem, wv * NB, env0, lane, t, false, true, kargs_off);
      }
    } else if constexpr (has_views<F>::value) {
      static_assert(!PIPE, "the pipelined rollout has no window phase (the families with agent views do not pipeline)");
      if (writes && (ae.need & (LN_VIEWS | LN_OBSVIEWS)))
        views_phase<F>(s, ae, smem, wv * NB, env0, lane, t, false, true, kargs_off);
    }
    // ... and leave it: the pair's draining wave takes the buffer over at the barrier (pipelined rollout), or this wave
    // copies it out itself
    if constexpr (PIPE) {
      lds_workgroup_barrier();
    } else if (leader) {
      lds_wave_sync();
      if (writes) {
        emit_drain<F, false, !has_board_part<F>::value>(ae, le, env0, lane, ae.write_every != 0 ? (long long)t * ae.n_pad : 0, true, true);
        SGW_STAMP(ae, 11);
        emit_small_direct<F>(s, discount, ae, le, env0, lane, ae.write_every != 0 ? (long long)t * ae.n_pad : 0, true);
      }
      SGW_STAMP(ae, 3);
      if (acc_any) accumulate_returns(ae, le, wave_id, lane);
    }
    if constexpr (KIND == K_STEP && step_rereads<F>::value) { if (leader) F::store(s, ae, env); return; }
  }
  SGW_STAMP(a, 4);
  if (leader) F::store(s, a, env);
  SGW_STAMP(a, 5);
  SGW_STAMP_RT(a, 7);
}

// ---- compile-time output geometry ("shape") of a one-step kernel ----------------------------------------------------------
// A shaped k_engine overwrites the geometry fields of its argument copy with constants: board H x W, reward row width A * K (one
// agent) and the universe-dimension -> column map.  Everything downstream reads them from that copy, so the compiler folds them:
// the board row becomes HW / 16 LDS quad writes plus the agent byte, every reward cell a fixed LDS offset with no trash row, each
// drain a fixed number of unguarded 16-byte stores per lane and the returns transpose a single pass of fixed width.  Which
// outputs a launch asks for (`need`) stays a runtime mask.  The launcher picks a shaped kernel only when the engine's spec holds
// exactly these values (sgw_api.hip, ShapedSteps); everything else runs the generic kernel (NoShape).
struct NoShape { static constexpr bool ON = false; };
template <int H_, int W_, int K_, int... SLOT>
struct StepShape {
  static constexpr bool ON = true;
  static constexpr int H = H_, W = W_, HW = H_ * W_, K = K_, NSLOT = (int)sizeof...(SLOT);
  static_assert(HW <= SGW_MAX_CELLS && K >= 1 && K <= SGW_MAX_K && NSLOT <= SGW_MAX_K, "");
  __host__ __device__ static constexpr int slot(int u) { constexpr int8_t s[NSLOT] = {(int8_t)SLOT...}; return s[u]; }
  __host__ static bool matches(const KSpec& k) {
    if (k.H != H || k.W != W || k.HW != HW || k.A != 1 || k.K != K) return false;
    for (int u = 0; u < SGW_MAX_K; ++u) if (k.dim_slot[0][u] != (u < NSLOT ? slot(u) : -1)) return false;
    return true;
  }
  __device__ static void apply(KSpec& k) {
    k.H = H; k.W = W; k.HW = HW; k.A = 1; k.K = K;
#pragma unroll
    for (int u = 0; u < NSLOT; ++u) k.dim_slot[0][u] = (int8_t)slot(u);
  }
};

template <class F, int KIND, class SH = NoShape>
__global__ SGW_OCC __launch_bounds__((wg_threads<F, KIND>())) void k_engine(uint64_t* hot_state, const uint8_t* hot_tables, const int8_t* hot_actions,
                                                                      long long hot_n_pad, long long hot_n_envs, int hot_words,
                                                                      const KArgs a_in) {
  // the leading scalar arguments repeat the few values the prologue's loads need (state / tables / actions pointers, sizes):
  // as LEADING kernel arguments they are preloaded into SGPRs at wave launch (-mllvm -amdgpu-kernarg-preload-count), so
  // the first global loads issue without waiting for a scalar load of the kernarg segment from memory
  KArgs a = a_in;
  a.state = hot_state; a.tables = hot_tables; a.actions = hot_actions; a.n_pad = hot_n_pad; a.n_envs = hot_n_envs; a.sp.words = hot_words;
  if constexpr (SH::ON) {
    // (a re-reading family would fetch the runtime geometry back from the kernarg segment)
    static_assert(KIND == K_STEP && !step_rereads<F>::value && !F::PER_AGENT && F::NA == 1 && SH::NSLOT == F::NU, "");
    SH::apply(a.sp);
  }
  engine_body<F, KIND, SGW_KARGS_OFFSET + (int)sizeof(KArgs)>(a, (long long)blockIdx.x, SGW_KARGS_OFFSET);
}

// ---- the forked one-step kernel: a state wave and an output wave per env-wave, no hand-over ---------------------------------
// A one-step launch of at most one env-wave per SIMD (the headline: 65 536 envs = 1 024 waves on 1 024 SIMDs) is one serial
// chain per wave, and a lone wave leaves more than half of its SIMD's issue slots idle.  Here every env-wave is TWO wavefronts
// that load the same old state and the same action and run the same deterministic rules, so both hold the same bits:
//   the S wave (waves [0, EW) of the workgroup) keeps the state side: returns accumulation and the state store;
//   the O wave (waves [EW, 2 EW)) keeps the output side: board / reward / ... staging, the drains and the small direct stores.
// Nothing passes from one to the other (the hand-over form, a second wave that waits for the first one's play behind a barrier,
// is the pair that was measured and lost, see pipelined() above).  The O wave leaves the rules' regrowth pass out unless
// `metrics` is asked for: no other output reads what the pass writes.  The LDS plan is k_engine's for EW env-waves: the O wave
// owns board / vec_r / vec_c / vec_m and the small-output regions of its env-wave, the S wave vec_a.
// F provides play_events (the play without the regrowth pass) and the pow stage for a workgroup of any size (CtxN / init_issue_n / init_ctx_n).
#ifndef SGW_FORK_EW
#define SGW_FORK_EW 2        // env-waves per workgroup: 2 (256 threads, one wave per SIMD) or 4 (512 threads); measured at the headline:
                             // 4.87-4.91 us per launch with 2, 5.29-5.34 with 4, the one-wave kernel 5.17-5.19
#endif
constexpr int FORK_EW = SGW_FORK_EW, FORK_THREADS = 2 * FORK_EW * WAVE;
static_assert(FORK_EW == 2 || FORK_EW == 4, "");
enum { ROLE_STATE = 0, ROLE_OUTPUT = 1 };

// one role's part of the step, after the staging barrier: straight-line but for the auto-reset / play branch
template <class F, int ROLE>
__device__ __forceinline__ void fork_role(typename F::State& s, const int (&action)[F::NA], const KArgs& a, const Lds& l, const long long wave_id,
                                          const long long env0, const int lane, const bool real, const unsigned kargs_off) {
  const long long env = env0 + lane;
  double r[F::NU];
#pragma unroll
  for (int u = 0; u < F::NU; ++u) r[u] = 0.0;
  double discount = __longlong_as_double(0x7ff8000000000000LL);   // None at FIRST
  bool over_now = false;
  if (s.step_type >= ST_LAST) {
    F::pre_autoreset(s, a, action);
    F::begin_episode(s, a, l, env, a.env_id_base + env);
  } else {
    if constexpr (ROLE == ROLE_STATE) {
      discount = F::play(s, action, a, l, r, env);
    } else {
      // wave-uniform: `metrics` shows d_avail / f_avail, so a launch that asks for it plays the whole rules here too
      if (a.need & LN_METRICS) discount = F::play(s, action, a, l, r, env);
      else discount = F::play_events(s, action, a, l, r, env);
    }
    const bool over = (discount == 0.0) || (s.frame >= a.sp.max_iterations);
    s.step_type = over ? ST_LAST : ST_MID;
    if (over && s.term == TERM_NONE4) s.term = SGW_MAX_STEPS;
#pragma unroll
    for (int u = 0; u < F::NU; ++u) s.cum[u] += r[u];
    over_now = over;
  }
  SGW_STAMP(a, 2);
  if constexpr (ROLE == ROLE_STATE) {
    F::store(s, a, env);
    SGW_STAMP(a, 4);
    if (a.need & LN_RETURNS) {
      if (__ballot(over_now && real) != 0ull) {                    // wave-uniform
        const int C = a.sp.A * a.sp.K + 1;
        const StageRow row_a(l.vec_a, l.trash, lane, C);
#pragma unroll
        for (int u = 0; u < F::NU; ++u) *row_a.cell(F::slot(a.sp, u)) = (over_now && real) ? s.cum[u] : 0.0;
        l.vec_a[lane * C + C - 1] = (over_now && real) ? 1.0 : 0.0;
        lds_wave_sync();
        accumulate_returns(a, l, wave_id, lane);
      }
    }
    SGW_STAMP(a, 5);
  } else {
    emit_stage<F, false, true>(s, r, discount, a, l, lane);
    emit_decodes_direct<F>(s, a, env0, lane, 0, true, kargs_off);
    lds_wave_sync();
    emit_drain<F, false, true>(a, l, env0, lane, 0, true, true);
    SGW_STAMP(a, 11);
    emit_small_direct<F>(s, discount, a, l, env0, lane, 0, true);
    SGW_STAMP(a, 3);
  }
  SGW_STAMP_RT(a, 7);
}

template <class F, int TOUCH_END>
__device__ __forceinline__ void fork_body(const KArgs& a, const long long block, const unsigned kargs_off) {
  static_assert(!F::COOPERATIVE && F::WAVES == 1 && !F::PER_AGENT && F::NA == 1 && !has_views<F>::value && !cum_in_lds<F>::value &&
                !step_rereads<F>::value && !has_idle_round<F>::value && !has_board_part<F>::value && F::LDS_EXTRA == SGW_POW_LDS_BYTES /* the pow tables and nothing init_args would fill */, "");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int EW = FORK_EW, NT = FORK_THREADS;
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave_in_wg = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bool out_role = wave_in_wg >= EW;
  const int wv = out_role ? wave_in_wg - EW : wave_in_wg;          // env-wave within the workgroup
  const long long wave_id = block * EW + wv;
  const long long env0 = wave_id * WAVE;
  const long long env = env0 + lane;
  const bool real = env < a.n_envs;
  const bool wave_live = env0 < a.n_pad;                 // the last workgroup may hold fewer than EW env-waves

  SGW_STAMP_RT(a, 6);
  SGW_STAMP(a, 0);
  // k_engine's prologue in k_engine's order, the same in both roles and with no branch up to the barrier: level tables, state,
  // action, pow pieces, kernarg touch, then the LDS commits (a dead env-wave loads env-wave 0's data)
  TableStage ts;
  lds_tables_issue<NT>(ts, a.tables);
  const Lds l = lds_carve(smem, a.lp, F::LDS_EXTRA, wv);
  typename F::template CtxN<NT> cx;
  typename F::State s;
  F::load(s, a, wave_live ? env : (long long)lane);
  int action[1];
  {
    const bool have = a.actions != nullptr && real;
    const int8_t* ap = have ? a.actions + env : reinterpret_cast<const int8_t*>(a.tables);
    const int v = (int)*ap;
    action[0] = have ? v : 0;
  }
  F::template init_issue_n<NT>(cx);
  const uint32_t touch = kernarg_touch_issue<TOUCH_END>();
  lds_tables_commit<NT>(ts, smem);
  F::template init_ctx_n<NT>(cx, l);
  kernarg_touch_settle(touch);
  // THE ordering the fork rests on: every wave's loads of the OLD state have returned before any S wave stores the new one.  An
  // env-wave's two waves are in one workgroup, and __syncthreads() is `s_waitcnt vmcnt(0)` + s_barrier: each wave drains its own
  // loads before it arrives, so when the barrier opens all of the workgroup's state loads are back.  No store stands ahead of it.
  // (tests/test_step_fork_asm.py reads both off the assembly.)
  __syncthreads();
  if (!wave_live) return;
  SGW_STAMP(a, 1);
  if (out_role) fork_role<F, ROLE_OUTPUT>(s, action, a, l, wave_id, env0, lane, real, kargs_off);
  else fork_role<F, ROLE_STATE>(s, action, a, l, wave_id, env0, lane, real, kargs_off);
}

// the same parameter list as k_engine (SGW_HOT_ARGS, then KArgs: SGW_KARGS_OFFSET and the preload count hold); a kernel of its
// own name, not a k_engine instantiation
template <class F, class SH>
__global__ SGW_OCC __launch_bounds__(FORK_THREADS) void k_step_fork(uint64_t* hot_state, const uint8_t* hot_tables, const int8_t* hot_actions,
                                                                    long long hot_n_pad, long long hot_n_envs, int hot_words, const KArgs a_in) {
  KArgs a = a_in;
  a.state = hot_state; a.tables = hot_tables; a.actions = hot_actions; a.n_pad = hot_n_pad; a.n_envs = hot_n_envs; a.sp.words = hot_words;
  static_assert(SH::ON && SH::NSLOT == F::NU, "");
  SH::apply(a.sp);
  fork_body<F, SGW_KARGS_OFFSET + (int)sizeof(KArgs)>(a, (long long)blockIdx.x, SGW_KARGS_OFFSET);
}

// ---- heterogeneous launch: several engines (env families) in ONE grid --------------------------------------------------
// A mixed suite sharded over one GPU (BASELINE config 5: island_navigation_ex + boat_race_ex + safe_interruptibility) is three
// small launches otherwise -- 171 workgroups each on a 256-CU chip, three kernel boundaries per step.  Here workgroup b belongs
// to member m with first_block[m] <= b < first_block[m + 1]; it reads that member's KArgs from the kernarg segment and runs the
// member's family body.  Members are families whose workgroups have the same shape (GROUP_THREADS threads: four env-waves per
// step workgroup, two wave pairs per fused-rollout workgroup); the launch's dynamic LDS is the largest member's.
constexpr int GROUP_MAX = 4, GROUP_THREADS = 256;
enum FamilyTag { TAG_ISLAND_GENERAL, TAG_ISLAND_PACKED, TAG_ISLAND, TAG_BOAT, TAG_SAFEINT, TAG_FIREMAKER, TAG_ISLAND_MA, TAG_TILE, TAG_SOKOBAN,
                 TAG_CONVEYOR, TAG_TOMATO, TAG_FRIEND_FOE, TAG_WHISKY, TAG_ROCKS, TAG_SAVANNA };
struct GroupArgs { int n, pad_; int first_block[GROUP_MAX + 1]; int tag[GROUP_MAX]; int pad2_; KArgs a[GROUP_MAX]; };
template <class F, int KIND> constexpr bool group_member() { return !F::COOPERATIVE && wg_threads<F, KIND>() == GROUP_THREADS; }

// SGW_KARGS_OFFSET (where the fused rollout / the re-reading step kernels find the KArgs block in the kernarg segment) is tied
// to k_engine's parameter list: a struct with the same members in the same order has the same layout as the segment
struct EngineKernargMirror { uint64_t* hot_state; const uint8_t* hot_tables; const int8_t* hot_actions; long long hot_n_pad, hot_n_envs; int hot_words; KArgs a_in; };
static_assert(offsetof(EngineKernargMirror, a_in) == SGW_KARGS_OFFSET, "SGW_KARGS_OFFSET does not match k_engine's leading arguments (SGW_HOT_ARGS)");

// synthetic action stream materialised in HBM: int8 [T, N, A]
__global__ void k_fill_actions(int8_t* out, long long n, int A, int T, unsigned long long seed, long long step0,
                               long long env_id_base, int lo, int nact) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long total = (long long)T * n * A;
  for (; i < total; i += (long long)gridDim.x * blockDim.x) {
    int ag = (int)(i % A);
    long long e = (i / A) % n;
    long long t = i / (A * n);
    out[i] = (int8_t)synth_action(seed, env_id_base + e, step0 + t, ag, lo, nact);
  }
}

// out[c] = sum over waves of acc[wave][c]; one workgroup per column, fixed-order tree => deterministic
__global__ __launch_bounds__(256) void k_read_returns(double* acc, long long n_waves, int C, double* out, int clear) {
  __shared__ double part[256];
  const int c = blockIdx.x;
  double v = 0.0;
  for (long long w = threadIdx.x; w < n_waves; w += 256) v += acc[w * C + c];
  part[threadIdx.x] = v;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) part[threadIdx.x] += part[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = part[0];
  if (clear) for (long long w = threadIdx.x; w < n_waves; w += 256) acc[w * C + c] = 0.0;
}

// (sum of episode returns, #episodes) over envs whose step_type is LAST
__global__ void k_accumulate_returns(const double* cumulative, const uint8_t* step_type, long long n, int AK,
                                     double* accum) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool last = e < n && step_type[e] == ST_LAST;
  for (int k = 0; k < AK; ++k) {
    double v = wave_sum(last ? cumulative[e * AK + k] : 0.0);
    if ((threadIdx.x & (WAVE - 1)) == 0 && v != 0.0) atomicAdd(&accum[k], v);
  }
  double c = wave_sum(last ? 1.0 : 0.0);
  if ((threadIdx.x & (WAVE - 1)) == 0 && c != 0.0) atomicAdd(&accum[AK], c);
}

__global__ void k_pow(const double* x, double y, double* out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = sgw_glibc_pow(x[i], y);
}

// numpy PCG64 streams into the state of a family that owns a generator (its place: sgw_pcg64.hpp), nothing buffered
__global__ void k_set_rng(uint64_t* state, long long n_pad, long long n, int words, const uint64_t* pcg) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_pad) return;
  // padding lanes run the same code as real envs: give them a working stream too (an all-zero PCG state returns 0 for
  // ever, and Lemire's rejection loop never leaves on a constant 0)
  const uint64_t pad[4] = {0x9E3779B97F4A7C15ull, (uint64_t)e, 0ull, 1ull};
  for (int k = 0; k < 4; ++k) state[state_index(PCG64_WORD0 + k, e, words)] = e < n ? pcg[e * 4 + k] : pad[k];
  state[state_index(PCG64_FLAG_WORD, e, words)] &= ~(1ull << PCG64_FLAG_BIT);
  state[state_index(PCG64_U32_WORD, e, words)] &= ~PCG64_U32_MASK;
}

// canonical view of the state for sgw_get_state / sgw_set_state: uint64 [words][n_pad] <-> the engine's pair layout
__global__ void k_state_export(const uint64_t* state, long long n_pad, int words, uint64_t* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)words * n_pad) return;
  const int w = (int)(i / n_pad);
  const long long e = i - (long long)w * n_pad;
  out[i] = state[state_index(w, e, words)];
}
__global__ void k_state_import(uint64_t* state, long long n_pad, int words, const uint64_t* in) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)words * n_pad) return;
  const int w = (int)(i / n_pad);
  const long long e = i - (long long)w * n_pad;
  state[state_index(w, e, words)] = in[i];
}
// every env "never reset": step_type ST_NONE, termination reason absent, everything else zero
__global__ void k_state_init(uint64_t* state, long long n_pad, int words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= state_alloc_words(words, n_pad)) return;
  const bool word0 = ((i & 127) & 1) == 0 && ((i >> 7) % state_pairs(words)) == 0;
  state[i] = word0 ? (((uint64_t)ST_NONE << 32) | ((uint64_t)15 << 36)) : 0ull;
}

}  // namespace sgw
