// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the two roles of k_step_fork (csrc/sgw_kernels.hpp) side by side on the
// host.  The S role plays IslandL9Default's whole rules and keeps the state; the O role starts every step from the S role's
// state, plays the rules WITHOUT the regrowth pass (IslandL9Default::play_events) and must arrive at the same bytes in everything
// an output other than `metrics` shows: r[], discount, step_type, term, safety, frame, row, col, actual and cum.  A launch that
// asks for `metrics` makes the O role play the whole rules: then all nine metrics are the same bytes too.
// tests/test_step_fork_host.py builds it with the host sanitizers and pattern-initialised locals.
//
//   island_fork_check <spec>     one sgw_spec (the bytes of make_spec(...).native) that IslandL9Default accepts;
//                                prints "steps <n> regrowths <g> mismatches <m>", exit 0 iff m == 0
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_island.hpp"

using namespace sgw;
using F = IslandL9Default;
using State = F::State;
constexpr int NU = F::NU;

struct Host {
  sgw_spec spec; KArgs a; Lds l;
  std::vector<uint8_t> tables, lds;
};

static void setup(Host& h) {             // what sgw_create and the kernel's prologue put in front of play (island_rules_check.cpp)
  const sgw_spec& sp = h.spec;
  KSpec& k = h.a.sp;
  std::memset(&h.a, 0, sizeof(h.a));
  k.family = sp.family; k.H = sp.H; k.W = sp.W; k.HW = sp.H * sp.W; k.K = sp.K; k.M = sp.M; k.A = sp.A;
  k.max_iterations = sp.max_iterations; k.flags = sp.flags | F::F_PACKED; k.action_lo = sp.action_lo; k.n_actions = sp.n_actions;
  k.words = F::words(sp.K);
  std::memcpy(k.start_cell, sp.start_cell, sizeof(k.start_cell));
  kspec_derive(k);
  std::memcpy(k.dim_slot, sp.dim_slot, sizeof(k.dim_slot));
  std::memcpy(k.metric_slot, sp.metric_slot, sizeof(k.metric_slot));
  h.tables.assign(TABLE_BYTES, 0);
  std::memcpy(h.tables.data(), sp.static_board, k.HW);
  std::memcpy(h.tables.data() + SGW_MAX_CELLS, sp.art, k.HW);
  std::memcpy(h.tables.data() + 2 * SGW_MAX_CELLS, sp.aux, k.HW);
  std::memcpy(h.tables.data() + 3 * SGW_MAX_CELLS, sp.value_map, 512);
  std::memcpy(h.tables.data() + 3 * SGW_MAX_CELLS + 512, sp.params, SGW_N_PARAMS * 8);
  h.a.tables = h.tables.data(); h.a.T = 1;
  const int extra = F::LDS_EXTRA;
  h.lds.assign(lds_total_bytes(k.HW, k.A, k.K, k.M, 1, 0, 0, extra, 1, 1) + 64, 0);
  std::memcpy(h.lds.data(), h.tables.data(), TABLE_BYTES);
  h.a.lp = lds_plan(k.HW, k.A, k.K, k.M, 1, 0, 0);
  h.l = lds_carve(h.lds.data(), h.a.lp, extra, 0);
  // the pow tables as the forked kernel's 512-thread workgroup stages them: one piece per thread
  for (int t = 0; t < 512; ++t) { threadIdx.x = t; F::CtxN<512> cx; F::init_issue_n<512>(cx); F::init_ctx_n<512>(cx, h.l); }
}

// fork_role's step for one env: auto-reset, or play + step bookkeeping + cum += r.  REGROW: the whole rules.
template <bool REGROW> static double tick(State& s, int action, const Host& h, double (&r)[NU]) {
  for (int u = 0; u < NU; ++u) r[u] = 0.0;
  double discount = __builtin_nan("");
  const int a1[1] = {action};
  if (s.step_type >= ST_LAST) {
    F::begin_episode(s, h.a, h.l, 0, 0);
  } else {
    discount = REGROW ? F::play(s, a1, h.a, h.l, r, 0) : F::play_events(s, a1, h.a, h.l, r, 0);
    const bool over = (discount == 0.0) || (s.frame >= h.a.sp.max_iterations);
    s.step_type = over ? ST_LAST : ST_MID;
    if (over && s.term == 15) s.term = SGW_MAX_STEPS;
    for (int u = 0; u < NU; ++u) s.cum[u] += r[u];
  }
  return discount;
}

// what the O role's outputs other than `metrics` read
static bool same_outputs(const State& x, const State& y) {
  return x.row == y.row && x.col == y.col && x.frame == y.frame && x.step_type == y.step_type && x.term == y.term && x.actual == y.actual &&
         x.safety == y.safety && std::memcmp(x.cum, y.cum, NU * 8) == 0;
}
static bool same_metrics(const State& x, const State& y) {
  for (int id = 0; id < F::NMETRIC; ++id) { const double p = F::metric(x, id), q = F::metric(y, id); if (std::memcmp(&p, &q, 8) != 0) return false; }
  return true;
}

// the project's action stream in 0..4; a seeded 2 % (agent stream 1 of the same generator) replaced by QUIT / out-of-range values
static int action_of(unsigned long long seed, long long env, long long t) {
  const U4 pick = philox4x32_10((uint32_t)t, TAG_ACTION, 1u, 0u, (uint32_t)seed, (uint32_t)env);
  const int odd[5] = {9, -1, 5, 10, 127};
  if (pick.x % 50u == 0u) return odd[pick.y % 5u];
  return synth_action(seed, env, t, 0, 0, 5);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  Host h;
  if (std::fread(&h.spec, sizeof(h.spec), 1, in) != 1) return 2;
  std::fclose(in);
  if (!F::matches(h.spec)) { std::fprintf(stderr, "the spec is not the compiled one\n"); return 3; }
  setup(h);

  long long steps = 0, regrowths = 0, bad = 0;
  for (long long env = 0; env < 2048; ++env) {
    State s; std::memset(&s, 0, sizeof(s));
    s.step_type = ST_NONE; s.term = 15;                     // sgw_create's initial state: the first step resets
    for (long long t = 0; t < 300; ++t) {
      const int action = action_of(0xF02Cull, env, t);
      const State old = s;
      double rs[NU], ro[NU], rm[NU];
      const double ds = tick<true>(s, action, h, rs);        // the S role: its state goes on
      State o = old, m = old;                               // the O role, handed the S role's state every step
      const double d_o = tick<false>(o, action, h, ro);      // ... regrowth skipped
      const double d_m = tick<true>(m, action, h, rm);       // ... regrowth enabled (`metrics` asked for)
      ++steps;
      if (old.step_type < ST_LAST && (s.d_avail != o.d_avail || s.f_avail != o.f_avail || s.d_frac != o.d_frac || s.f_frac != o.f_frac)) ++regrowths;
      const bool ok = same_outputs(s, o) && std::memcmp(rs, ro, sizeof(rs)) == 0 && std::memcmp(&ds, &d_o, 8) == 0 &&
                      same_outputs(s, m) && same_metrics(s, m) && std::memcmp(rs, rm, sizeof(rs)) == 0 && std::memcmp(&ds, &d_m, 8) == 0;
      if (!ok && bad++ < 10) std::fprintf(stderr, "the roles differ: env %lld step %lld action %d cell (%d, %d)\n", env, t, action, old.row, old.col);
    }
  }
  std::printf("steps %lld regrowths %lld mismatches %lld\n", steps, regrowths, bad);
  return bad == 0 ? 0 : 1;
}
