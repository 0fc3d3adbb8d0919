// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the two rules providers of csrc/sgw_island.hpp side by side on the
// host.  IslandRulesRuntime (any spec, read from the launch's tables) against IslandRulesL9 (level 9's default rule set as
// compile-time constants), with and without the level masks, on the same states and actions; everything is compared as bytes.
// tests/test_island_rules.py builds it with the host sanitizers and pattern-initialised locals.
//
//   island_rules_check run <spec>        one sgw_spec (the bytes of make_spec(...).native) that the constant provider accepts:
//                                        trajectories, then the state sweep; prints "calls <n> mismatches <m>", exit 0 iff m == 0
//   island_rules_check matches <specs>   any number of sgw_spec blobs: prints one character per spec, '1' = IslandL9Default::matches
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_island.hpp"

using namespace sgw;
using F = IslandPacked;
using State = F::State;
constexpr int NU = F::NU;

struct Host {
  sgw_spec spec; KArgs a; Lds l;
  std::vector<uint8_t> tables, lds;
};

static void setup(Host& h) {             // what sgw_create and k_engine's prologue put in front of play (host_families.cpp)
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
  for (int t = 0; t < F::ENV_WAVES_MAX * WAVE; ++t) { threadIdx.x = t; F::Ctx cx; F::init_issue(cx); F::init_ctx(cx, h.l); }
}

// field by field: State has padding bytes, which a copy need not carry
static bool same_state(const State& x, const State& y) {
  const bool ints = x.row == y.row && x.col == y.col && x.frame == y.frame && x.step_type == y.step_type && x.term == y.term &&
                    x.actual == y.actual && x.safety == y.safety && x.gap_v == y.gap_v && x.drink_v == y.drink_v &&
                    x.food_v == y.food_v && x.gold_v == y.gold_v && x.silver_v == y.silver_v && x.episode == y.episode;
  return ints && std::memcmp(&x.drink_sat, &y.drink_sat, 6 * 8) == 0 && std::memcmp(x.cum, y.cum, NU * 8) == 0;
}

// the three providers
struct Runtime { static double play(State& s, int act, const Host& h, double (&r)[NU]) { const int a1[1] = {act}; return F::play(s, a1, h.a, h.l, r, 0); }
                 static void begin(State& s, const Host& h) { F::begin_episode(s, h.a, h.l, 0, 0); } };
template <bool MASKS> struct Constant {
  using R = IslandRulesL9<MASKS>;
  static double play(State& s, int act, const Host& h, double (&r)[NU]) { return F::play_rules(R(h.a, h.l), s, act, h.l, r); }
  static void begin(State& s, const Host& h) { F::begin_episode_rules<R>(s, h.a, h.l); }
};
struct Shipped { static double play(State& s, int act, const Host& h, double (&r)[NU]) { const int a1[1] = {act}; return IslandL9Default::play(s, a1, h.a, h.l, r, 0); }
                 static void begin(State& s, const Host& h) { IslandL9Default::begin_episode(s, h.a, h.l, 0, 0); } };

// k_engine's non-cooperative step for one env: auto-reset, or play + step bookkeeping + cum += r
template <class P> static double tick(State& s, int action, const Host& h, double (&r)[NU]) {
  for (int u = 0; u < NU; ++u) r[u] = 0.0;
  double discount = __builtin_nan("");
  if (s.step_type >= ST_LAST) {
    P::begin(s, h);
  } else {
    discount = P::play(s, action, h, r);
    const bool over = (discount == 0.0) || (s.frame >= h.a.sp.max_iterations);
    s.step_type = over ? ST_LAST : ST_MID;
    if (over && s.term == 15) s.term = SGW_MAX_STEPS;
    for (int u = 0; u < NU; ++u) s.cum[u] += r[u];
  }
  return discount;
}

static long long calls = 0, bad = 0;
template <class P> static void against_runtime(const State& s0, int action, const Host& h, const State& want, const double (&rw)[NU], double dw,
                                               const char* who) {
  State s = s0; double r[NU];
  const double d = tick<P>(s, action, h, r);
  ++calls;
  if (!same_state(s, want) || std::memcmp(r, rw, sizeof(r)) != 0 || std::memcmp(&d, &dw, 8) != 0) {
    if (bad++ < 10) std::fprintf(stderr, "%s differs: cell (%d, %d) action %d frame %d\n", who, s0.row, s0.col, action, s0.frame);
  }
}
static State step_all(const State& s0, int action, const Host& h) {
  State want = s0; double rw[NU];
  const double dw = tick<Runtime>(want, action, h, rw);
  against_runtime<Constant<false>>(s0, action, h, want, rw, dw, "constant flags and parameters");
  against_runtime<Constant<true>>(s0, action, h, want, rw, dw, "constant flags, parameters and level masks");
  against_runtime<Shipped>(s0, action, h, want, rw, dw, "IslandL9Default");
  return want;
}

// the project's action stream in 0..4; a seeded 2 % (agent stream 1 of the same generator) replaced by QUIT / out-of-range values
static int action_of(unsigned long long seed, long long env, long long t) {
  const U4 pick = philox4x32_10((uint32_t)t, TAG_ACTION, 1u, 0u, (uint32_t)seed, (uint32_t)env);
  const int odd[5] = {9, -1, 5, 10, 127};
  if (pick.x % 50u == 0u) return odd[pick.y % 5u];
  return synth_action(seed, env, t, 0, 0, 5);
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = std::fopen(argv[2], "rb");
  if (!in) return 2;
  if (!std::strcmp(argv[1], "matches")) {
    sgw_spec sp;
    while (std::fread(&sp, sizeof(sp), 1, in) == 1) std::putchar(IslandL9Default::matches(sp) ? '1' : '0');
    std::putchar('\n');
    return 0;
  }
  Host h;
  if (std::fread(&h.spec, sizeof(h.spec), 1, in) != 1) return 2;
  if (!IslandL9Default::matches(h.spec)) { std::fprintf(stderr, "the spec is not the compiled one\n"); return 3; }
  setup(h);

  // ---- trajectories: 2 048 envs x 300 steps
  for (long long env = 0; env < 2048; ++env) {
    State s; std::memset(&s, 0, sizeof(s));
    s.step_type = ST_NONE; s.term = 15;                     // sgw_create's initial state: the first step resets
    for (long long t = 0; t < 300; ++t) s = step_all(s, action_of(0xC0DEull, env, t), h);
  }
  const long long traj_calls = calls;

  // ---- state sweep: (cell, action, frame) in full, the other coordinates drawn per call from a fixed seed
  const int actions[6] = {0, 1, 2, 3, 4, 9}, frames[3] = {0, 98, 99};
  const double avail[8] = {0, 1, 3, 9, 10, 13, 19, 20}, sat[9] = {-21, -20, -19, -1, 0, 1, 3, 4, 5};
  std::vector<double> frac = {0.0, 0.25, 0.98, std::nextafter(1.0, 0.0)};
  for (int i = 0; i < 64; ++i) frac.push_back((double)(rnd() >> 11) * (1.0 / 9007199254740992.0));
  int cells = 0;
  for (int cell = 0; cell < h.a.sp.HW; ++cell) {
    if (h.spec.static_board[cell] == '#') continue;
    ++cells;
    for (int ai = 0; ai < 6; ++ai) for (int fi = 0; fi < 3; ++fi) for (int rep = 0; rep < 3200; ++rep) {
      State s; std::memset(&s, 0, sizeof(s));
      s.row = cell / h.a.sp.W; s.col = cell % h.a.sp.W; s.frame = frames[fi]; s.step_type = ST_MID; s.term = 15;
      s.actual = (int)(rnd() % 6) - 1; s.safety = (int)(rnd() % 4); s.episode = 1;
      s.gap_v = (uint32_t)(rnd() % 100); s.drink_v = (uint32_t)(rnd() % 100); s.food_v = (uint32_t)(rnd() % 100);
      s.gold_v = (uint32_t)(rnd() % 100); s.silver_v = (uint32_t)(rnd() % 100);
      s.d_avail = avail[rnd() % 8]; s.f_avail = avail[rnd() % 8];
      s.d_frac = frac[rnd() % frac.size()]; s.f_frac = frac[rnd() % frac.size()];
      s.drink_sat = sat[rnd() % 9]; s.food_sat = sat[rnd() % 9];
      for (int u = 0; u < NU; ++u) s.cum[u] = (double)((long long)(rnd() % 201) - 100);
      step_all(s, actions[ai], h);
    }
  }
  std::printf("cells %d trajectory_calls %lld calls %lld mismatches %lld\n", cells, traj_calls, calls, bad);
  return bad == 0 ? 0 : 1;
}
