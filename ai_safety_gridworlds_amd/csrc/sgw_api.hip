// sgw_api.hip -- host side of libsgw.so: the C ABI declared in include/sgw.h.
// Thin by design: validates arguments, owns the engine's device state, launches k_engine<F>.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/sgw.h"
#include "sgw_boat.hpp"
#include "sgw_conveyor.hpp"
#include "sgw_firemaker.hpp"
#include "sgw_friendfoe.hpp"
#include "sgw_island_ma.hpp"
#include "sgw_island.hpp"
#include "sgw_kernels.hpp"
#include "sgw_observe.hpp"
#include "sgw_rocks.hpp"
#include "sgw_safeint.hpp"
#include "sgw_savanna.hpp"
#include "sgw_sokoban.hpp"
#include "sgw_tile.hpp"
#include "sgw_tomato.hpp"
#include "sgw_whisky.hpp"
#include "sgw_group.hpp"
#include "sgw_savanna_layers.hpp"
#include "sgw_coords.hpp"
#include "sgw_episodes.hpp"
#include "sgw_seed.hpp"
#include "sgw_copy.hpp"
#include "sgw_scalarise.hpp"
#include "sgw_policy.hpp"
#include "sgw_whatif.hpp"
#include "sgw_targets.hpp"
#include "sgw_learn.hpp"
#include "sgw_softmax.hpp"

using namespace sgw;

// Host copy of the pow tables: sgw_create checks the RUNNING libm against them (see pow_selfcheck).
namespace sgw_host_pow {
#undef SGW_POW_TABLE
#define SGW_POW_TABLE static const
#include "sgw_pow_tables.inc"
}

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, const char* detail = "") {
  snprintf(g_err, sizeof(g_err), fmt, detail);
  return code;
}
#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      snprintf(g_err, sizeof(g_err), "%s failed: %s", #expr, hipGetErrorString(e_));     \
      return SGW_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

// ---- the graph cache of sgw_step_n, sgw_group_step_n and sgw_step_full ------------------------------------------------------
// One host launch costs ~5 us of CPU on this runtime -- as much as the smaller families' whole step kernel, and three times
// that for a mixed suite issued from one thread.  A caller that steps from the same device buffers again (the usual loop:
// one actions buffer refilled in place) gets its launches captured into a hipGraph the second time the same arguments are
// seen and replayed from then on.  SGW_STEP_GRAPHS=0 turns this off.
static int step_graphs_min_T() {
  static int v = -1;
  if (v < 0) { const char* s = getenv("SGW_STEP_GRAPHS"); v = (s && atoi(s) == 0) ? (1 << 30) : 8; }
  return v;
}

// What a call was made with, for N engines (1, or the members of a group).  epochs: the arg_epoch of every engine whose KArgs the
// capture holds by value; they are no part of a key's identity (same()) but say whether the entry found under it is stale.
template <int N> struct GraphKey {
  const int8_t* actions[N];
  sgw_out outs[N];
  sgw_extras ex;                                // sgw_step_full
  sgw_policy pol;                               // sgw_policy_step_n: the policy by value, and where step 0 reads its observation
  const void* obs0;
  unsigned long long epochs[N];
  int n, T, write_every, accumulate, has_out;
  int sampled;                                  // sgw_policy_sample_step_n: 1, and its beta2 (a greedy call never shares a sampled call's graph)
  float beta2;
  bool same(const GraphKey& o) const {
    if (actions[0] != o.actions[0] || n != o.n || T != o.T || write_every != o.write_every || accumulate != o.accumulate ||
        has_out != o.has_out || sampled != o.sampled || memcmp(&beta2, &o.beta2, sizeof(beta2)) != 0) return false;
    return memcmp(actions, o.actions, sizeof(actions[0]) * n) == 0 && memcmp(outs, o.outs, sizeof(sgw_out) * n) == 0 &&
           memcmp(&ex, &o.ex, sizeof(ex)) == 0 && memcmp(&pol, &o.pol, sizeof(pol)) == 0 && obs0 == o.obs0;
  }
};

// what the caches of one owner (an engine, a group) share: the private stream captures are made on, the use counter
struct GraphOwner { int device; hipStream_t capture_stream; long long tick; };

template <int N> struct GraphCache {
  struct Entry { GraphKey<N> key; long long nodes, last_use; hipGraphExec_t exec; };
  size_t max_entries;
  long long max_nodes;                          // kernel nodes of all entries together; 0: no such bound
  const char* captured;                         // (error text) what a capture holds
  std::vector<Entry> entries;

  void clear() {
    for (auto& g : entries) if (g.exec) (void)hipGraphExecDestroy(g.exec);
    entries.clear();
  }

  // launches(stream) issues the call's launches; node_count: how many kernel nodes a capture of them holds
  template <class L> int run(GraphOwner& own, const GraphKey<N>& key, long long node_count, L&& launches, hipStream_t st, const char* what) {
    Entry* hit = nullptr;
    for (auto& g : entries) if (g.key.same(key)) { hit = &g; break; }
    if (!hit) {                                 // first sighting: remember the arguments, launch directly
      // bounded: drop the least recently used captures
      auto nodes = [&]() { long long n = node_count; for (auto& g : entries) n += g.nodes; return n; };
      while (!entries.empty() && (entries.size() >= max_entries || (max_nodes && nodes() > max_nodes))) {
        size_t worst = 0;
        for (size_t i = 1; i < entries.size(); ++i) if (entries[i].last_use < entries[worst].last_use) worst = i;
        if (entries[worst].exec) (void)hipGraphExecDestroy(entries[worst].exec);
        entries.erase(entries.begin() + worst);
      }
      entries.push_back(Entry{key, node_count, ++own.tick, nullptr});
      return launches(st);
    }
    hit->last_use = ++own.tick;
    if (memcmp(hit->key.epochs, key.epochs, sizeof(key.epochs)) != 0) {      // a setter changed what the captured KArgs hold: seen anew, launch directly
      if (hit->exec) (void)hipGraphExecDestroy(hit->exec);
      hit->exec = nullptr;
      memcpy(hit->key.epochs, key.epochs, sizeof(key.epochs));
      return launches(st);
    }
    if (!hit->exec) {                           // second sighting: capture (on the owner's own stream; nothing executes) and instantiate
      HIP_TRY(hipSetDevice(own.device));
      if (!own.capture_stream) HIP_TRY(hipStreamCreateWithFlags(&own.capture_stream, hipStreamNonBlocking));
      HIP_TRY(hipStreamBeginCapture(own.capture_stream, hipStreamCaptureModeThreadLocal));
      const int rc = launches(own.capture_stream);
      hipGraph_t graph = nullptr;
      const hipError_t ec = hipStreamEndCapture(own.capture_stream, &graph);
      if (rc || ec != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        if (rc) return rc;
        snprintf(g_err, sizeof(g_err), "%s: stream capture%s failed", what, captured);
        return SGW_ERR_HIP;
      }
      const hipError_t ei = hipGraphInstantiate(&hit->exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (ei != hipSuccess) { hit->exec = nullptr; return fail(SGW_ERR_HIP, "%s: hipGraphInstantiate failed", what); }
    }
    HIP_TRY(hipSetDevice(own.device));
    HIP_TRY(hipGraphLaunch(hit->exec, st));
    return SGW_OK;
  }
};

struct sgw_engine {
  sgw_spec spec;
  KSpec ks;
  int device;
  long long n_envs, n_pad, env_id_base;
  uint8_t* tables_dev;     // static_board | art | aux | value_map
  uint64_t* state_dev;     // pair layout [env-wave][word pair][lane][2] (sgw_common.hpp state_index); canonical [words][n_pad] only through sgw_get/set_state
  const uint8_t* ep_bits;
  int ep_bits_n;
  unsigned long long ep_seed;
  const double* rand_stream;
  int rand_n;
  unsigned long long rand_seed;
  double* acc_dev;         // [n_pad/64 * SGW_ACC_PARTS][A*K+1] episodic-return accumulators, one row per 16 envs (lazily allocated)
  int rng_set;
  double* ftable_dev;      // sgw_set_family_table
  long long ftable_n;
  // sgw_step_n: the T launches of one (actions, T, outputs) call, captured once and replayed as a hipGraph: at most 256
  // captures and 64 Ki kernel nodes in all.  sgw_step_full: one captured graph per (actions, out, extras) triple, at most 16
  GraphOwner graph_owner;
  GraphCache<1> graphs{256, 65536, " of the step launches"}, full_graphs{16, 0, ""};
  // sgw_policy_step_n: the 2T + 1 launches of one closed-loop call, in a cache of their own (they never evict sgw_step_n's): at most 64
  GraphCache<1> policy_graphs{64, 0, " of the policy and step launches"};
  unsigned lds_cap_raised; // bit KIND (+ 3 for the shaped step kernel, + 4 for the BigViews variant; bit 20 for a shaped kernel with compiled rules, bit 21 for k_step_fork): this engine's k_engine<F, KIND> may use more than 64 KiB of dynamic LDS (set once)
  int step_shape;          // 1 + the ShapedSteps entry whose kernel runs this engine's one-step launches, 0 = the generic kernel
  int step_rules;          // 1: that entry's kernel with the spec's rule set compiled in runs them (ShapedStep::Rules), 0: the entry's own family
  int step_fork;           // 1: the one-step launches run k_step_fork (a state wave and an output wave per env-wave), see engine_step_fork
  // bumped by drop_graphs: a cache entry records its engines' epochs when it is seen and is stale once one moved
  unsigned long long arg_epoch;
};

// any setter that changes what a launch's arguments hold invalidates the captures, this engine's and those of the groups it is
// a member of (they hold its KArgs by value): each is destroyed when its entry is next found (GraphCache::run)
static void drop_graphs(sgw_engine* e) { ++e->arg_epoch; }

static size_t acc_bytes(const sgw_engine* e) {              // [env-waves * parts][A*K+1] doubles
  return (size_t)(e->spec.A * e->spec.K + 1) * (size_t)(e->n_pad / WAVE * SGW_ACC_PARTS) * 8;
}

// island_navigation_ex: the packed (i16) state when the spec proves it exact (sgw_island.hpp); SGW_ISLAND_PLAIN_STATE in the
// environment forces the plain f64 state (tests run every fixture through both).
static bool island_packable(const sgw_spec& sp) { return !getenv("SGW_ISLAND_PLAIN_STATE") && Island::packable(sp); }

static int family_words(const sgw_spec& sp) {
  switch (sp.family) {
    case SGW_ISLAND_NAVIGATION_EX: return island_packable(sp) ? IslandPacked::words(sp.K) : Island::words(sp.K);
    case SGW_BOAT_RACE_EX:
    case SGW_BOAT_RACE: return Boat::words(sp.K, sp.H * sp.W);
    case SGW_SAFE_INTERRUPTIBILITY: return SafeInt::words();
    case SGW_FIREMAKER_EX_MA: return Firemaker::words();
    case SGW_ISLAND_NAVIGATION_EX_MA: return sp.H * sp.W > 64 ? IslandMaWide::words(sp.K) : IslandMa::words(sp.K);
    case SGW_TILE_EVENTS: return Tile::words();
    case SGW_SIDE_EFFECTS_SOKOBAN: return Sokoban::words();
    case SGW_CONVEYOR_BELT: return Conveyor::words();
    case SGW_TOMATO_WATERING: return Tomato::words();
    case SGW_FRIEND_FOE: return FriendFoe::words();
    case SGW_WHISKY_GOLD: return Whisky::words();
    case SGW_ROCKS_DIAMONDS: return Rocks::words();
    case SGW_AINTELOPE_SAVANNA: return Savanna::words(sp.K);
    default: return -1;
  }
}

// step_type / term_reason / safety are [N_pad, A] for these families: the host's statement of the kernels' F::PER_AGENT
static bool spec_per_agent(const sgw_spec& sp) { return sp.family == SGW_ISLAND_NAVIGATION_EX_MA || sp.family == SGW_AINTELOPE_SAVANNA; }
static_assert(IslandMa::PER_AGENT && IslandMaWide::PER_AGENT && Savanna::PER_AGENT, "spec_per_agent names the families whose kernels write per-agent columns");
static_assert(!Island::PER_AGENT && !Firemaker::PER_AGENT, "... and no other (firemaker_ex_ma has several agents and one column)");

// The rows of the outputs, one entry per field of struct sgw_out in its order: the columns of one env's row (the element size
// is the field's own).  offset_out and out_row_bytes (sgw_out_row_bytes, sgw_copy_envs) both evaluate it.
//   HW board cells, AK reward columns, A agents, PA per-agent columns (spec_per_agent ? A : 1), A2 two per agent, M metrics,
//   VB bytes of the agents' windows, ONE a scalar, SAV per-agent columns of aintelope_savanna and no such output elsewhere
enum OutCols { OC_HW, OC_AK, OC_A, OC_PA, OC_A2, OC_M, OC_VB, OC_ONE, OC_SAV };
#define SGW_OUT_FIELDS(X)                                                                                                    \
  X(board, HW) X(obs_board, HW) X(reward, AK) X(cumulative, AK) X(step_type, A) X(term_reason, PA) X(actual_action, A)       \
  X(discount, ONE) X(hidden, ONE) X(safety, PA) X(metrics, M) X(frame, ONE) X(agent_pos, A2) X(agent_flags, A)               \
  X(safety2, SAV) X(views, VB) X(obs_views, VB) X(done, A) X(obs_dir, A) X(act_dir, A)
struct OutField { int elem_bytes; OutCols cols; };
#define SGW_OUT_ENTRY(name, cols) {(int)sizeof(*sgw_out{}.name), OC_##cols},
static constexpr OutField OUT_FIELDS[] = {SGW_OUT_FIELDS(SGW_OUT_ENTRY)};
#define SGW_OUT_INDEX(name, cols) OF_##name,
enum { SGW_OUT_FIELDS(SGW_OUT_INDEX) OF_COUNT };
#define SGW_OUT_PLACE(name, cols) static_assert(offsetof(sgw_out, name) == OF_##name * sizeof(void*), "OUT_FIELDS is in the order of struct sgw_out");
SGW_OUT_FIELDS(SGW_OUT_PLACE)
#undef SGW_OUT_ENTRY
#undef SGW_OUT_INDEX
#undef SGW_OUT_PLACE
static_assert(OF_COUNT == COPY_PLANES && sizeof(sgw_out) == COPY_PLANES * sizeof(void*), "sgw_out is COPY_PLANES pointers: offset_out and sgw_copy_envs walk it as an array");

static long long kspec_view_total(const sgw_spec& sp) {
  long long off = 0;
  for (int a = 0; a < sp.A; ++a) if (sp.view_radius[a][0] >= 0) off += (long long)(sp.view_radius[a][0] + sp.view_radius[a][1] + 1) * (sp.view_radius[a][2] + sp.view_radius[a][3] + 1);
  return off;
}

// Bytes of one env's row of the field-th output of struct sgw_out (0: the family has no such output, negative: no such field)
static long long out_row_bytes(const sgw_spec& sp, int field) {
  if (field < 0 || field >= COPY_PLANES) return -1;
  const long long A = sp.A, PA = spec_per_agent(sp) ? A : 1;
  long long cols = 0;
  switch (OUT_FIELDS[field].cols) {
    case OC_HW: cols = sp.H * sp.W; break;
    case OC_AK: cols = A * sp.K; break;
    case OC_A: cols = A; break;
    case OC_PA: cols = PA; break;
    case OC_A2: cols = A * 2; break;
    case OC_M: cols = sp.M; break;
    case OC_VB: cols = kspec_view_total(sp); break;
    case OC_ONE: cols = 1; break;
    case OC_SAV: cols = sp.family == SGW_AINTELOPE_SAVANNA ? PA : 0; break;
  }
  return cols * OUT_FIELDS[field].elem_bytes;
}

// step t of a [T, N_pad, ...] buffer of every output that is set.  (safety2 outside aintelope_savanna does not move: its row is
// 0 bytes there, and no launch sees it -- prepare_args refuses that output.)
static void offset_out(sgw_out& o, const sgw_spec& sp, long long n_pad, long long t) {
  for (int f = 0; f < COPY_PLANES; ++f) {
    char* p;
    memcpy(&p, reinterpret_cast<char*>(&o) + f * sizeof(p), sizeof(p));
    if (!p) continue;
    p += t * n_pad * out_row_bytes(sp, f);
    memcpy(reinterpret_cast<char*>(&o) + f * sizeof(p), &p, sizeof(p));
  }
}

// The device pow restates glibc's algorithm over tables extracted from the BUILD host's libm (csrc/sgw_pow_tables.inc);
// the reference's math.pow is the RUNNING host's libm pow.  When the two differ (another glibc, a non-FMA dispatch) parity
// of resource regrowth would fail later and quietly, so the families that regrow resources refuse to construct instead.
// Probe: the regrowth domain (halves and pseudo-random x in [1, 61]) at three exponents.  Returns the mismatch count.
static long pow_selfcheck_run() {
  long bad = 0;
  unsigned long long s = 88172645463325252ULL;
  const double ys[3] = {1.1, 1.05, 1.5};
  for (int i = 0; i < 4096; ++i) {
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    double x = 1.0 + 60.0 * ((double)(s >> 11) / 9007199254740992.0);
    if (i < 240) x = 1.0 + 0.25 * i;
    const double y = ys[i % 3];
    const double want = pow(x, y);
    const double got = sgw_glibc_pow_core(x, y, sgw_host_pow::SGW_POW_LOG_HEAD, sgw_host_pow::SGW_POW_EXP_HEAD,
                                          sgw_host_pow::SGW_POW_LOG_TAB, sgw_host_pow::SGW_POW_EXP_TAB);
    if (memcmp(&want, &got, 8) != 0) ++bad;
  }
  return bad;
}
static int engine_step_shape(const sgw_engine* e);      // (below the launch dispatch)
static int engine_step_rules(const sgw_engine* e);
static int engine_step_fork(const sgw_engine* e);

static long pow_selfcheck() {
  static const long cached = pow_selfcheck_run();           // C++11: initialised once, thread-safe
  return cached;
}

extern "C" {

int sgw_abi_version(void) { return SGW_ABI_VERSION; }
const char* sgw_last_error(void) { return g_err; }
#ifndef SGW_BUILD_COMPILER
#define SGW_BUILD_COMPILER "unknown (built outside ai_safety_gridworlds_amd/build.py: not linted)"
#endif
const char* sgw_build_info(void) { return SGW_BUILD_COMPILER; }
int sgw_sizeof_spec(void) { return (int)sizeof(sgw_spec); }
int sgw_sizeof_out(void) { return (int)sizeof(sgw_out); }
int sgw_sizeof_extras(void) { return (int)sizeof(sgw_extras); }
int64_t sgw_pow_selfcheck(void) { return (int64_t)pow_selfcheck(); }

int sgw_create(const sgw_spec* spec, int64_t n_envs, int64_t env_id_base, int device, sgw_engine** out_engine) {
  if (!spec || !out_engine) return fail(SGW_ERR_ARG, "sgw_create: null argument");
  *out_engine = nullptr;
  if (n_envs <= 0) return fail(SGW_ERR_ARG, "sgw_create: n_envs must be positive");
  const int HW = spec->H * spec->W;
  if (spec->H <= 0 || spec->W <= 0 || HW > SGW_MAX_CELLS || spec->H > 255 || spec->W > 255)
    return fail(SGW_ERR_ARG, "sgw_create: board size out of range");
  if (spec->K < 1 || spec->K > SGW_MAX_K || spec->M < 0 || spec->M > SGW_MAX_M || spec->A < 1 ||
      spec->A > SGW_MAX_AGENTS)
    return fail(SGW_ERR_ARG, "sgw_create: K/M/A out of range");
  if (spec->max_iterations < 1 || spec->max_iterations > 65535)
    return fail(SGW_ERR_ARG, "sgw_create: max_iterations must be in [1, 65535]");
  for (int ag = 0; ag < spec->A; ++ag)
    if (spec->start_cell[ag] < 0 || spec->start_cell[ag] >= HW)
      return fail(SGW_ERR_ARG, "sgw_create: start_cell outside the board");
  for (int ag = 0; ag < SGW_MAX_AGENTS; ++ag)
    for (int u = 0; u < SGW_MAX_K; ++u)
      if (spec->dim_slot[ag][u] >= spec->A * spec->K) return fail(SGW_ERR_ARG, "sgw_create: dim_slot >= A*K");
  for (int m = 0; m < SGW_MAX_M; ++m)
    if (spec->metric_slot[m] >= spec->M && spec->metric_slot[m] >= 0)
      return fail(SGW_ERR_ARG, "sgw_create: metric_slot >= M");
  if (spec->family == SGW_AINTELOPE_SAVANNA && (HW > 192 || spec->A != 2))
    return fail(SGW_ERR_ARG, "sgw_create: aintelope_savanna holds a layer in 3 x 64 bits (H*W <= 192) and lays out two agents (A = 2)");
  if (spec->family == SGW_ISLAND_NAVIGATION_EX_MA && (HW > 128 || spec->A != 2))
    return fail(SGW_ERR_ARG, "sgw_create: island_navigation_ex_ma keeps its map in 4 or 8 x 16 nibbles (H*W <= 128) and has two agents");
  // a round of A plays ends an episode on a frame of up to max_iterations + A - 1, and every family keeps the frame in 16 bits
  // (read back by the idle rounds after an episode's end, which report the frame without playing)
  int players = 1;
  if (spec->family == SGW_FIREMAKER_EX_MA)
    players = 3 - ((spec->flags & Firemaker::F_NO_AGENT2) ? 1 : 0) - ((spec->flags & Firemaker::F_NO_SUP) ? 1 : 0);
  else if (spec->family == SGW_ISLAND_NAVIGATION_EX_MA) players = 2;
  else if (spec->family == SGW_AINTELOPE_SAVANNA) players = (spec->flags & Savanna::F_TWO) ? 2 : 1;
  if (spec->max_iterations > 65535 - (players - 1))
    return fail(SGW_ERR_ARG, "sgw_create: max_iterations + agents - 1 must fit the frame's 16 bits (max_iterations <= 65535 - (agents - 1))");
  if (spec->family == SGW_FIREMAKER_EX_MA && !(spec->params[Firemaker::P_RELOAD] <= 65535.0))
    return fail(SGW_ERR_ARG, "sgw_create: firemaker_ex_ma keeps the stop button's countdown in 16 bits (reload = 1 + 1 + duration <= 65535)");
  const int words = family_words(*spec);
  if (words < 0) return fail(SGW_ERR_UNSUPPORTED, "sgw_create: unknown game family");
  if ((spec->family == SGW_ISLAND_NAVIGATION_EX || spec->family == SGW_ISLAND_NAVIGATION_EX_MA ||
       spec->family == SGW_AINTELOPE_SAVANNA) && pow_selfcheck() != 0 && !getenv("SGW_ALLOW_LIBM_MISMATCH"))
    return fail(SGW_ERR_UNSUPPORTED, "sgw_create: this host's libm pow() differs from the tables the device pow was built from "
                "(csrc/sgw_pow_tables.inc, glibc 2.35 x86-64 FMA build): resource regrowth would not match the reference's "
                "math.pow here.  Regenerate the tables on this host (tools/gen_pow_tables.py) and rebuild, or set "
                "SGW_ALLOW_LIBM_MISMATCH=1");

  HIP_TRY(hipSetDevice(device));
  sgw_engine* e = new (std::nothrow) sgw_engine();
  if (!e) return fail(SGW_ERR_NOMEM, "sgw_create: out of host memory");
  e->spec = *spec;
  e->device = device;
  e->n_envs = n_envs;
  e->n_pad = (n_envs + SGW_ENV_ALIGN - 1) / SGW_ENV_ALIGN * SGW_ENV_ALIGN;
  e->env_id_base = env_id_base;
  e->ep_bits = nullptr; e->ep_bits_n = 0; e->ep_seed = 0; e->rand_stream = nullptr; e->rand_n = 0; e->rand_seed = 0; e->acc_dev = nullptr; e->rng_set = 0; e->ftable_dev = nullptr; e->ftable_n = 0; e->graph_owner = GraphOwner{device, nullptr, 0}; e->lds_cap_raised = 0; e->arg_epoch = 0;

  KSpec& k = e->ks;
  memset(&k, 0, sizeof(k));
  k.family = spec->family; k.H = spec->H; k.W = spec->W; k.HW = HW; k.K = spec->K; k.M = spec->M;
  k.A = spec->A; k.max_iterations = spec->max_iterations; k.flags = spec->flags;
  if (spec->family == SGW_ISLAND_NAVIGATION_EX) k.flags = (k.flags & ~Island::F_PACKED) | (island_packable(*spec) ? Island::F_PACKED : 0);
  k.action_lo = spec->action_lo; k.n_actions = spec->n_actions; k.words = words;
  memcpy(k.start_cell, spec->start_cell, sizeof(k.start_cell));
  kspec_derive(k);
  kspec_views(k, *spec);
  if (spec->family == SGW_ISLAND_NAVIGATION_EX_MA) k.view_rotates = (spec->flags & (IslandMa::F_ODIR | IslandMa::F_ODIR_TURN)) ? 1 : 0;
  if (spec->family == SGW_AINTELOPE_SAVANNA) k.view_rotates = (spec->flags & (Savanna::F_ODIR | Savanna::F_ODIR_TURN)) ? 1 : 0;
  if (spec->family == SGW_FIREMAKER_EX_MA) k.view_rotates = (spec->flags & (Firemaker::F_ODIR | Firemaker::F_ODIR_TURN)) ? 1 : 0;
  memcpy(k.dim_slot, spec->dim_slot, sizeof(k.dim_slot));
  memcpy(k.metric_slot, spec->metric_slot, sizeof(k.metric_slot));
  // the one-step kernel with this spec's output geometry compiled in, if the library has one; SGW_GENERIC_STEP keeps the generic
  // kernel (the tests compare the two)
  e->step_shape = getenv("SGW_GENERIC_STEP") ? 0 : engine_step_shape(e);
  // ... and that kernel with the spec's whole rule set compiled in, when the shape's entry has one and the spec is exactly it;
  // SGW_GENERIC_RULES keeps the entry's own family
  e->step_rules = (e->step_shape > 0 && !getenv("SGW_GENERIC_RULES")) ? engine_step_rules(e) : 0;
  // ... as a pair of waves per env-wave when the launch is small enough for the second wave to find an idle issue slot;
  // SGW_NO_FORK keeps the one-wave kernel
  e->step_fork = (e->step_rules > 0 && !getenv("SGW_NO_FORK")) ? engine_step_fork(e) : 0;

  const size_t tbytes = TABLE_BYTES;
  uint8_t host_tables[TABLE_BYTES];
  memset(host_tables, 0, sizeof(host_tables));
  memcpy(host_tables, spec->static_board, HW);
  memcpy(host_tables + SGW_MAX_CELLS, spec->art, HW);
  memcpy(host_tables + 2 * SGW_MAX_CELLS, spec->aux, HW);
  memcpy(host_tables + 3 * SGW_MAX_CELLS, spec->value_map, 512);
  memcpy(host_tables + 3 * SGW_MAX_CELLS + 512, spec->params, SGW_N_PARAMS * 8);

  hipError_t err = hipMalloc((void**)&e->tables_dev, tbytes);
  if (err == hipSuccess) err = hipMemcpy(e->tables_dev, host_tables, tbytes, hipMemcpyHostToDevice);
  const size_t sbytes = (size_t)state_alloc_words(words, e->n_pad) * 8;      // pair layout (sgw_common.hpp): ceil(words / 2) KiB per env-wave
  if (err == hipSuccess) err = hipMalloc((void**)&e->state_dev, sbytes);
  // the episodic-return accumulators (sgw_read_returns): part of the engine from the start, zeroed here with the state --
  // sgw_create ends with a device synchronisation, so no stream of the caller can run ahead of the zeroing
  if (err == hipSuccess) err = hipMalloc((void**)&e->acc_dev, acc_bytes(e));
  if (err == hipSuccess) err = hipMemset(e->acc_dev, 0, acc_bytes(e));
  if (err != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "sgw_create: device allocation failed: %s", hipGetErrorString(err));
    if (e->tables_dev) (void)hipFree(e->tables_dev);
    if (e->state_dev) (void)hipFree(e->state_dev);
    if (e->acc_dev) (void)hipFree(e->acc_dev);
    delete e;
    return SGW_ERR_HIP;
  }
  *out_engine = e;
  // step_type ST_NONE (3) in every env's core word => the first sgw_step auto-resets
  hipLaunchKernelGGL(k_state_init, dim3((unsigned)((sbytes / 8 + 255) / 256)), dim3(256), 0, 0, e->state_dev, e->n_pad, words);
  err = hipGetLastError();
  if (err != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "sgw_create: state init failed: %s", hipGetErrorString(err));
    sgw_destroy(e); *out_engine = nullptr;
    return SGW_ERR_HIP;
  }
  // the state / table initialisation above went through the null stream: finished before the caller can launch on any
  // (possibly non-blocking) stream of its own
  err = hipStreamSynchronize(nullptr);
  if (err != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "sgw_create: initialisation did not complete: %s", hipGetErrorString(err));
    sgw_destroy(e); *out_engine = nullptr;
    return SGW_ERR_HIP;
  }
  return SGW_OK;
}

int sgw_destroy(sgw_engine* e) {
  if (!e) return SGW_OK;
  e->graphs.clear();
  e->full_graphs.clear();
  e->policy_graphs.clear();
  if (e->graph_owner.capture_stream) (void)hipStreamDestroy(e->graph_owner.capture_stream);
  if (e->tables_dev) (void)hipFree(e->tables_dev);
  if (e->state_dev) (void)hipFree(e->state_dev);
  if (e->acc_dev) (void)hipFree(e->acc_dev);
  if (e->ftable_dev) (void)hipFree(e->ftable_dev);
  delete e;
  return SGW_OK;
}

int64_t sgw_n_envs(const sgw_engine* e) { return e ? e->n_envs : 0; }
int64_t sgw_n_pad(const sgw_engine* e) { return e ? e->n_pad : 0; }
int sgw_state_words(const sgw_engine* e) { return e ? e->ks.words : 0; }
int sgw_step_shape(const sgw_engine* e) { return e ? e->step_shape : 0; }
int sgw_step_rules(const sgw_engine* e) { return e ? e->step_rules : 0; }
int sgw_step_fork(const sgw_engine* e) { return e ? e->step_fork : 0; }
int64_t sgw_state_bytes(const sgw_engine* e) { return e ? (int64_t)e->ks.words * e->n_pad * 8 : 0; }

int sgw_set_episode_bits(sgw_engine* e, const uint8_t* bits_dev, int n_per_env, uint64_t seed) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_set_episode_bits: null engine");
  if (bits_dev && n_per_env <= 0) return fail(SGW_ERR_ARG, "sgw_set_episode_bits: n_per_env must be positive");
  e->ep_bits = bits_dev; e->ep_bits_n = bits_dev ? n_per_env : 0; e->ep_seed = seed;
  drop_graphs(e);
  return SGW_OK;
}

int sgw_set_random_stream(sgw_engine* e, const double* u_dev, int n_per_env, uint64_t seed) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_set_random_stream: null engine");
  if (u_dev && n_per_env <= 0) return fail(SGW_ERR_ARG, "sgw_set_random_stream: n_per_env must be positive");
  e->rand_stream = u_dev; e->rand_n = u_dev ? n_per_env : 0; e->rand_seed = seed;
  drop_graphs(e);
  return SGW_OK;
}

int sgw_set_rng_state(sgw_engine* e, const uint64_t* pcg_state_dev) {
  if (!e || !pcg_state_dev) return fail(SGW_ERR_ARG, "sgw_set_rng_state: null argument");
  if (e->spec.family != SGW_FIREMAKER_EX_MA && e->spec.family != SGW_ISLAND_NAVIGATION_EX_MA &&
      e->spec.family != SGW_AINTELOPE_SAVANNA)
    return fail(SGW_ERR_UNSUPPORTED, "sgw_set_rng_state: this game family has no env-side RNG stream");
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_set_rng, dim3((unsigned)((e->n_pad + 255) / 256)), dim3(256), 0, 0, e->state_dev, e->n_pad,
                     e->n_envs, e->ks.words, pcg_state_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(0));
  e->rng_set = 1;
  return SGW_OK;
}

int sgw_seed_rng(sgw_engine* e, const uint64_t* seeds_dev, uint64_t seed_base, const uint32_t* layout_seeds_dev,
                 const uint8_t* mask_dev, int flags, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_seed_rng: null engine");
  if (flags & ~SEED_FLAGS_ALL) return fail(SGW_ERR_ARG, "sgw_seed_rng: unknown flag bits");
  if (e->spec.family != SGW_FIREMAKER_EX_MA && e->spec.family != SGW_ISLAND_NAVIGATION_EX_MA &&
      e->spec.family != SGW_AINTELOPE_SAVANNA)
    return fail(SGW_ERR_UNSUPPORTED, "sgw_seed_rng: this game family has no env-side RNG stream");
  if (mask_dev && !e->rng_set)
    return fail(SGW_ERR_ARG, "sgw_seed_rng: a masked call reseeds some envs of a seeded engine; seed every env first (mask_dev == NULL, "
                "sgw_set_rng_state or sgw_set_state)");
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_seed_rng, dim3((unsigned)((e->n_pad + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->state_dev, e->n_pad,
                     e->n_envs, e->ks.words, seeds_dev, seed_base + (uint64_t)e->env_id_base, layout_seeds_dev, mask_dev, flags);
  HIP_TRY(hipGetLastError());
  if (!mask_dev) e->rng_set = 1;
  return SGW_OK;
}

int sgw_pcg64_from_seeds(const uint64_t* seeds_dev, uint64_t seed_base, int64_t id_base, const uint32_t* layout_seeds_dev, int flags,
                         int64_t n, uint64_t* pcg_state_dev, int device, void* stream) {
  if (!pcg_state_dev || n < 0 || (flags & ~SEED_FLAGS_ALL))
    return fail(SGW_ERR_ARG, "sgw_pcg64_from_seeds: null output, negative n or unknown flag bits");
  if (n == 0) return SGW_OK;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_pcg64_from_seeds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seeds_dev,
                     seed_base + (uint64_t)id_base, layout_seeds_dev, flags, (long long)n, pcg_state_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_set_family_table(sgw_engine* e, const double* table_host, int64_t n) {
  if (!e || !table_host || n <= 0) return fail(SGW_ERR_ARG, "sgw_set_family_table: null / empty argument");
  const bool island_general = e->spec.family == SGW_ISLAND_NAVIGATION_EX && (e->spec.flags & Island::F_GENERAL);
  if (e->spec.family != SGW_AINTELOPE_SAVANNA && !island_general)
    return fail(SGW_ERR_UNSUPPORTED, "sgw_set_family_table: this game family / configuration has no lookup table");
  if (e->spec.family == SGW_AINTELOPE_SAVANNA && n != 2 * ((int64_t)e->spec.max_iterations + 2))
    return fail(SGW_ERR_ARG, "sgw_set_family_table: aintelope_savanna expects 2 * (max_iterations + 2) entries");
  if (island_general && n != 15 * 12 + 15)
    return fail(SGW_ERR_ARG, "sgw_set_family_table: island_navigation_ex per-event reward vectors are 15 x 12 values + 15 masks");
  HIP_TRY(hipSetDevice(e->device));
  drop_graphs(e);
  if (e->ftable_dev) { (void)hipFree(e->ftable_dev); e->ftable_dev = nullptr; e->ftable_n = 0; }
  HIP_TRY(hipMalloc((void**)&e->ftable_dev, (size_t)n * 8));
  HIP_TRY(hipMemcpy(e->ftable_dev, table_host, (size_t)n * 8, hipMemcpyHostToDevice));
  e->ftable_n = n;
  return SGW_OK;
}

#ifdef SGW_SAV_PROF     // diagnostic build only
extern "C" int sgw_debug_sav_prof(unsigned long long* out, int clear) {      // out[4096 * 16]
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sav_prof), 4096 * 16 * 8) != hipSuccess) return -1;
  if (clear) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_sav_prof)) != hipSuccess || hipMemset(p, 0, 4096 * 16 * 8) != hipSuccess) return -1; }
  return 0;
}
#endif
#ifdef SGW_PHASE_PROF   // diagnostic build only
extern "C" int sgw_debug_phase_prof(unsigned long long* out, int clear) {    // out[4096 * 8]
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_prof), 4096 * 8 * 8) != hipSuccess) return -1;
  if (clear) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_phase_prof)) != hipSuccess || hipMemset(p, 0, 4096 * 8 * 8) != hipSuccess) return -1; }
  return 0;
}
#endif
#ifdef SGW_FM_PROF      // diagnostic build only
extern "C" int sgw_debug_fm_prof(unsigned long long* out, int clear) {      // out[4096 * 16]
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fm_prof), 4096 * 16 * 8) != hipSuccess) return -1;
  if (clear) { void* p = nullptr; if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_fm_prof)) != hipSuccess || hipMemset(p, 0, 4096 * 16 * 8) != hipSuccess) return -1; }
  return 0;
}
#endif

int sgw_pow_f64(const double* x_dev, double y, double* out_dev, int64_t n, int device, void* stream) {
  if (!x_dev || !out_dev || n < 0) return fail(SGW_ERR_ARG, "sgw_pow_f64: null / negative argument");
  if (n == 0) return SGW_OK;
  HIP_TRY(hipSetDevice(device));
  hipLaunchKernelGGL(k_pow, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_dev, y, out_dev, (long long)n);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

}  // extern "C"

// ---- launch planning: the same validation and LDS / grid arithmetic for a family's own launch and for a group member ------
template <class F> struct FamilyType { using type = F; };
// fn(FamilyType<F>{}, tag) for the family (and state variant) this engine runs
template <class Fn> static int with_family(const sgw_engine* e, Fn&& fn) {
  switch (e->spec.family) {
    case SGW_ISLAND_NAVIGATION_EX:
      if (e->spec.flags & Island::F_GENERAL) return fn(FamilyType<IslandGeneral>{}, (int)TAG_ISLAND_GENERAL);
      if (e->ks.flags & Island::F_PACKED) return fn(FamilyType<IslandPacked>{}, (int)TAG_ISLAND_PACKED);
      return fn(FamilyType<Island>{}, (int)TAG_ISLAND);
    case SGW_BOAT_RACE_EX:
    case SGW_BOAT_RACE: return fn(FamilyType<Boat>{}, (int)TAG_BOAT);
    case SGW_SAFE_INTERRUPTIBILITY: return fn(FamilyType<SafeInt>{}, (int)TAG_SAFEINT);
    case SGW_FIREMAKER_EX_MA:
      if (e->spec.flags & Firemaker::F_WIDE) return fn(FamilyType<FiremakerWide>{}, (int)TAG_FIREMAKER);     // spread distance > 3
      return fn(FamilyType<Firemaker>{}, (int)TAG_FIREMAKER);
    case SGW_ISLAND_NAVIGATION_EX_MA:
      if (e->spec.H * e->spec.W > 64) return fn(FamilyType<IslandMaWide>{}, (int)TAG_ISLAND_MA);      // resized maps of 65..128 cells
      return fn(FamilyType<IslandMa>{}, (int)TAG_ISLAND_MA);
    case SGW_TILE_EVENTS: return fn(FamilyType<Tile>{}, (int)TAG_TILE);
    case SGW_SIDE_EFFECTS_SOKOBAN: return fn(FamilyType<Sokoban>{}, (int)TAG_SOKOBAN);
    case SGW_CONVEYOR_BELT: return fn(FamilyType<Conveyor>{}, (int)TAG_CONVEYOR);
    case SGW_TOMATO_WATERING: return fn(FamilyType<Tomato>{}, (int)TAG_TOMATO);
    case SGW_FRIEND_FOE: return fn(FamilyType<FriendFoe>{}, (int)TAG_FRIEND_FOE);
    case SGW_WHISKY_GOLD: return fn(FamilyType<Whisky>{}, (int)TAG_WHISKY);
    case SGW_ROCKS_DIAMONDS: return fn(FamilyType<Rocks>{}, (int)TAG_ROCKS);
    case SGW_AINTELOPE_SAVANNA: return fn(FamilyType<Savanna>{}, (int)TAG_SAVANNA);
    default: return fail(SGW_ERR_UNSUPPORTED, "launch: unknown game family");
  }
}

// The shaped one-step kernels (sgw_kernels.hpp StepShape): a family (state variant included) and the output geometry its kernel
// has compiled in.  An engine whose family and spec match an entry steps with that kernel; adding a shape is one line here.
// RF: a family type that differs from F in its rules only, compiled for one spec (RF::matches(sgw_spec) says which); an engine
// whose spec it accepts steps with k_engine<RF, K_STEP, SH> instead (e->step_rules).  void = the entry has none.
template <class F, class SH, class RF = void> struct ShapedStep { using Family = F; using Shape = SH; using Rules = RF; };
using ShapedSteps = std::tuple<
    // island_navigation_ex, level 9, default flags (the headline): 6 x 8 board, 10 reward columns, FINAL and DEATH not enabled;
    // the default parameters on top of that: the rules compiled in as well
    ShapedStep<IslandPacked, StepShape<6, 8, 10, 0, 1, 2, 3, -1, 4, 5, 6, 7, 8, 9, -1>, IslandL9Default>>;

// 1 + the index of the entry for family F and this spec, or 0
template <class F, size_t I = 0> static int find_step_shape(const KSpec& k) {
  if constexpr (I < std::tuple_size<ShapedSteps>::value) {
    using E = std::tuple_element_t<I, ShapedSteps>;
    if constexpr (std::is_same<typename E::Family, F>::value) { if (E::Shape::matches(k)) return (int)I + 1; }
    return find_step_shape<F, I + 1>(k);
  } else {
    return 0;
  }
}

static int engine_step_shape(const sgw_engine* e) {
  const int s = with_family(e, [&](auto ft, int) { using F = typename decltype(ft)::type; return find_step_shape<F>(e->ks); });
  return s > 0 ? s : 0;
}

// does the engine's shape entry have a compiled rule set that accepts this spec?
template <size_t I = 0> static int find_step_rules(const sgw_engine* e) {
  if constexpr (I < std::tuple_size<ShapedSteps>::value) {
    using E = std::tuple_element_t<I, ShapedSteps>;
    if constexpr (!std::is_void<typename E::Rules>::value) { if (e->step_shape == (int)I + 1) return E::Rules::matches(e->spec) ? 1 : 0; }
    return find_step_rules<I + 1>(e);
  } else {
    return 0;
  }
}
static int engine_step_rules(const sgw_engine* e) { return find_step_rules(e); }

// The forked step kernel (sgw_kernels.hpp k_step_fork) doubles the launch's wavefronts and reads the state twice: that pays
// while a SIMD holds at most one env-wave, so that the second wave takes issue slots nobody uses.  A larger launch is bound by
// HBM with many waves per SIMD already and keeps the one-wave kernel.  (DESIGN.md §4.1 has the sizes measured.)
static int engine_step_fork(const sgw_engine* e) {
#ifdef SGW_FORK_ANY_SIZE       // diagnostic build: the size sweep behind the rule below
  return 1;
#endif
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || cus <= 0) return 0;
  return e->n_pad / WAVE <= 4ll * cus ? 1 : 0;
}

static int launch_kind(const KArgs& a) {                      // K_STEP reads the caller's actions only
  return a.mode == MODE_RESET ? K_RESET : ((a.T == 1 && a.actions) ? K_STEP : K_ROLLOUT);
}

// what has to be true of the engine before any launch, and the engine's own fields of the arguments
static int prepare_args(sgw_engine* e, KArgs& a) {
  if (e->spec.family == SGW_FIREMAKER_EX_MA && !e->rng_set)
    return fail(SGW_ERR_ARG, "firemaker_ex_ma: call sgw_set_rng_state first (the env draws from a per-env numpy PCG64 stream)");
  if (e->spec.family == SGW_ISLAND_NAVIGATION_EX_MA && !e->rng_set &&
      (e->spec.flags & (IslandMa::F_SHUFFLE | (3 << IslandMa::F_MRF_SHIFT))))
    return fail(SGW_ERR_ARG, "island_navigation_ex_ma: call sgw_set_rng_state first (action-order shuffle / map randomisation "
                             "draw from a per-env numpy PCG64 stream)");
  if (e->spec.family == SGW_AINTELOPE_SAVANNA && (!e->rng_set || !e->ftable_dev))
    return fail(SGW_ERR_ARG, "aintelope_savanna: call sgw_set_rng_state and sgw_set_family_table first (per-env numpy PCG64 "
                             "stream; host-evaluated gold / silver visit rewards)");
  if (e->spec.family == SGW_ISLAND_NAVIGATION_EX && (e->spec.flags & Island::F_GENERAL) && !e->ftable_dev)
    return fail(SGW_ERR_ARG, "island_navigation_ex: spec.flags asks for per-event reward vectors; call sgw_set_family_table first");
  if (a.out.safety2 && e->spec.family != SGW_AINTELOPE_SAVANNA)
    return fail(SGW_ERR_UNSUPPORTED, "launch: the safety2 output exists for aintelope_savanna only");
  if ((a.out.obs_dir || a.out.act_dir) && e->spec.family != SGW_ISLAND_NAVIGATION_EX_MA && e->spec.family != SGW_AINTELOPE_SAVANNA &&
      e->spec.family != SGW_FIREMAKER_EX_MA)
    return fail(SGW_ERR_UNSUPPORTED, "launch: the obs_dir / act_dir outputs exist for the families whose agents carry directions "
                                     "(island_navigation_ex_ma, aintelope_savanna, firemaker_ex_ma)");
  a.sp = e->ks; a.tables = e->tables_dev; a.state = e->state_dev; a.ftable = e->ftable_dev;
  a.n_pad = e->n_pad; a.n_envs = e->n_envs; a.env_id_base = e->env_id_base;
  a.ep_bits = e->ep_bits; a.ep_bits_n = e->ep_bits_n; a.ep_seed = e->ep_seed;
  a.rand_stream = e->rand_stream; a.rand_n = e->rand_n; a.rand_seed = e->rand_seed;
  return SGW_OK;
}

// The caller's part of the arguments of T steps in one launch: from `actions` ([T, N, A]), or, without, from the in-kernel
// stream of (seed, step0).  accumulate: finished episodes' returns go to the engine's accumulators (allocated and zeroed by
// sgw_create: nothing is allocated on the step path).
static int step_args(sgw_engine* e, const int8_t* actions, int T, uint64_t seed, int64_t step0, int write_every, const sgw_out* out,
                     int accumulate, KArgs& a) {
  if (accumulate && !e->acc_dev) return fail(SGW_ERR_ARG, "the engine's return accumulators are missing");
  memset(&a, 0, sizeof(a));
  a.mode = MODE_STEP; a.actions = actions; a.T = T; a.seed = seed; a.step0 = step0;
  a.write_every = write_every; a.ep_acc = accumulate ? e->acc_dev : nullptr;
  if (out) a.out = *out;
  return SGW_OK;
}

// Envs per chunk of the in-launch windows that are larger than the board (sgw_common.hpp lds_view_chunk rounds it up to what the
// row size allows): VIEWS_CHUNK_DEFAULT, chosen by measurement.  A diagnostic build (-DSGW_VIEWS_CHUNK_KNOB, the
// sweep of tools/diag/views_inlaunch_probe.py) reads SGW_VIEWS_CHUNK = 8 / 16 / 32 / 64 from the environment instead.
static int views_chunk_envs() {
#ifdef SGW_VIEWS_CHUNK_KNOB
  const char* s = getenv("SGW_VIEWS_CHUNK");
  const int g = s ? atoi(s) : 0;
  if (g == 8 || g == 16 || g == 32 || g == 64) return g;
#endif
  return VIEWS_CHUNK_DEFAULT;
}
struct LaunchPlan { size_t lds_bytes; unsigned blocks, threads; };
// LDS plan + grid of k_engine<F, KIND> for these arguments (fills a.lp / a.need)
// (EW env-waves per workgroup with NB staging buffers each, `threads` threads: k_engine<F, KIND>'s, or k_step_fork's)
template <class F> static int plan_launch_as(const sgw_engine* e, KArgs& a, LaunchPlan& p, const int EW, const int NB, const unsigned threads) {
  const long long n_waves = e->n_pad / WAVE;
  const int need = lds_need(a, F::LDS_SCRATCH_M), pa = F::PER_AGENT ? F::NA : 1;
  if ((need & (LN_VIEWS | LN_OBSVIEWS)) && (!has_views<F>::value || a.sp.view_total <= 0))
    return fail(SGW_ERR_UNSUPPORTED, "launch: the views / obs_views outputs exist for the families with agent windows only");
  // one-wavefront families, a window larger than the board: the family's BigViews variant assembles them (launch() picks it)
  if ((need & (LN_VIEWS | LN_OBSVIEWS)) && F::WAVES == 1 && a.sp.view_prefill && !has_chunked_views<F>::value)
    return fail(SGW_ERR_UNSUPPORTED, "launch: a window larger than the board is not assembled by this launch path: use sgw_agent_views");
  // (rot90 is for square windows, as in sgw_agent_views: the landing offsets of a non-square one would leave its row of the chunk)
  if (has_chunked_views<F>::value && (need & (LN_VIEWS | LN_OBSVIEWS)) && a.sp.view_rotates)
    for (int ag = 0; ag < SGW_MAX_AGENTS; ++ag)
      if (a.sp.view_h[ag] != a.sp.view_w[ag])
        return fail(SGW_ERR_UNSUPPORTED, "launch: rotation by observation direction needs square windows");
  const int vb = a.sp.view_total > 0 ? a.sp.view_total : 0;
  // ... a chunk of the image at a time (views_chunked); every other launch stages the env-wave's whole image
  const int VG = (has_chunked_views<F>::value && (need & (LN_VIEWS | LN_OBSVIEWS))) ? lds_view_chunk(vb, views_chunk_envs()) : WAVE;
  const int CS = cum_stash_rows<F>(a.sp.A, a.sp.K);
  a.lp = lds_plan(a.sp.HW, a.sp.A, a.sp.K, a.sp.M, pa, need, vb, CS, VG); a.need = need;
  p.lds_bytes = lds_total_bytes(a.sp.HW, a.sp.A, a.sp.K, a.sp.M, pa, need, vb, F::LDS_EXTRA, EW, NB, CS, VG);
  p.blocks = (unsigned)((n_waves + EW - 1) / EW);
  p.threads = threads;
  // the bytes requested == the bytes the plan hands out (checked on every launch)
  if ((size_t)TABLE_BYTES + F::LDS_EXTRA + (size_t)EW * NB * a.lp.wave_bytes != p.lds_bytes || (F::LDS_EXTRA & 15) != 0 ||
      (a.lp.wave_bytes & 15) != 0 || (a.lp.st & 15) != 0)
    return fail(SGW_ERR_ARG, "launch: LDS footprint mismatch between the launcher and the kernel's plan");
  if (p.lds_bytes > 160 * 1024) return fail(SGW_ERR_UNSUPPORTED, "launch: the requested outputs need more than 160 KiB of LDS per workgroup");
  return SGW_OK;
}

template <class F, int KIND> static int plan_launch(const sgw_engine* e, KArgs& a, LaunchPlan& p) {
  return plan_launch_as<F>(e, a, p, env_waves<F, KIND>(), lds_buffers<F, KIND>(), (unsigned)wg_threads<F, KIND>());
}

template <class F, int KIND, class SH = NoShape, bool RULES = false> static int launch_as(sgw_engine* e, KArgs& a, hipStream_t st) {
  LaunchPlan p;
  int rc = plan_launch<F, KIND>(e, a, p);
  if (rc) return rc;
  // above the default dynamic-LDS cap: raised ONCE per engine and kernel, to the CU's 160 KiB -- a launch that needs it
  // is then never the first inside a stream capture (sgw_step_n)
  // (a kernel with compiled rules is another function than its entry's own: a bit of its own)
  constexpr unsigned bit = RULES ? 1u << 20 : 1u << (KIND + (SH::ON ? 3 : 0) + (has_chunked_views<F>::value ? 4 : 0));
  static_assert(!RULES || (KIND == K_STEP && SH::ON), "compiled rules exist for shaped one-step kernels only");
  if (p.lds_bytes > 65536 && !(e->lds_cap_raised & bit)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_engine<F, KIND, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    e->lds_cap_raised |= bit;
  }
  hipLaunchKernelGGL((k_engine<F, KIND, SH>), dim3(p.blocks), dim3(p.threads), p.lds_bytes, st, SGW_HOT_ARGS(a), a);
  return SGW_OK;
}

// one step by k_step_fork<RF, SH>: FORK_EW env-waves per workgroup, two wavefronts each
template <class RF, class SH> static int launch_fork(sgw_engine* e, KArgs& a, hipStream_t st) {
  LaunchPlan p;
  int rc = plan_launch_as<RF>(e, a, p, FORK_EW, 1, (unsigned)FORK_THREADS);
  if (rc) return rc;
  constexpr unsigned bit = 1u << 21;
  if (p.lds_bytes > 65536 && !(e->lds_cap_raised & bit)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_step_fork<RF, SH>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    e->lds_cap_raised |= bit;
  }
  hipLaunchKernelGGL((k_step_fork<RF, SH>), dim3(p.blocks), dim3(p.threads), p.lds_bytes, st, SGW_HOT_ARGS(a), a);
  return SGW_OK;
}

// one step: the engine's shaped kernel when it has one (e->step_shape), the generic one otherwise
template <class F, size_t I = 0> static int launch_step(sgw_engine* e, KArgs& a, hipStream_t st) {
  if constexpr (I < std::tuple_size<ShapedSteps>::value) {
    using E = std::tuple_element_t<I, ShapedSteps>;
    if constexpr (std::is_same<typename E::Family, F>::value) {
      if (e->step_shape == (int)I + 1) {
        if constexpr (!std::is_void<typename E::Rules>::value) {
          if (e->step_fork) return launch_fork<typename E::Rules, typename E::Shape>(e, a, st);
          if (e->step_rules) return launch_as<typename E::Rules, K_STEP, typename E::Shape, true>(e, a, st);
        }
        return launch_as<F, K_STEP, typename E::Shape>(e, a, st);
      }
    }
    return launch_step<F, I + 1>(e, a, st);
  } else {
    return launch_as<F, K_STEP>(e, a, st);
  }
}

template <class F> struct big_views_variant { using type = F; };
template <> struct big_views_variant<Savanna> { using type = SavannaBigViews; };
template <> struct big_views_variant<IslandMa> { using type = IslandMaBigViews; };
template <> struct big_views_variant<IslandMaWide> { using type = IslandMaWideBigViews; };

static int launch(sgw_engine* e, KArgs& a, hipStream_t st) {
  int rc = prepare_args(e, a);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  const int kind = launch_kind(a);
  // a spec with a window larger than the board that asks for the windows runs the family's BigViews variant
  const bool big = (a.out.views || a.out.obs_views) && e->ks.view_prefill;
  rc = with_family(e, [&](auto ft, int) {
    using F = typename decltype(ft)::type;
    using B = typename big_views_variant<F>::type;
    if constexpr (!std::is_same<B, F>::value) {
      if (big) {
        if (kind == K_STEP) return launch_as<B, K_STEP>(e, a, st);
        if (kind == K_ROLLOUT) return launch_as<B, K_ROLLOUT>(e, a, st);
        return launch_as<B, K_RESET>(e, a, st);
      }
    }
    if (kind == K_STEP) return launch_step<F>(e, a, st);
    if (kind == K_ROLLOUT) return launch_as<F, K_ROLLOUT>(e, a, st);
    return launch_as<F, K_RESET>(e, a, st);
  });
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

extern "C" {

int sgw_reset(sgw_engine* e, const uint8_t* mask_dev, const sgw_out* out, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_reset: null engine");
  KArgs a;
  (void)step_args(e, nullptr, 1, 0, 0, 0, out, 0, a);
  a.mode = MODE_RESET; a.mask = mask_dev;
  return launch(e, a, (hipStream_t)stream);
}

int64_t sgw_step_lds_bytes(sgw_engine* e, const sgw_out* out) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_step_lds_bytes: null engine");
  KArgs a;
  (void)step_args(e, nullptr, 1, 0, 0, 0, out, 0, a);
  a.sp = e->ks;
  const bool big = (a.out.views || a.out.obs_views) && e->ks.view_prefill;
  LaunchPlan p{};
  const int rc = with_family(e, [&](auto ft, int) {
    using F = typename decltype(ft)::type;
    using B = typename big_views_variant<F>::type;
    if constexpr (!std::is_same<B, F>::value) { if (big) return plan_launch<B, K_STEP>(e, a, p); }
    return plan_launch<F, K_STEP>(e, a, p);
  });
  return rc ? (int64_t)rc : (int64_t)p.lds_bytes;
}

int sgw_step(sgw_engine* e, const int8_t* actions_dev, const sgw_out* out, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_step: null engine");
  if (!actions_dev) return fail(SGW_ERR_ARG, "sgw_step: null actions");
  KArgs a;
  (void)step_args(e, actions_dev, 1, 0, 0, 0, out, 0, a);
  return launch(e, a, (hipStream_t)stream);
}

static int step_n_launches(sgw_engine* e, const int8_t* actions_dev, int T, int write_every, const sgw_out* out,
                           int accumulate, hipStream_t st) {
  for (int t = 0; t < T; ++t) {
    KArgs a;
    int rc = step_args(e, actions_dev + (long long)t * e->n_envs * e->spec.A, 1, 0, 0, 0, out, accumulate, a);
    if (rc) return rc;
    if (out && write_every) offset_out(a.out, e->spec, e->n_pad, t);
    rc = launch(e, a, st);
    if (rc) return rc;
  }
  return SGW_OK;
}

int sgw_step_n(sgw_engine* e, const int8_t* actions_dev, int T, int write_every, const sgw_out* out,
               int accumulate, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_step_n: null engine");
  if (!actions_dev || T < 1) return fail(SGW_ERR_ARG, "sgw_step_n: bad argument");
  const hipStream_t st = (hipStream_t)stream;
  auto launches = [&](hipStream_t s) { return step_n_launches(e, actions_dev, T, write_every, out, accumulate, s); };
  if (T < step_graphs_min_T()) return launches(st);
  GraphKey<1> key; memset(&key, 0, sizeof(key));
  key.actions[0] = actions_dev; key.epochs[0] = e->arg_epoch;
  key.n = 1; key.T = T; key.write_every = write_every != 0; key.accumulate = accumulate != 0; key.has_out = out != nullptr;
  if (out) key.outs[0] = *out;
  return e->graphs.run(e->graph_owner, key, T, launches, st, "sgw_step_n");
}

}  // extern "C"

// ---- groups: one heterogeneous launch over several engines (k_engine_group, sgw_group.hpp) -----------------------------------
struct sgw_group {
  std::vector<sgw_engine*> members;
  int device;
  unsigned lds_cap_raised;
  // sgw_group_step_n: at most 64 captures (a key records every member's arg_epoch: a member setter makes them stale)
  GraphOwner graph_owner;
  GraphCache<GROUP_MAX> graphs{64, 0, " of the step launches"};
};

static bool group_tag(int tag) {
  switch (tag) {
#define SGW_GROUP_TAG(TAG, F) case TAG: return true;
    SGW_GROUP_FAMILIES(SGW_GROUP_TAG)
#undef SGW_GROUP_TAG
    default: return false;
  }
}

// one launch of k_engine_group<KIND> over the members' prepared arguments (a[m].actions / out / T / seed ... set by the caller)
template <int KIND> static int group_launch(sgw_group* g, std::vector<KArgs>& a, hipStream_t st) {
  GroupArgs ga; memset(&ga, 0, sizeof(ga));
  ga.n = (int)g->members.size();
  size_t lds = 0; unsigned blocks = 0;
  for (size_t m = 0; m < g->members.size(); ++m) {
    sgw_engine* e = g->members[m];
    int rc = prepare_args(e, a[m]);
    if (rc) return rc;
    LaunchPlan p{};
    int tag_m = -1;
    rc = with_family(e, [&](auto ft, int tag) {
      using F = typename decltype(ft)::type;
      tag_m = tag;
      if constexpr (group_member<F, K_STEP>() && group_member<F, K_ROLLOUT>()) return plan_launch<F, KIND>(e, a[m], p);
      else return fail(SGW_ERR_UNSUPPORTED, "group launch: this env family is not a group member (its round kernel has its own workgroup shape)");
    });
    if (rc) return rc;
    if (!group_tag(tag_m)) return fail(SGW_ERR_UNSUPPORTED, "group launch: this env family / configuration is not a group member");
    ga.first_block[m] = (int)blocks; ga.tag[m] = tag_m; ga.a[m] = a[m];
    blocks += p.blocks;
    lds = p.lds_bytes > lds ? p.lds_bytes : lds;
  }
  for (size_t m = g->members.size(); m <= GROUP_MAX; ++m) ga.first_block[m] = (int)blocks;
  if (lds > 65536 && !(g->lds_cap_raised & (1u << KIND))) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_engine_group<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    g->lds_cap_raised |= 1u << KIND;
  }
  GroupHot h{ga.n, ga.first_block[1], ga.first_block[2], ga.first_block[3],
             ga.tag[0] | (ga.tag[1] << 8) | (ga.tag[2] << 16) | (ga.tag[3] << 24)};
  hipLaunchKernelGGL((k_engine_group<KIND>), dim3(blocks), dim3(GROUP_THREADS), lds, st, SGW_GROUP_HOT_ARGS(h), ga);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

static int group_step_launches(sgw_group* g, const int8_t* const* actions, int T, int write_every, const sgw_out* outs, int accumulate,
                               hipStream_t st) {
  const size_t n = g->members.size();
  std::vector<KArgs> a(n);
  for (int t = 0; t < T; ++t) {
    for (size_t m = 0; m < n; ++m) {
      sgw_engine* e = g->members[m];
      int rc = step_args(e, actions[m] + (long long)t * e->n_envs * e->spec.A, 1, 0, 0, 0, outs ? &outs[m] : nullptr, accumulate, a[m]);
      if (rc) return rc;
      if (outs && write_every) offset_out(a[m].out, e->spec, e->n_pad, t);
    }
    int rc = group_launch<K_STEP>(g, a, st);
    if (rc) return rc;
  }
  return SGW_OK;
}

extern "C" {

int sgw_group_create(sgw_engine* const* engines, int n, sgw_group** out_group) {
  if (!engines || !out_group || n < 1 || n > GROUP_MAX) return fail(SGW_ERR_ARG, "sgw_group_create: 1 to 4 engines");
  *out_group = nullptr;
  for (int m = 0; m < n; ++m) {
    if (!engines[m]) return fail(SGW_ERR_ARG, "sgw_group_create: null engine");
    if (engines[m]->device != engines[0]->device) return fail(SGW_ERR_ARG, "sgw_group_create: the engines of a group live on one device");
    for (int k = 0; k < m; ++k) if (engines[k] == engines[m]) return fail(SGW_ERR_ARG, "sgw_group_create: an engine is listed twice");
    int tag_m = -1;
    (void)with_family(engines[m], [&](auto, int tag) { tag_m = tag; return 0; });
    if (!group_tag(tag_m)) return fail(SGW_ERR_UNSUPPORTED, "sgw_group_create: this env family / configuration is not a group member");
  }
  sgw_group* g = new (std::nothrow) sgw_group();
  if (!g) return fail(SGW_ERR_NOMEM, "sgw_group_create: out of host memory");
  g->members.assign(engines, engines + n);
  g->device = engines[0]->device; g->lds_cap_raised = 0; g->graph_owner = GraphOwner{g->device, nullptr, 0};
  *out_group = g;
  return SGW_OK;
}

int sgw_group_destroy(sgw_group* g) {
  if (!g) return SGW_OK;
  g->graphs.clear();
  if (g->graph_owner.capture_stream) (void)hipStreamDestroy(g->graph_owner.capture_stream);
  delete g;
  return SGW_OK;
}

int sgw_group_step_n(sgw_group* g, const int8_t* const* actions_dev, int T, int write_every, const sgw_out* outs, int accumulate,
                     void* stream) {
  if (!g || !actions_dev || T < 1) return fail(SGW_ERR_ARG, "sgw_group_step_n: bad argument");
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = g->members.size();
  for (size_t m = 0; m < n; ++m) if (!actions_dev[m]) return fail(SGW_ERR_ARG, "sgw_group_step_n: null actions");
  HIP_TRY(hipSetDevice(g->device));
  auto launches = [&](hipStream_t s) { return group_step_launches(g, actions_dev, T, write_every, outs, accumulate, s); };
  if (T < step_graphs_min_T()) return launches(st);
  GraphKey<GROUP_MAX> key; memset(&key, 0, sizeof(key));
  for (size_t m = 0; m < n; ++m) {
    key.actions[m] = actions_dev[m]; key.epochs[m] = g->members[m]->arg_epoch;
    if (outs) key.outs[m] = outs[m];
  }
  key.n = (int)n; key.T = T; key.write_every = write_every != 0; key.accumulate = accumulate != 0; key.has_out = outs != nullptr;
  return g->graphs.run(g->graph_owner, key, T, launches, st, "sgw_group_step_n");
}

int sgw_group_rollout(sgw_group* g, int T, uint64_t seed, int64_t step0, int write_every, const sgw_out* outs, int accumulate,
                      void* stream) {
  if (!g || T < 1) return fail(SGW_ERR_ARG, "sgw_group_rollout: bad argument");
  const hipStream_t st = (hipStream_t)stream;
  const size_t n = g->members.size();
  std::vector<KArgs> a(n);
  for (size_t m = 0; m < n; ++m) {
    sgw_engine* e = g->members[m];
    if (e->spec.n_actions < 1) return fail(SGW_ERR_ARG, "sgw_group_rollout: spec has no action range");
    int rc = step_args(e, nullptr, T, seed, step0, write_every, outs ? &outs[m] : nullptr, accumulate, a[m]);
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(g->device));
  return group_launch<K_ROLLOUT>(g, a, st);
}

int sgw_read_returns(sgw_engine* e, double* out_dev, int clear, void* stream) {
  if (!e || !out_dev) return fail(SGW_ERR_ARG, "sgw_read_returns: null argument");
  hipLaunchKernelGGL(k_read_returns, dim3(e->spec.A * e->spec.K + 1), dim3(256), 0, (hipStream_t)stream, e->acc_dev,
                     e->n_pad / WAVE * SGW_ACC_PARTS, e->spec.A * e->spec.K + 1, out_dev, clear);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_rollout(sgw_engine* e, int T, uint64_t seed, int64_t step0, int write_every, const sgw_out* out,
                int accumulate, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_rollout: null engine");
  if (T < 1) return fail(SGW_ERR_ARG, "sgw_rollout: T must be >= 1");
  if (e->spec.n_actions < 1) return fail(SGW_ERR_ARG, "sgw_rollout: spec has no action range");
  KArgs a;
  int rc = step_args(e, nullptr, T, seed, step0, write_every, out, accumulate, a);
  return rc ? rc : launch(e, a, (hipStream_t)stream);
}

int sgw_replay(sgw_engine* e, const int8_t* actions_dev, int T, int write_every, const sgw_out* out, int accumulate, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_replay: null engine");
  if (!actions_dev || T < 1) return fail(SGW_ERR_ARG, "sgw_replay: bad argument");
  KArgs a;
  int rc = step_args(e, actions_dev, T, 0, 0, write_every, out, accumulate, a);
  return rc ? rc : launch(e, a, (hipStream_t)stream);
}

constexpr int FILL_ACTIONS_MAX_BLOCKS = 4096;      // k_fill_actions strides over the rest
int sgw_fill_actions(sgw_engine* e, int T, uint64_t seed, int64_t step0, int8_t* actions_dev, void* stream) {
  if (!e || !actions_dev || T < 1) return fail(SGW_ERR_ARG, "sgw_fill_actions: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  long long total = (long long)T * e->n_envs * e->spec.A;
  int blocks = (int)((total + 255) / 256 < FILL_ACTIONS_MAX_BLOCKS ? (total + 255) / 256 : FILL_ACTIONS_MAX_BLOCKS);
  hipLaunchKernelGGL(k_fill_actions, dim3(blocks), dim3(256), 0, (hipStream_t)stream, actions_dev, e->n_envs,
                     e->spec.A, T, seed, step0, e->env_id_base, e->spec.action_lo, e->spec.n_actions);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_accumulate_returns(sgw_engine* e, const double* cumulative_dev, const uint8_t* step_type_dev,
                           double* ep_accum_dev, void* stream) {
  if (!e || !cumulative_dev || !step_type_dev || !ep_accum_dev)
    return fail(SGW_ERR_ARG, "sgw_accumulate_returns: null argument");
  HIP_TRY(hipSetDevice(e->device));
  int blocks = (int)((e->n_envs + 255) / 256);
  hipLaunchKernelGGL(k_accumulate_returns, dim3(blocks), dim3(256), 0, (hipStream_t)stream, cumulative_dev,
                     step_type_dev, e->n_envs, e->spec.A * e->spec.K, ep_accum_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

// ceil(2^32 / x) for div_recip (sgw_common.hpp): exact for every f <= f_max, or refused by the caller.  Each reciprocal is
// checked over the quotients its users take: a block's cell index / HW (< PLANES_ENVS * HW) and a block's 4-cell item / Q
// (< PLANES_ENVS * Q).  (The bound used to be the block's P * HW output bytes, for a per-byte expansion no kernel calls: it
// refused e.g. 32 layers of a 17 x 17 board.)
static bool plane_geom(int HW, int P, PlaneGeom& g) {
  auto recip = [](uint64_t x, uint64_t f_max, uint32_t& out) {
    if (x <= 1) { out = 0; return true; }
    const uint64_t r = ((1ull << 32) + x - 1) / x, err = r * x - (1ull << 32);
    out = (uint32_t)r;
    return f_max * err < (1ull << 32);
  };
  g.HW = HW; g.P = P;
  const uint64_t Q = (uint64_t)(HW + 3) / 4;
  uint32_t b = 0, c = 0;
  const bool ok = recip((uint64_t)HW, (uint64_t)PLANES_ENVS * HW, b) && recip(Q, (uint64_t)PLANES_ENVS * Q, c);
  g.recip_HW = (int)b; g.recip_Q = (int)c;
  return ok;
}
static int raise_lds_cap(sgw_engine* e, const void* fn, size_t lds, unsigned bit) {
  if (lds > 160 * 1024) return fail(SGW_ERR_UNSUPPORTED, "observe: the board is too large for the plane kernels' LDS staging");
  if (lds > 65536 && !(e->lds_cap_raised & bit)) {
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    e->lds_cap_raised |= bit;
  }
  return SGW_OK;
}

int sgw_observe(sgw_engine* e, const uint8_t* board_dev, const uint8_t* rgb_lut_dev, uint8_t* rgb_dev,
                const uint8_t* layer_chars_dev, int n_layers, uint8_t* layers_dev, void* stream) {
  if (!e || !board_dev) return fail(SGW_ERR_ARG, "sgw_observe: null argument");
  if (rgb_dev && !rgb_lut_dev) return fail(SGW_ERR_ARG, "sgw_observe: rgb requested without a LUT");
  if (layers_dev && (!layer_chars_dev || n_layers < 1 || n_layers > 128)) return fail(SGW_ERR_ARG, "sgw_observe: bad layer list");
  if (!rgb_dev && !layers_dev) return SGW_OK;
  HIP_TRY(hipSetDevice(e->device));
  PlaneGeom g_rgb, g_lay;
  if (!plane_geom(e->ks.HW, 3, g_rgb) || !plane_geom(e->ks.HW, layers_dev ? n_layers : 1, g_lay))
    return fail(SGW_ERR_UNSUPPORTED, "sgw_observe: board / layer count outside the plane kernels' index arithmetic");
  const int epb = PLANES_ENVS;
  const size_t lds = (((size_t)epb * e->ks.HW + 15) & ~(size_t)15) + 3 * 128;
  int rc = raise_lds_cap(e, reinterpret_cast<const void*>(&k_observe), lds, 16u);
  if (rc) return rc;
  const unsigned blocks = (unsigned)((e->n_envs + epb - 1) / epb);
  hipLaunchKernelGGL(k_observe, dim3(blocks), dim3(PLANES_THREADS), lds, (hipStream_t)stream, board_dev, (long long)e->n_envs, epb, g_rgb,
                     rgb_lut_dev, rgb_dev, g_lay, layer_chars_dev, layers_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_derived_stats(sgw_engine* e, const double* reward_dev, const double* cumulative_dev, const int32_t* frame_dev,
                      const int32_t* k_agent, double* stats_dev, void* stream) {
  if (!e || !reward_dev || !cumulative_dev || !frame_dev || !k_agent || !stats_dev)
    return fail(SGW_ERR_ARG, "sgw_derived_stats: null argument");
  if (((uintptr_t)reward_dev | (uintptr_t)cumulative_dev | (uintptr_t)stats_dev) & 15)
    return fail(SGW_ERR_ARG, "sgw_derived_stats: reward / cumulative / stats must be 16-byte aligned (rows move as 16-byte accesses)");
  AgentK ak; memset(&ak, 0, sizeof(ak));
  for (int a = 0; a < e->spec.A; ++a) {
    if (k_agent[a] < 0 || k_agent[a] > e->spec.K) return fail(SGW_ERR_ARG, "sgw_derived_stats: k_agent out of range");
    ak.k[a] = k_agent[a];
  }
  HIP_TRY(hipSetDevice(e->device));
  const int A = e->spec.A, K = e->spec.K;
  const size_t lds = (size_t)(2 * A * K + A * (5 + K)) * WAVE * 8;           // R | C | O (sgw_observe.hpp k_derived_stats)
  if (lds > 65536 && !(e->lds_cap_raised & 8u)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_derived_stats), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    e->lds_cap_raised |= 8u;
  }
  hipLaunchKernelGGL(k_derived_stats, dim3((unsigned)((e->n_envs + WAVE - 1) / WAVE)), dim3(WAVE), lds, (hipStream_t)stream, reward_dev,
                     cumulative_dev, frame_dev, e->n_envs, A, K, ak, ((1 << 18) + A * K - 1) / (A * K), stats_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_observe_layers(sgw_engine* e, const uint8_t* board_dev, const uint8_t* layer_chars_dev,
                       const uint8_t* layer_static_dev, int n_layers, int gap_index, const uint8_t* agent_pos_dev,
                       const uint8_t* agent_flags_dev, int hidden_layer, uint8_t* layers_dev, void* stream) {
  if ((agent_pos_dev == nullptr) != (agent_flags_dev == nullptr) || hidden_layer >= n_layers)
    return fail(SGW_ERR_ARG, "sgw_observe_layers: agent_pos/agent_flags/hidden_layer mismatch");
  if (!e || !board_dev || !layer_chars_dev || !layer_static_dev || !layers_dev || n_layers < 1 || gap_index >= n_layers)
    return fail(SGW_ERR_ARG, "sgw_observe_layers: bad argument");
  if (n_layers > 32) return fail(SGW_ERR_UNSUPPORTED, "sgw_observe_layers: at most 32 layers (a cell's layers are one 32-bit mask)");
  HIP_TRY(hipSetDevice(e->device));
  PlaneGeom g;
  if (!plane_geom(e->ks.HW, n_layers, g))
    return fail(SGW_ERR_UNSUPPORTED, "sgw_observe_layers: board / layer count outside the plane kernels' index arithmetic");
  const size_t HW = (size_t)e->ks.HW;
  // 64 envs per workgroup, 16 when their boards + masks would take more than a quarter of the CU's LDS (firemaker's 17 x 17: 95 KB
  // for 64 envs = one workgroup per CU and a serial chain of barriers; 24 KB for 16)
  const int epb = (5 * PLANES_ENVS * HW > 40 * 1024) ? 16 : PLANES_ENVS;
  const size_t lds = ((epb * HW + 15) & ~(size_t)15) + epb * HW * 4 + HW * 8 + 512;   // boards | masks | dyn, on | per-char
  int rc = raise_lds_cap(e, reinterpret_cast<const void*>(&k_observe_layers), lds, 32u);
  if (rc) return rc;
  const unsigned blocks = (unsigned)((e->n_envs + epb - 1) / epb);
  hipLaunchKernelGGL(k_observe_layers, dim3(blocks), dim3(PLANES_THREADS), lds, (hipStream_t)stream, board_dev, (long long)e->n_envs, epb, g,
                     e->ks.W, layer_chars_dev, layer_static_dev, gap_index, agent_pos_dev, agent_flags_dev, e->spec.A,
                     agent_pos_dev ? hidden_layer : -1, layers_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_state_layers(sgw_engine* e, const uint8_t* layer_chars_dev, int n_layers, int gap_only_blank, uint8_t* layers_dev,
                     void* stream) {
  if (!e || !layer_chars_dev || !layers_dev || n_layers < 1) return fail(SGW_ERR_ARG, "sgw_state_layers: bad argument");
  if (e->spec.family != SGW_AINTELOPE_SAVANNA)
    return fail(SGW_ERR_UNSUPPORTED, "sgw_state_layers: this family's layers follow from its board (sgw_observe_layers)");
  if (n_layers > 32) return fail(SGW_ERR_UNSUPPORTED, "sgw_state_layers: at most 32 layers");
  HIP_TRY(hipSetDevice(e->device));
  PlaneGeom g;
  if (!plane_geom(e->ks.HW, n_layers, g)) return fail(SGW_ERR_UNSUPPORTED, "sgw_state_layers: board / layer count outside the plane kernels' index arithmetic");
  const int epb = 16;                                             // 16 envs: 3.5 KB of state words + 10.6 KB of code vectors per workgroup
  const size_t lds = (size_t)epb * SAV_LAYER_WORDS * 8 + (size_t)epb * e->ks.HW * 4 + 32 * 4;
  hipLaunchKernelGGL(k_savanna_layers, dim3((unsigned)((e->n_envs + epb - 1) / epb)), dim3(PLANES_THREADS), lds, (hipStream_t)stream, e->state_dev,
                     e->n_pad, (long long)e->n_envs, e->ks.words, g, e->ks.W, (e->spec.flags & Savanna::F_TWO) ? 1 : 0, layer_chars_dev, gap_only_blank,
                     epb, layers_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

static ViewSpec make_viewspec(const sgw_engine* e) {
  ViewSpec v; memset(&v, 0, sizeof(v));
  v.A = e->spec.A; v.H = e->spec.H; v.W = e->spec.W;
  int off = 0;
  for (int a = 0; a < e->spec.A; ++a) {
    const int32_t* rad = e->spec.view_radius[a];
    if (rad[0] < 0) { v.off[a] = off; continue; }
    v.off[a] = off; v.up[a] = rad[0]; v.left[a] = rad[2];
    v.vh[a] = rad[0] + rad[1] + 1; v.vw[a] = rad[2] + rad[3] + 1;
    off += v.vh[a] * v.vw[a];
  }
  v.total = off;
  return v;
}

int sgw_view_bytes(const sgw_engine* e) { return e ? make_viewspec(e).total : 0; }

// LDS stage of one wave of the window kernels: the largest window + one 16-byte phase, rounded to 16
static int view_stage_bytes(const ViewSpec& v) {
  int mx = 0;
  for (int a = 0; a < v.A; ++a) mx = v.vh[a] * v.vw[a] > mx ? v.vh[a] * v.vw[a] : mx;
  return (mx + 16 + 15) / 16 * 16;
}

static bool views_all_small(const ViewSpec& v) {
  for (int a = 0; a < v.A; ++a) if (v.vh[a] * v.vw[a] > WAVE) return false;
  return true;
}

static int check_rotation(const sgw_engine* e, const ViewSpec& v, const uint8_t* flags) {
  if (!flags) return SGW_OK;
  for (int a = 0; a < v.A; ++a)
    if (v.vh[a] != v.vw[a]) return fail(SGW_ERR_UNSUPPORTED, "agent views: rotation by observation direction needs square windows");
  (void)e;
  return SGW_OK;
}

// grid caps of the window launches: every kernel below walks what is left in a stride loop (tests/grid_caps.py has a row for each)
constexpr int AGENT_VIEWS_SMALL_MAX_BLOCKS = 65536, AGENT_LAYER_VIEWS_SMALL_MAX_BLOCKS = 65536;      // one thread per output byte
constexpr int AGENT_VIEWS_LDS_MAX_BLOCKS = 8192, AGENT_VIEWS_LDS_GROUP_ENVS = 4;                     // one-wave workgroups, GROUP_ENVS envs per pass
constexpr int AGENT_LAYER_VIEWS_LDS_MAX_BLOCKS = 4096;                                               // a workgroup per env
constexpr int AGENT_VIEWS_WAVE_MAX_BLOCKS = 65536, AGENT_LAYER_VIEWS_WAVE_MAX_BLOCKS = 65536;        // four waves, a wave per window

int sgw_agent_views(sgw_engine* e, const uint8_t* board_dev, const uint8_t* agent_pos_dev, const uint8_t* agent_flags_dev,
                    uint8_t outside_chr, uint8_t* views_dev, void* stream) {
  if (!e || !board_dev || !agent_pos_dev || !views_dev) return fail(SGW_ERR_ARG, "sgw_agent_views: null argument");
  ViewSpec v = make_viewspec(e);
  if (v.total <= 0) return fail(SGW_ERR_UNSUPPORTED, "sgw_agent_views: the spec defines no agent views");
  if (check_rotation(e, v, agent_flags_dev)) return SGW_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(e->device));
  if (views_all_small(v)) {                                              // every window <= 64 cells: one thread per byte
    long long total = e->n_envs * (long long)v.total;
    int blocks = (int)((total + 255) / 256 < AGENT_VIEWS_SMALL_MAX_BLOCKS ? (total + 255) / 256 : AGENT_VIEWS_SMALL_MAX_BLOCKS);
    hipLaunchKernelGGL(k_agent_views_small, dim3(blocks), dim3(256), 0, (hipStream_t)stream, board_dev, agent_pos_dev,
                       agent_flags_dev, e->n_envs, v, outside_chr, views_dev);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
  }
  {
    // one wave per env: the board and the env's row of windows in LDS, the row out as dword stores at its byte address (the layer-cube
    // kernel with one plane; round 2's k_agent_views -- a wave per window, cells loaded from global memory -- took 26 us for 16 384 envs)
    const int lay_bytes = (e->ks.HW + 15) / 16 * 16, img_bytes = (v.total + 15) / 16 * 16 + 16;      // (+ 16: the image sits at its row's 16-byte phase)
    constexpr int G = AGENT_VIEWS_LDS_GROUP_ENVS;      // envs a one-wave workgroup takes per pass (k_agent_layer_views_lds; 16 384 envs: G = 2 18.9, G = 4 17.8, G = 8 24.8 us)
    const size_t lds = 128 + 16 * G + (size_t)G * ((size_t)lay_bytes + (size_t)img_bytes);       // table | per-env words | G x (planes | image)
    if (lds <= 64 * 1024) {
      const long long groups = (e->n_envs + G - 1) / G;
      const int blocks = (int)(groups < AGENT_VIEWS_LDS_MAX_BLOCKS ? groups : AGENT_VIEWS_LDS_MAX_BLOCKS);           // (each walks its groups; 4 096..16 384 workgroups measured the same, fewer are slower)
      hipLaunchKernelGGL(k_agent_layer_views_lds<G>, dim3(blocks), dim3(WAVE), lds, (hipStream_t)stream, board_dev, agent_pos_dev, agent_flags_dev,
                         (long long)e->n_envs, v, (const uint8_t*)nullptr, 1, outside_chr, views_dev, lay_bytes, img_bytes, 1);
      HIP_TRY(hipGetLastError());
      return SGW_OK;
    }
  }
  long long total = e->n_envs * (long long)v.A * WAVE;                   // one wave per (env, agent) window
  int blocks = (int)((total + 255) / 256 < AGENT_VIEWS_WAVE_MAX_BLOCKS ? (total + 255) / 256 : AGENT_VIEWS_WAVE_MAX_BLOCKS);
  const int lds_per_wave = view_stage_bytes(v);
  hipLaunchKernelGGL(k_agent_views, dim3(blocks), dim3(256), 4 * lds_per_wave, (hipStream_t)stream, board_dev, agent_pos_dev,
                     agent_flags_dev, e->n_envs, v, outside_chr, views_dev, lds_per_wave);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_agent_layer_views(sgw_engine* e, const uint8_t* layers_dev, const uint8_t* agent_pos_dev, const uint8_t* agent_flags_dev,
                          const uint8_t* layer_chars_dev, int n_layers, uint8_t outside_chr, uint8_t* out_dev, void* stream) {
  if (!e || !layers_dev || !agent_pos_dev || !layer_chars_dev || !out_dev || n_layers < 1)
    return fail(SGW_ERR_ARG, "sgw_agent_layer_views: bad argument");
  ViewSpec v = make_viewspec(e);
  if (v.total <= 0) return fail(SGW_ERR_UNSUPPORTED, "sgw_agent_layer_views: the spec defines no agent views");
  if (check_rotation(e, v, agent_flags_dev)) return SGW_ERR_UNSUPPORTED;
  HIP_TRY(hipSetDevice(e->device));
  if (views_all_small(v)) {
    long long total = e->n_envs * (long long)v.total * n_layers;
    int blocks = (int)((total + 255) / 256 < AGENT_LAYER_VIEWS_SMALL_MAX_BLOCKS ? (total + 255) / 256 : AGENT_LAYER_VIEWS_SMALL_MAX_BLOCKS);
    hipLaunchKernelGGL(k_agent_layer_views_small, dim3(blocks), dim3(256), 0, (hipStream_t)stream, layers_dev, agent_pos_dev,
                       agent_flags_dev, e->n_envs, v, layer_chars_dev, n_layers, outside_chr, out_dev);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
  }
  // a workgroup per env: the env's layer planes and its whole output row in LDS (k_agent_layer_views_lds)
  const int lay_bytes = (n_layers * e->ks.HW + 15) / 16 * 16, img_bytes = (v.total * n_layers + 15) / 16 * 16 + 16;
  const size_t lds = 128 + 16 + (size_t)lay_bytes + (size_t)img_bytes;
  if (lds <= 64 * 1024) {
    const int blocks = (int)(e->n_envs < AGENT_LAYER_VIEWS_LDS_MAX_BLOCKS ? e->n_envs : AGENT_LAYER_VIEWS_LDS_MAX_BLOCKS);
    hipLaunchKernelGGL(k_agent_layer_views_lds<1>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, layers_dev, agent_pos_dev, agent_flags_dev,
                       (long long)e->n_envs, v, layer_chars_dev, n_layers, outside_chr, out_dev, lay_bytes, img_bytes, 0);
    HIP_TRY(hipGetLastError());
    return SGW_OK;
  }
  long long total = e->n_envs * (long long)v.A * n_layers * WAVE;        // (rows too large for LDS) one wave per (env, agent, layer) window
  int blocks = (int)((total + 255) / 256 < AGENT_LAYER_VIEWS_WAVE_MAX_BLOCKS ? (total + 255) / 256 : AGENT_LAYER_VIEWS_WAVE_MAX_BLOCKS);
  const int lds_per_wave = view_stage_bytes(v);
  hipLaunchKernelGGL(k_agent_layer_views, dim3(blocks), dim3(256), 4 * lds_per_wave, (hipStream_t)stream, layers_dev, agent_pos_dev,
                     agent_flags_dev, e->n_envs, v, layer_chars_dev, n_layers, outside_chr, out_dev, lds_per_wave);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

// sgw_layer_coords / sgw_agent_layer_coords: the lane split and the reciprocals of k_plane_coords (sgw_coords.hpp) for planes of at most
// max_cells cells, and the launch.  Plain launches on the caller's stream: nothing is allocated, nothing of the engine changes.
constexpr int PLANE_COORDS_MAX_BLOCKS = 8192;      // 4 waves per workgroup; each wave walks its planes
static int coords_launch(sgw_engine* e, bool rel, const uint8_t* planes, long long items, CoordGeom& g, int max_cells, int32_t* counts,
                         int16_t* coords, void* stream, const char* who) {
  if (((uintptr_t)counts | (uintptr_t)coords) & 3) return fail(SGW_ERR_ARG, "%s: counts and coords must be 4-byte aligned (a coordinate pair is one store)", who);
  if (items > 0x7fffffffLL) return fail(SGW_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 planes", who);
  for (int a = 0; a < g.A; ++a) {
    if (g.cells[a] > 32767) return fail(SGW_ERR_UNSUPPORTED, "%s: a plane has more cells than an int16 coordinate holds", who);
    const uint32_t w = (uint32_t)(g.W[a] > 0 ? g.W[a] : 1);
    g.recip_W[a] = w == 1 ? 0 : (int)(uint32_t)(((1ull << 32) + w - 1) / w);      // exact for every cell index: cells * W < 2^32
  }
  const int need = (max_cells + 3 + 3) / 4;             // dwords a plane touches at the worst alignment
  g.seg_shift = 0;
  while ((1 << g.seg_shift) < need && g.seg_shift < 6) ++g.seg_shift;
  g.n_pass = (need + (1 << g.seg_shift) - 1) >> g.seg_shift;
  if (items <= 0 || max_cells <= 0) return SGW_OK;
  HIP_TRY(hipSetDevice(e->device));
  const long long per_wave = WAVE >> g.seg_shift, waves = (items + per_wave - 1) / per_wave;
  const unsigned blocks = (unsigned)((waves + 3) / 4 < PLANE_COORDS_MAX_BLOCKS ? (waves + 3) / 4 : PLANE_COORDS_MAX_BLOCKS);
  if (rel) hipLaunchKernelGGL(k_plane_coords<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, planes, (unsigned)items, g, counts, coords);
  else hipLaunchKernelGGL(k_plane_coords<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, planes, (unsigned)items, g, counts, coords);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_layer_coords(sgw_engine* e, const uint8_t* layers_dev, int n_layers, int cap, int32_t* counts_dev, int16_t* coords_dev,
                     void* stream) {
  if (!e || !layers_dev || !counts_dev || !coords_dev || n_layers < 1 || n_layers > 32 || cap < 1)
    return fail(SGW_ERR_ARG, "sgw_layer_coords: bad argument (pointers, n_layers in 1..32, cap >= 1)");
  CoordGeom g; memset(&g, 0, sizeof(g));
  g.L = n_layers; g.A = 1; g.cap = cap;
  g.cells[0] = e->ks.HW; g.W[0] = e->ks.W; g.own[0] = -1;
  g.row_bytes = (long long)n_layers * e->ks.HW;
  return coords_launch(e, false, layers_dev, e->n_envs * n_layers, g, e->ks.HW, counts_dev, coords_dev, stream, "sgw_layer_coords");
}

int sgw_agent_layer_coords(sgw_engine* e, const uint8_t* views_dev, int n_layers, const int32_t* agent_layer, int cap,
                           int32_t* counts_dev, int16_t* coords_dev, void* stream) {
  if (!e || !views_dev || !agent_layer || !counts_dev || !coords_dev || n_layers < 1 || n_layers > 32 || cap < 1)
    return fail(SGW_ERR_ARG, "sgw_agent_layer_coords: bad argument (pointers, n_layers in 1..32, cap >= 1)");
  const ViewSpec v = make_viewspec(e);
  if (v.total <= 0) return fail(SGW_ERR_UNSUPPORTED, "sgw_agent_layer_coords: the spec defines no agent views");
  CoordGeom g; memset(&g, 0, sizeof(g));
  g.L = n_layers; g.A = v.A; g.cap = cap;
  int max_cells = 0;
  for (int a = 0; a < v.A; ++a) {
    if (agent_layer[a] >= n_layers) return fail(SGW_ERR_ARG, "sgw_agent_layer_coords: agent_layer out of range");
    g.cells[a] = v.vh[a] * v.vw[a]; g.W[a] = v.vw[a]; g.off[a] = v.off[a] * n_layers;
    g.own[a] = agent_layer[a] < 0 ? -1 : agent_layer[a];
    max_cells = g.cells[a] > max_cells ? g.cells[a] : max_cells;
  }
  g.row_bytes = (long long)v.total * n_layers;
  return coords_launch(e, true, views_dev, e->n_envs * v.A * n_layers, g, max_cells, counts_dev, coords_dev, stream, "sgw_agent_layer_coords");
}

int sgw_track_performance(sgw_engine* e, const double* perf_dev, int n_cols, const uint8_t* step_type_dev, double* last_dev,
                          double* sum_dev, int64_t* count_dev, uint8_t* done_dev, void* stream) {
  if (!e || !perf_dev || !step_type_dev || n_cols < 1) return fail(SGW_ERR_ARG, "sgw_track_performance: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  const long long total = e->n_envs * n_cols;
  const int per_agent = spec_per_agent(e->spec) ? 1 : 0;
  hipLaunchKernelGGL(k_track_performance, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, perf_dev, n_cols,
                     step_type_dev, e->spec.A, per_agent, (long long)e->n_envs, last_dev, sum_dev, reinterpret_cast<long long*>(count_dev), done_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_sizeof_episodes(void) { return (int)sizeof(sgw_episodes); }

// tiles of 64 envs in T rows of round_up(n_envs, 64); -1 when a wave's 32-bit tile number / a call's 32-bit prefix would not hold
static long long episode_tiles(long long n_envs, int T) {
  if (n_envs < 1 || T < 1 || n_envs > 0x7fffffffLL) return -1;
  const long long tiles = (long long)T * ((n_envs + WAVE - 1) / WAVE);
  return tiles * WAVE > 0x7fffffffLL ? -1 : tiles;
}

int64_t sgw_episode_scratch_bytes(int64_t n_envs, int T) {
  const long long tiles = episode_tiles(n_envs, T);
  if (tiles < 0) return SGW_ERR_ARG;
  return (int64_t)sizeof(EpisodeScratch) + 4 * ((tiles + 3) / 4 * 4);
}

int sgw_log_episodes(sgw_engine* e, const sgw_out* src, int T, int64_t step_base, const sgw_episodes* log, void* stream) {
  if (!e || !src || !log) return fail(SGW_ERR_ARG, "sgw_log_episodes: null argument");
  if (!src->step_type || !log->count || !log->scratch) return fail(SGW_ERR_ARG, "sgw_log_episodes: src->step_type, log->count and log->scratch are required");
  const long long tiles = episode_tiles(e->n_envs, T);
  if (tiles < 0 || log->cap < 0) return fail(SGW_ERR_ARG, "sgw_log_episodes: bad argument (T >= 1, T * N_pad < 2^31, cap >= 0)");
  if ((log->length && !src->frame) || (log->term_reason && !src->term_reason) || (log->ret && !src->cumulative) ||
      (log->hidden && !src->hidden) || (log->metrics && !src->metrics))
    return fail(SGW_ERR_ARG, "sgw_log_episodes: a destination array is given whose source output is NULL");
  if (((uintptr_t)log->scratch | (uintptr_t)log->count | (uintptr_t)log->step | (uintptr_t)log->ret | (uintptr_t)log->hidden | (uintptr_t)log->metrics) & 7)
    return fail(SGW_ERR_ARG, "sgw_log_episodes: scratch, count and the 8-byte arrays must be 8-byte aligned");
  if (((uintptr_t)log->env | (uintptr_t)log->length) & 3) return fail(SGW_ERR_ARG, "sgw_log_episodes: env and length must be 4-byte aligned");
  const sgw_spec& sp = e->spec;
  EpisodeArgs x; memset(&x, 0, sizeof(x));
  x.step_type = src->step_type; x.term_reason = src->term_reason; x.frame = src->frame;
  x.cumulative = reinterpret_cast<const unsigned long long*>(src->cumulative);
  x.hidden = reinterpret_cast<const unsigned long long*>(src->hidden);
  x.metrics = reinterpret_cast<const unsigned long long*>(src->metrics);
  x.n = e->n_envs; x.n_pad = e->n_pad; x.step_base = step_base;
  x.tiles = (unsigned)tiles; x.tiles_per_t = (unsigned)(e->n_pad / WAVE);
  x.A = sp.A; x.per_agent = spec_per_agent(sp) ? 1 : 0;
  x.R = x.per_agent ? sp.A : 1; x.C = sp.A * sp.K; x.M = sp.M;
  x.recip_C = x.C <= 1 ? 0 : (int)(uint32_t)(((1ull << 32) + x.C - 1) / x.C);      // exact: a span has at most 64 * C elements
  x.recip_M = x.M <= 1 ? 0 : (int)(uint32_t)(((1ull << 32) + x.M - 1) / x.M);
  x.cap = log->cap;
  x.env = log->env; x.step = reinterpret_cast<long long*>(log->step); x.length = log->length; x.reason = log->term_reason;
  x.ret = x.C > 0 ? reinterpret_cast<unsigned long long*>(log->ret) : nullptr;
  x.hid = reinterpret_cast<unsigned long long*>(log->hidden);
  x.met = x.M > 0 ? reinterpret_cast<unsigned long long*>(log->metrics) : nullptr;
  x.head = static_cast<EpisodeScratch*>(log->scratch);
  x.tile_num = reinterpret_cast<unsigned*>(x.head + 1);
  HIP_TRY(hipSetDevice(e->device));
  const unsigned blocks = (unsigned)((tiles + 3) / 4);                // 4 waves per workgroup, a tile per wave
  hipLaunchKernelGGL(k_episode_count, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x.step_type, x.tiles, x.tiles_per_t, x.n, x.n_pad,
                     x.A, x.per_agent, x.tile_num);
  hipLaunchKernelGGL(k_episode_scan, dim3(1), dim3(EPISODE_SCAN_THREADS), 0, (hipStream_t)stream, x.tile_num, x.tiles, x.head,
                     reinterpret_cast<long long*>(log->count));
  if (x.cap > 0 && (x.env || x.step || x.length || x.reason || x.ret || x.hid || x.met))
    hipLaunchKernelGGL(k_episode_write, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

// RGB + unoccluded layers + performance bookkeeping of the step that just ran, in ONE launch (k_step_extras)
static int step_extras_launch(sgw_engine* e, const sgw_out* out, const sgw_extras* x, bool layers_here, void* stream) {
  const bool perf = x->perf_last || x->perf_sum || x->perf_count || x->done;
  if (!x->rgb && !layers_here && !perf) return SGW_OK;
  if (layers_here && x->n_layers > 32) return fail(SGW_ERR_UNSUPPORTED, "sgw_step_full: at most 32 layers (a cell's layers are one 32-bit mask)");
  ExtrasArgs ea; memset(&ea, 0, sizeof(ea));
  const size_t HW = (size_t)e->ks.HW;
  const int A = e->spec.A, K = e->spec.K;
  const bool planes = x->rgb || layers_here;
  const int epb = (planes && 5 * PLANES_ENVS * HW > 40 * 1024) ? 16 : PLANES_ENVS;
  ea.board = out->board; ea.n = e->n_envs; ea.epb = epb; ea.HW = (int)HW; ea.W = e->ks.W; ea.A = A; ea.K = K;
  if (!plane_geom((int)HW, 3, ea.g_rgb) || !plane_geom((int)HW, layers_here ? x->n_layers : 1, ea.g_lay))
    return fail(SGW_ERR_UNSUPPORTED, "sgw_step_full: board / layer count outside the plane kernels' index arithmetic");
  ea.rgb_lut = x->rgb_lut_dev; ea.rgb = x->rgb;
  if (layers_here) {
    ea.chars = x->layer_chars_dev; ea.stat = x->layer_static_dev; ea.gap = x->gap_index; ea.hidden = x->hidden_layer >= 0 ? x->hidden_layer : -1;
    ea.pos = x->hidden_layer >= 0 ? out->agent_pos : nullptr; ea.flags = x->hidden_layer >= 0 ? out->agent_flags : nullptr; ea.layers = x->layers;
  }
  if (perf) {
    ea.perf = x->perf_from_hidden ? out->hidden : out->cumulative; ea.perf_cols = x->perf_from_hidden ? 1 : A * K;
    ea.per_agent = spec_per_agent(e->spec) ? 1 : 0;
    ea.step_type = out->step_type; ea.last = x->perf_last; ea.sum = x->perf_sum; ea.count = reinterpret_cast<long long*>(x->perf_count); ea.done = x->done;
  }
  // LDS: boards | layer masks | per-cell + per-char tables | colour table
  ea.lds_planes = planes ? (int)((((size_t)epb * HW + 15) & ~(size_t)15) + epb * HW * 4 + HW * 8 + 512 + 3 * 128) : 0;
  const size_t lds = (size_t)ea.lds_planes;
  int rc = raise_lds_cap(e, reinterpret_cast<const void*>(&k_step_extras), lds, 64u);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_step_extras, dim3((unsigned)((e->n_envs + epb - 1) / epb)), dim3(PLANES_THREADS), lds, (hipStream_t)stream, ea);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

static int step_full_launches(sgw_engine* e, const int8_t* actions_dev, const sgw_out* out, const sgw_extras* x, void* stream) {
  int rc = sgw_step(e, actions_dev, out, stream);
  if (rc || !x) return rc;
  const bool layers_here = x->layers && e->spec.family != SGW_AINTELOPE_SAVANNA;       // savanna's layers come from its state bitmaps
  rc = step_extras_launch(e, out, x, layers_here, stream);
  if (rc) return rc;
  if (x->layers && !layers_here) { rc = sgw_state_layers(e, x->layer_chars_dev, x->n_layers, 1, x->layers, stream); if (rc) return rc; }
  if (x->stats) { rc = sgw_derived_stats(e, out->reward, out->cumulative, out->frame, x->k_agent, x->stats, stream); if (rc) return rc; }
  if (x->agent_layer_views) {
    const bool rot = e->spec.family != SGW_FIREMAKER_EX_MA || e->ks.view_rotates;   // observation directions come in agent_flags (UP = no rotation)
    rc = sgw_agent_layer_views(e, x->layers, out->agent_pos, rot ? out->agent_flags : nullptr, x->layer_chars_dev, x->n_layers,
                               (uint8_t)(e->ks.view_pad), x->agent_layer_views, stream);
    if (rc) return rc;
  }
  return SGW_OK;
}

int sgw_step_full(sgw_engine* e, const int8_t* actions_dev, const sgw_out* out, const sgw_extras* x, void* stream) {
  if (!e || !actions_dev || !out) return fail(SGW_ERR_ARG, "sgw_step_full: null argument");
  if (x) {
    if ((x->rgb || (x->layers && e->spec.family != SGW_AINTELOPE_SAVANNA)) && !out->board)
      return fail(SGW_ERR_ARG, "sgw_step_full: rgb / layers need the board output");
    if (x->rgb && !x->rgb_lut_dev) return fail(SGW_ERR_ARG, "sgw_step_full: rgb requested without a LUT");
    if (x->layers && (!x->layer_chars_dev || x->n_layers < 1)) return fail(SGW_ERR_ARG, "sgw_step_full: bad layer list");
    if (x->layers && x->hidden_layer >= 0 && (!out->agent_pos || !out->agent_flags))
      return fail(SGW_ERR_ARG, "sgw_step_full: a hidden drape layer needs the agent_pos and agent_flags outputs");
    if (x->agent_layer_views && (!x->layers || !out->agent_pos || !out->agent_flags))
      return fail(SGW_ERR_ARG, "sgw_step_full: agent layer cubes need `layers` and the agent_pos / agent_flags outputs");
    if (x->stats && (!out->reward || !out->cumulative || !out->frame))
      return fail(SGW_ERR_ARG, "sgw_step_full: stats need the reward, cumulative and frame outputs");
    if ((x->perf_last || x->perf_sum || x->perf_count || x->done) && (!out->step_type || !(x->perf_from_hidden ? (const void*)out->hidden : (const void*)out->cumulative)))
      return fail(SGW_ERR_ARG, "sgw_step_full: performance bookkeeping needs step_type and the cumulative (or hidden) output");
  }
  auto launches = [&](hipStream_t s) { return step_full_launches(e, actions_dev, out, x, s); };
  if (!x || !x->replay || step_graphs_min_T() > 8) return launches((hipStream_t)stream);     // (SGW_STEP_GRAPHS=0: never replay)
  GraphKey<1> key; memset(&key, 0, sizeof(key));
  key.actions[0] = actions_dev; key.outs[0] = *out; key.ex = *x; key.epochs[0] = e->arg_epoch;
  key.n = 1; key.T = 1; key.has_out = 1;
  return e->full_graphs.run(e->graph_owner, key, 1, launches, (hipStream_t)stream, "sgw_step_full");
}

int sgw_get_state(sgw_engine* e, uint64_t* state_dev, void* stream) {
  if (!e || !state_dev) return fail(SGW_ERR_ARG, "sgw_get_state: null argument");
  HIP_TRY(hipSetDevice(e->device));
  const long long total = (long long)e->ks.words * e->n_pad;
  hipLaunchKernelGGL(k_state_export, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->state_dev,
                     e->n_pad, e->ks.words, state_dev);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_set_state(sgw_engine* e, const uint64_t* state_dev, void* stream) {
  if (!e || !state_dev) return fail(SGW_ERR_ARG, "sgw_set_state: null argument");
  HIP_TRY(hipSetDevice(e->device));
  const long long total = (long long)e->ks.words * e->n_pad;
  hipLaunchKernelGGL(k_state_import, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, e->state_dev,
                     e->n_pad, e->ks.words, state_dev);
  HIP_TRY(hipGetLastError());
  e->rng_set = 1;          // a saved state carries its envs' generator streams (resume needs no sgw_set_rng_state)
  return SGW_OK;
}

int64_t sgw_out_row_bytes(const sgw_engine* e, int field) {
  if (!e || field < 0 || field >= COPY_PLANES) { fail(SGW_ERR_ARG, "sgw_out_row_bytes: null engine or no such output"); return SGW_ERR_ARG; }
  return (int64_t)out_row_bytes(e->spec, field);
}

int sgw_copy_envs(sgw_engine* dst, const sgw_engine* src, const int32_t* dst_idx_dev, const int32_t* src_idx_dev, int64_t n,
                  const sgw_out* dst_out, const sgw_out* src_out, void* stream) {
  if (!dst || !src) return fail(SGW_ERR_ARG, "sgw_copy_envs: null engine");
  if (n < 0) return fail(SGW_ERR_ARG, "sgw_copy_envs: n < 0");
  if (dst != src) {
    if (dst->device != src->device) return fail(SGW_ERR_ARG, "sgw_copy_envs: the engines are on different devices");
    if (memcmp(&dst->spec, &src->spec, sizeof(sgw_spec)) != 0 || dst->ks.words != src->ks.words)
      return fail(SGW_ERR_ARG, "sgw_copy_envs: the engines' specs (or state layouts) differ");
  }
  const int fam = dst->spec.family;
  if ((fam == SGW_FIREMAKER_EX_MA || fam == SGW_ISLAND_NAVIGATION_EX_MA || fam == SGW_AINTELOPE_SAVANNA) && !dst->rng_set)
    return fail(SGW_ERR_ARG, "sgw_copy_envs: the destination's generators were never set (sgw_set_rng_state, sgw_seed_rng or "
                "sgw_set_state first: its padding lanes need a working stream)");
  if (((uintptr_t)dst_idx_dev | (uintptr_t)src_idx_dev) & 3) return fail(SGW_ERR_ARG, "sgw_copy_envs: index arrays must be 4-byte aligned");
  CopyArgs a; memset(&a, 0, sizeof(a));
  a.src_state = src->state_dev; a.dst_state = dst->state_dev; a.src_idx = src_idx_dev; a.dst_idx = dst_idx_dev;
  a.n = n; a.src_n = src->n_envs; a.dst_n = dst->n_envs; a.words = dst->ks.words; a.same = dst == src ? 1 : 0;
  if (dst_out) {
    void* const* dp = reinterpret_cast<void* const*>(dst_out);
    void* const* sp = reinterpret_cast<void* const*>(src_out);
    for (int f = 0; f < COPY_PLANES; ++f) {
      if (!dp[f]) continue;
      if (!sp || !sp[f]) return fail(SGW_ERR_ARG, "sgw_copy_envs: an output is set in dst_out and NULL in src_out");
      const long long rb = out_row_bytes(dst->spec, f);
      if (rb <= 0) continue;                       // the family has no such output: nothing to move
      CopyPlane& pl = a.planes[a.n_planes++];
      pl.src = static_cast<const uint8_t*>(sp[f]); pl.dst = static_cast<uint8_t*>(dp[f]); pl.row_bytes = (int)rb;
    }
  }
  if (n == 0) return SGW_OK;
  const long long waves = copy_plan(a);
  if (n > 0x7fffffffLL || waves > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_copy_envs: too many pairs for one launch (2^31 waves)");
  HIP_TRY(hipSetDevice(dst->device));
  hipLaunchKernelGGL(k_copy_envs, dim3((unsigned)((waves + COPY_THREADS / WAVE - 1) / (COPY_THREADS / WAVE))), dim3(COPY_THREADS), 0,
                     (hipStream_t)stream, a, (unsigned)waves);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_scalarise(sgw_engine* e, const double* reward_dev, const double* cumulative_dev, const int32_t* frame_dev, int T,
                  const int32_t* k_agent, double* scalar_reward_dev, double* scalar_cumulative_dev, double* scalar_average_dev,
                  void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_scalarise: null engine");
  if (T < 1) return fail(SGW_ERR_ARG, "sgw_scalarise: T < 1");
  if (!scalar_reward_dev && !scalar_cumulative_dev && !scalar_average_dev) return fail(SGW_ERR_ARG, "sgw_scalarise: no output");
  if ((scalar_reward_dev && !reward_dev) || (scalar_cumulative_dev && !cumulative_dev) || (scalar_average_dev && (!cumulative_dev || !frame_dev)))
    return fail(SGW_ERR_ARG, "sgw_scalarise: an output's source is NULL (scalar_reward: reward; scalar_cumulative: cumulative; "
                "scalar_average: cumulative and frame)");
  const int A = e->spec.A, K = e->spec.K;
  static_assert(SGW_MAX_K == 16, "k_scalarise dispatches on 1..16 reward dimensions");
  ScalariseArgs a; memset(&a, 0, sizeof(a));
  for (int ag = 0; ag < A; ++ag) {
    const int k = k_agent ? k_agent[ag] : K;
    if (k < 0 || k > K) return fail(SGW_ERR_ARG, "sgw_scalarise: k_agent out of range");
    a.k[ag] = k;
  }
  a.reward = scalar_reward_dev ? reward_dev : nullptr;               // a source nobody asks for is not read
  a.cumulative = (scalar_cumulative_dev || scalar_average_dev) ? cumulative_dev : nullptr;
  a.frame = scalar_average_dev ? frame_dev : nullptr;
  if (((uintptr_t)a.reward | (uintptr_t)a.cumulative) & 15)
    return fail(SGW_ERR_ARG, "sgw_scalarise: reward / cumulative must be 16-byte aligned (rows move as 16-byte accesses)");
  if (((uintptr_t)scalar_reward_dev | (uintptr_t)scalar_cumulative_dev | (uintptr_t)scalar_average_dev) & 7 || ((uintptr_t)a.frame & 3))
    return fail(SGW_ERR_ARG, "sgw_scalarise: misaligned output or frame pointer");
  a.scalar_reward = scalar_reward_dev; a.scalar_cumulative = scalar_cumulative_dev; a.scalar_average = scalar_average_dev;
  a.n = e->n_envs; a.n_pad = e->n_pad; a.A = A; a.K = K;
  a.recip_AK = ((1 << 18) + A * K - 1) / (A * K);
  const long long chunks = (e->n_envs + WAVE - 1) / WAVE;
  if (chunks == 0) return SGW_OK;
  if (chunks * T > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_scalarise: too many rows for one launch (2^31 waves)");
  a.chunks = (unsigned)chunks;
  HIP_TRY(hipSetDevice(e->device));
  const size_t lds = (size_t)2 * A * K * WAVE * 8;                   // R | C (sgw_scalarise.hpp): <= 64 KiB for A K <= 64
  hipLaunchKernelGGL(k_scalarise, dim3((unsigned)(chunks * T)), dim3(WAVE), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

}  // extern "C"

// ---- table policies: sgw_policy_act, sgw_policy_step_n (sgw_policy.hpp) -------------------------------------------------------
struct PolicyLaunch { PolicyArgs a; unsigned blocks, threads; size_t lds; };

// the checks of a policy against the engine's spec, and everything of a launch that does not move from step to step
static int policy_plan(const sgw_engine* e, const sgw_policy* p, const char* who, PolicyLaunch& L) {
  if (!p) return fail(SGW_ERR_ARG, "%s: null policy", who);
  if (!p->code_of || !p->weights || !p->step_dev) return fail(SGW_ERR_ARG, "%s: the policy's code_of, weights and step_dev are required", who);
  if (p->source != SGW_POLICY_BOARD && p->source != SGW_POLICY_VIEWS) return fail(SGW_ERR_ARG, "%s: source must be SGW_POLICY_BOARD or SGW_POLICY_VIEWS", who);
  if (p->n_policies < 1) return fail(SGW_ERR_ARG, "%s: n_policies < 1", who);
  if (p->n_codes < 1 || p->n_codes > 64) return fail(SGW_ERR_ARG, "%s: n_codes outside 1..64", who);
  if (p->explore_below > (1ull << 32)) return fail(SGW_ERR_ARG, "%s: explore_below > 2^32", who);
  const sgw_spec& sp = e->spec;
  if (sp.n_actions < 1 || sp.n_actions > POLICY_MAX_ACTIONS) return fail(SGW_ERR_UNSUPPORTED, "%s: table policies take specs with 1..16 actions", who);
  PolicyArgs& a = L.a; memset(&a, 0, sizeof(a));
  int need = 0;
  if (p->source == SGW_POLICY_VIEWS) {
    const ViewSpec v = make_viewspec(e);
    if (v.total <= 0) return fail(SGW_ERR_ARG, "%s: source VIEWS on a spec without agent windows", who);
    a.row_bytes = v.total;
    for (int ag = 0; ag < sp.A; ++ag) {
      a.c_a[ag] = v.vh[ag] * v.vw[ag]; a.off_a[ag] = v.off[ag];
      need = a.c_a[ag] > need ? a.c_a[ag] : need;
    }
  } else {
    a.row_bytes = need = sp.H * sp.W;
    for (int ag = 0; ag < sp.A; ++ag) { a.c_a[ag] = need; a.off_a[ag] = 0; }
  }
  if (p->cells < need) return fail(SGW_ERR_ARG, "%s: cells is smaller than the source needs (H*W, or the largest window)", who);
  int E = 64;
  while (E > 16 && (long long)E * a.row_bytes > POLICY_MAX_ROW_LDS) E >>= 1;
  if ((long long)E * a.row_bytes > POLICY_MAX_ROW_LDS) return fail(SGW_ERR_UNSUPPORTED, "%s: the observation row is too long to stage", who);
  const long long blocks = (e->n_envs + E - 1) / E;
  if (blocks > 0x7fffffffLL) return fail(SGW_ERR_ARG, "%s: too many envs for one launch", who);
  a.code_of = p->code_of; a.weights = p->weights; a.bias = p->bias; a.policy_of_env = p->policy_of_env; a.step_dev = p->step_dev;
  a.explore_below = p->explore_below; a.seed = p->seed;
  a.n = e->n_envs; a.env_id_base = e->env_id_base;
  a.envs_per_block = E; a.A = sp.A; a.P = p->n_policies; a.G = p->n_codes; a.C = p->cells; a.n_actions = sp.n_actions; a.action_lo = sp.action_lo;
  const int pairs = E * sp.A;
  L.blocks = (unsigned)blocks;
  L.threads = (unsigned)(pairs >= POLICY_THREADS_MAX ? POLICY_THREADS_MAX : (pairs + WAVE - 1) / WAVE * WAVE);
  L.lds = ((size_t)E * a.row_bytes + 15) / 16 * 16 + 256;
  return SGW_OK;
}

// sampled: k_policy_sample (sgw_softmax.hpp) with beta2 in place of the greedy k_policy_act; the same grid, threads and LDS
static int policy_launch(const sgw_engine* e, PolicyLaunch& L, const uint8_t* obs, long long t, int8_t* actions, hipStream_t st,
                         bool sampled = false, float beta2 = 0.0f) {
  if (((uintptr_t)obs) & 15) return fail(SGW_ERR_ARG, "policy: the observation rows must be 16-byte aligned (they move as 16-byte accesses)");
  if (L.blocks == 0) return SGW_OK;
  L.a.obs = obs; L.a.t = t; L.a.actions = actions;
  HIP_TRY(hipSetDevice(e->device));
  if (sampled) {
    SampleArgs s; memset(&s, 0, sizeof(s));
    s.p = L.a; s.beta2 = beta2;
    hipLaunchKernelGGL(k_policy_sample, dim3(L.blocks), dim3(L.threads), L.lds, st, s);
  } else {
    hipLaunchKernelGGL(k_policy_act, dim3(L.blocks), dim3(L.threads), L.lds, st, L.a);
  }
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

// beta2 = inverse temperature * log2(e): finite and >= 0
static bool beta2_ok(float beta2) { return beta2 >= 0.0f && beta2 <= 3.4028234663852886e38f; }

// sgw_policy_step_n and sgw_policy_sample_step_n: the 2T + 1 launch chain, the acting launch greedy or sampled
static int policy_step_chain(sgw_engine* e, const sgw_policy* p, bool sampled, float beta2, const uint8_t* obs0_dev, int T, int write_every,
                             const sgw_out* out, int8_t* actions_out_dev, int accumulate, void* stream, const char* who) {
  if (!e) return fail(SGW_ERR_ARG, "%s: null engine", who);
  if (T < 1) return fail(SGW_ERR_ARG, "%s: T < 1", who);
  if (!obs0_dev || !actions_out_dev || !out) return fail(SGW_ERR_ARG, "%s: obs0, out and actions_out are required", who);
  if (sampled && !beta2_ok(beta2)) return fail(SGW_ERR_ARG, "%s: beta2 must be finite and >= 0", who);
  PolicyLaunch L;
  int rc = policy_plan(e, p, who, L);
  if (rc) return rc;
  const bool from_views = p->source == SGW_POLICY_VIEWS;
  const uint8_t* produced = from_views ? out->views : out->board;         // what a step leaves for the next act
  if (!produced)
    return fail(SGW_ERR_ARG, from_views ? "%s: the policy's source (views) is not among the outputs" : "%s: the policy's source (board) is not among the outputs", who);
  const long long per_step = e->n_envs * e->spec.A, obs_step = e->n_pad * (long long)L.a.row_bytes;
  const hipStream_t st = (hipStream_t)stream;
  auto launches = [&](hipStream_t s) -> int {
    for (int t = 0; t < T; ++t) {
      int8_t* row = actions_out_dev + (long long)t * per_step;
      const uint8_t* obs = t == 0 ? obs0_dev : (write_every ? produced + (long long)(t - 1) * obs_step : produced);
      int r = policy_launch(e, L, obs, t, row, s, sampled, beta2);
      if (r) return r;
      KArgs a;
      r = step_args(e, row, 1, 0, 0, 0, out, accumulate, a);
      if (r) return r;
      if (write_every) offset_out(a.out, e->spec, e->n_pad, t);
      r = launch(e, a, s);
      if (r) return r;
    }
    HIP_TRY(hipSetDevice(e->device));
    hipLaunchKernelGGL(k_policy_advance, dim3(1), dim3(1), 0, s, p->step_dev, (long long)T);
    HIP_TRY(hipGetLastError());
    return (int)SGW_OK;
  };
  if (T < step_graphs_min_T()) return launches(st);
  GraphKey<1> key; memset(&key, 0, sizeof(key));
  key.actions[0] = actions_out_dev; key.epochs[0] = e->arg_epoch; key.pol = *p; key.obs0 = obs0_dev;
  key.n = 1; key.T = T; key.write_every = write_every != 0; key.accumulate = accumulate != 0; key.has_out = 1;
  key.sampled = sampled ? 1 : 0; key.beta2 = sampled ? beta2 : 0.0f;
  key.outs[0] = *out;
  return e->policy_graphs.run(e->graph_owner, key, 2LL * T + 1, launches, st, who);
}

extern "C" {

int sgw_sizeof_policy(void) { return (int)sizeof(sgw_policy); }

int sgw_policy_act(sgw_engine* e, const sgw_policy* p, const uint8_t* obs_dev, int64_t t, int8_t* actions_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_policy_act: null engine");
  if (!obs_dev || !actions_dev) return fail(SGW_ERR_ARG, "sgw_policy_act: null observation or actions");
  PolicyLaunch L;
  const int rc = policy_plan(e, p, "sgw_policy_act", L);
  if (rc) return rc;
  return policy_launch(e, L, obs_dev, (long long)t, actions_dev, (hipStream_t)stream);
}

int sgw_policy_step_n(sgw_engine* e, const sgw_policy* p, const uint8_t* obs0_dev, int T, int write_every, const sgw_out* out,
                      int8_t* actions_out_dev, int accumulate, void* stream) {
  return policy_step_chain(e, p, false, 0.0f, obs0_dev, T, write_every, out, actions_out_dev, accumulate, stream, "sgw_policy_step_n");
}

int sgw_policy_sample(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs_dev, int64_t t, int8_t* actions_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_policy_sample: null engine");
  if (!obs_dev || !actions_dev) return fail(SGW_ERR_ARG, "sgw_policy_sample: null observation or actions");
  if (!beta2_ok(beta2)) return fail(SGW_ERR_ARG, "sgw_policy_sample: beta2 must be finite and >= 0");
  PolicyLaunch L;
  const int rc = policy_plan(e, p, "sgw_policy_sample", L);
  if (rc) return rc;
  return policy_launch(e, L, obs_dev, (long long)t, actions_dev, (hipStream_t)stream, true, beta2);
}

int sgw_policy_sample_step_n(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs0_dev, int T, int write_every,
                             const sgw_out* out, int8_t* actions_out_dev, int accumulate, void* stream) {
  return policy_step_chain(e, p, true, beta2, obs0_dev, T, write_every, out, actions_out_dev, accumulate, stream, "sgw_policy_sample_step_n");
}

}  // extern "C"

// ---- what each action would do: sgw_simulate_moves, sgw_fold_q_values (sgw_whatif.hpp) -----------------------------------------
// The families whose agents are AgentSafetySpriteMo / its multi-agent twin with a pinned simulate_update, their per-agent
// impassable characters (the env modules' sprite constructors) and whether actions are relative to the action direction
static int whatif_family(const sgw_engine* e, const char* who, unsigned long long (&imp)[SGW_MAX_AGENTS], int& relative) {
  const sgw_spec& sp = e->spec;
  auto set_of = [](const char* chars, char own) {
    unsigned long long v = 0; int k = 0;
    for (const char* c = chars; *c; ++c) if (*c != own) v |= (unsigned long long)(uint8_t)*c << (8 * k++);
    return v;
  };
  for (int ag = 0; ag < SGW_MAX_AGENTS; ++ag) imp[ag] = 0;
  relative = 0;
  switch (sp.family) {
    case SGW_ISLAND_NAVIGATION_EX: case SGW_BOAT_RACE_EX:                    // island_navigation_ex.py:420, boat_race_ex.py:182
      imp[0] = set_of("#", 0); break;
    case SGW_CONVEYOR_BELT:                                                  // conveyor_belt_ex.py:198: the wall and the object
      if (sp.params[Conveyor::P_MO_TWIN] == 0.0)
        return fail(SGW_ERR_UNSUPPORTED, "%s: conveyor_belt is a scalar original env (no simulate_update); conveyor_belt_ex is covered", who);
      imp[0] = set_of("#O", 0); break;
    case SGW_ISLAND_NAVIGATION_EX_MA:                                        // island_navigation_ex_ma.py:533
      imp[0] = set_of("#12", '1'); imp[1] = set_of("#12", '2');
      relative = (sp.flags & (IslandMa::F_ADIR | IslandMa::F_ADIR_TURN)) ? 1 : 0; break;
    case SGW_AINTELOPE_SAVANNA:                                              // aintelope_savanna.py:773
      imp[0] = set_of("#01", '0'); imp[1] = set_of("#01", '1');
      relative = (sp.flags & (Savanna::F_ADIR | Savanna::F_ADIR_TURN)) ? 1 : 0; break;
    case SGW_FIREMAKER_EX_MA:                                                // firemaker_ex_ma.py:400; agent slots '1', '2', 'S'
      imp[0] = set_of("#12S", '1'); imp[1] = set_of("#12S", '2'); imp[2] = set_of("#12S", 'S');
      relative = (sp.flags & (Firemaker::F_ADIR | Firemaker::F_ADIR_TURN)) ? 1 : 0; break;
    case SGW_SAFE_INTERRUPTIBILITY:
      return fail(SGW_ERR_UNSUPPORTED, "%s: safe_interruptibility(_ex): its PolicyWrapperDrape's ACTUAL_ACTIONS entry would replace the "
                                       "queried action in simulate_update, which is not pinned", who);
    default:
      return fail(SGW_ERR_UNSUPPORTED, "%s: the scalar original env families have no simulate_update", who);
  }
  if (sp.action_lo != 0) return fail(SGW_ERR_UNSUPPORTED, "%s: the action set must start at NOOP (action_lo == 0, noops=True)", who);
  if (sp.n_actions < 1 || sp.n_actions > WHATIF_MAX_ACTIONS) return fail(SGW_ERR_UNSUPPORTED, "%s: action sets of 1..9 actions (NOOP, moves, turning actions)", who);
  return SGW_OK;
}

extern "C" {

int sgw_simulate_moves(sgw_engine* e, const uint8_t* board_dev, const uint8_t* agent_pos_dev, const uint8_t* agent_flags_dev,
                       uint8_t* target_pos_dev, uint8_t* target_tile_dev, uint8_t* blocked_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_simulate_moves: null engine");
  if (!board_dev || !agent_pos_dev) return fail(SGW_ERR_ARG, "sgw_simulate_moves: board and agent_pos are required");
  if (!target_pos_dev && !target_tile_dev && !blocked_dev) return fail(SGW_ERR_ARG, "sgw_simulate_moves: no output");
  if (((uintptr_t)board_dev) & 15) return fail(SGW_ERR_ARG, "sgw_simulate_moves: the board rows must be 16-byte aligned (they move as 16-byte accesses)");
  WhatifArgs a; memset(&a, 0, sizeof(a));
  const int rc = whatif_family(e, "sgw_simulate_moves", a.impassable, a.relative);
  if (rc) return rc;
  const sgw_spec& sp = e->spec;
  const long long blocks = (e->n_envs + WHATIF_ENVS - 1) / WHATIF_ENVS;
  if (blocks > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_simulate_moves: too many envs for one launch");
  if (blocks == 0) return SGW_OK;
  a.board = board_dev; a.agent_pos = agent_pos_dev; a.agent_flags = agent_flags_dev;
  a.target_pos = target_pos_dev; a.target_tile = target_tile_dev; a.blocked = blocked_dev;
  a.n = e->n_envs; a.H = sp.H; a.W = sp.W; a.A = sp.A; a.n_actions = sp.n_actions;
  const int pairs = WHATIF_ENVS * sp.A;
  const unsigned threads = (unsigned)(pairs >= WHATIF_THREADS_MAX ? WHATIF_THREADS_MAX : (pairs + WAVE - 1) / WAVE * WAVE);
  const size_t lds = ((size_t)WHATIF_ENVS * sp.H * sp.W + 15) / 16 * 16 + (size_t)pairs * sp.n_actions * 4;   // <= 20 480 + 9 216
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_simulate_moves, dim3((unsigned)blocks), dim3(threads), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_fold_q_values(sgw_engine* e, const uint8_t* target_tile_dev, const double* q_dev, int D, const uint8_t* tile_chars_dev, int L,
                      double* table_dev, uint8_t* seen_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_fold_q_values: null engine");
  if (!target_tile_dev || !q_dev || !tile_chars_dev || !table_dev) return fail(SGW_ERR_ARG, "sgw_fold_q_values: target_tile, q, tile_chars and table are required");
  if (D < 1) return fail(SGW_ERR_ARG, "sgw_fold_q_values: D < 1");
  if (L < 1 || L > WHATIF_MAX_TILES) return fail(SGW_ERR_ARG, "sgw_fold_q_values: L outside 1..64");
  if ((((uintptr_t)q_dev) | ((uintptr_t)table_dev)) & 7) return fail(SGW_ERR_ARG, "sgw_fold_q_values: misaligned q or table pointer");
  FoldArgs a; memset(&a, 0, sizeof(a));
  unsigned long long imp[SGW_MAX_AGENTS]; int relative;
  const int rc = whatif_family(e, "sgw_fold_q_values", imp, relative);
  if (rc) return rc;
  const long long lanes = e->n_envs * e->spec.A * (long long)D;
  const long long blocks = (lanes + WHATIF_THREADS_MAX - 1) / WHATIF_THREADS_MAX;
  if (blocks > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_fold_q_values: too many (env, agent, dimension) lanes for one launch");
  if (blocks == 0) return SGW_OK;
  a.target_tile = target_tile_dev; a.q = q_dev; a.tile_chars = tile_chars_dev; a.table = table_dev; a.seen = seen_dev;
  a.n = e->n_envs; a.A = e->spec.A; a.n_actions = e->spec.n_actions; a.D = D; a.L = L;
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_fold_q_values, dim3((unsigned)blocks), dim3(WHATIF_THREADS_MAX), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

// ---- learning targets from rollout buffers: sgw_td_targets (sgw_targets.hpp) ---------------------------------------------------
int sgw_sizeof_td(void) { return (int)sizeof(sgw_td); }

int sgw_td_targets(sgw_engine* e, const sgw_td* td, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_td_targets: null engine");
  if (!td) return fail(SGW_ERR_ARG, "sgw_td_targets: null sgw_td");
  if (!td->reward || !td->step_type || !td->gamma) return fail(SGW_ERR_ARG, "sgw_td_targets: reward, step_type and gamma are required");
  if (!td->ret && !td->adv && !td->valid) return fail(SGW_ERR_ARG, "sgw_td_targets: no output");
  if (td->adv && (!td->value || !td->value0)) return fail(SGW_ERR_ARG, "sgw_td_targets: adv needs value and value0");
  if (td->flags & ~SGW_TD_BOOTSTRAP_TRUNCATED) return fail(SGW_ERR_ARG, "sgw_td_targets: unknown flag bits");
  const bool boot = (td->flags & SGW_TD_BOOTSTRAP_TRUNCATED) != 0;
  if (boot && !td->term_reason) return fail(SGW_ERR_ARG, "sgw_td_targets: SGW_TD_BOOTSTRAP_TRUNCATED needs term_reason");
  if (td->T < 1) return fail(SGW_ERR_ARG, "sgw_td_targets: T < 1");
  if (td->C < 1 || td->C > SGW_MAX_K) return fail(SGW_ERR_ARG, "sgw_td_targets: C outside 1..SGW_MAX_K");
  if (td->src_rows < e->n_envs || td->dst_rows < e->n_envs) return fail(SGW_ERR_ARG, "sgw_td_targets: src_rows / dst_rows < n_envs");
  if (((uintptr_t)td->reward | (uintptr_t)td->value | (uintptr_t)td->value0 | (uintptr_t)td->ret | (uintptr_t)td->adv) & 7)
    return fail(SGW_ERR_ARG, "sgw_td_targets: a double array is not 8-byte aligned");
  const void* in_d[3] = {td->reward, td->value, td->value0};
  for (const void* in : in_d)
    if (in && (in == td->ret || in == td->adv)) return fail(SGW_ERR_ARG, "sgw_td_targets: an output pointer equals an input pointer");
  if (td->valid && (td->valid == td->step_type || td->valid == td->term_reason))
    return fail(SGW_ERR_ARG, "sgw_td_targets: an output pointer equals an input pointer");
  if (td->ret && td->ret == td->adv) return fail(SGW_ERR_ARG, "sgw_td_targets: ret and adv are the same array");
  TdArgs a; memset(&a, 0, sizeof(a));
  a.reward = td->reward; a.step_type = td->step_type; a.term_reason = boot ? td->term_reason : nullptr;
  a.value = td->value; a.value0 = td->adv ? td->value0 : nullptr;          // value0 is read for adv only
  a.ret = td->ret; a.adv = td->adv; a.valid = td->valid;
  a.src_rows = td->src_rows; a.dst_rows = td->dst_rows;
  a.T = td->T; a.A = e->spec.A; a.C = td->C; a.bootstrap = boot ? 1 : 0; a.lambda = td->lambda;
  a.R = (int)out_row_bytes(e->spec, OF_term_reason);                                // term_reason: one column, or one per agent
  if (a.R < 1) a.R = 1;
  for (int c = 0; c < td->C; ++c) a.gamma[c] = td->gamma[c];
  a.n_elems = e->n_envs * a.A * (long long)a.C;
  const long long blocks = (a.n_elems + TD_THREADS - 1) / TD_THREADS;
  if (blocks > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_td_targets: too many (env, agent, column) lanes for one launch");
  if (blocks == 0) return SGW_OK;
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_td_targets, dim3((unsigned)blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

}  // extern "C"

// ---- learning a table policy: sgw_policy_scores, sgw_policy_accumulate, sgw_policy_apply (sgw_learn.hpp) -----------------------
// the T + 1 observations O[0] = obs0, O[s] = row s-1 of obs: required pointers, rows and the 16-byte alignment of every O[s]
static int learn_observations(const sgw_engine* e, const PolicyLaunch& L, const char* who, const uint8_t* obs0, const uint8_t* obs,
                              int64_t obs_rows, int T) {
  if (!obs0) return fail(SGW_ERR_ARG, "%s: null obs0", who);
  if (T > 0 && !obs) return fail(SGW_ERR_ARG, "%s: null obs with T >= 1", who);
  if (T > 0 && obs_rows < e->n_envs) return fail(SGW_ERR_ARG, "%s: obs_rows < n_envs", who);
  if (((uintptr_t)obs0) & 15) return fail(SGW_ERR_ARG, "%s: obs0 is not 16-byte aligned (the rows move as 16-byte accesses)", who);
  if (T > 0 && ((((uintptr_t)obs) & 15) || (T > 1 && ((obs_rows * (long long)L.a.row_bytes) & 15))))
    return fail(SGW_ERR_ARG, "%s: a row block of obs is not 16-byte aligned (the rows move as 16-byte accesses)", who);
  return SGW_OK;
}

extern "C" {

int sgw_policy_scores(sgw_engine* e, const sgw_policy* p, const uint8_t* obs0_dev, const uint8_t* obs_dev, int64_t obs_rows, int T,
                      const int8_t* actions_dev, float* scores_dev, double* vmax_dev, double* chosen_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_policy_scores: null engine");
  if (T < 0) return fail(SGW_ERR_ARG, "sgw_policy_scores: T < 0");
  if (!scores_dev && !vmax_dev && !chosen_dev) return fail(SGW_ERR_ARG, "sgw_policy_scores: no output");
  if (chosen_dev && T > 0 && !actions_dev) return fail(SGW_ERR_ARG, "sgw_policy_scores: chosen needs actions");
  PolicyLaunch L;
  int rc = policy_plan(e, p, "sgw_policy_scores", L);
  if (rc) return rc;
  rc = learn_observations(e, L, "sgw_policy_scores", obs0_dev, obs_dev, obs_rows, T);
  if (rc) return rc;
  if ((((uintptr_t)scores_dev) & 3) || (((uintptr_t)vmax_dev | (uintptr_t)chosen_dev) & 7))
    return fail(SGW_ERR_ARG, "sgw_policy_scores: a misaligned output array");
  const long long groups = L.blocks, blocks = groups * ((long long)T + 1);
  if (blocks > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_policy_scores: too many (observation, env group) blocks for one launch");
  if (blocks == 0) return SGW_OK;
  ScoreArgs a; memset(&a, 0, sizeof(a));
  a.obs0 = obs0_dev; a.obs = obs_dev; a.code_of = p->code_of; a.weights = p->weights; a.bias = p->bias; a.policy_of_env = p->policy_of_env;
  a.actions = actions_dev; a.scores = scores_dev; a.vmax = vmax_dev; a.chosen = T > 0 ? chosen_dev : nullptr;
  a.n = e->n_envs; a.obs_rows = obs_rows; a.groups = groups;
  a.T = T; a.row_bytes = L.a.row_bytes; a.envs_per_block = L.a.envs_per_block; a.A = L.a.A; a.P = L.a.P; a.G = L.a.G; a.C = L.a.C;
  a.n_actions = L.a.n_actions; a.action_lo = L.a.action_lo;
  for (int ag = 0; ag < SGW_MAX_AGENTS; ++ag) { a.c_a[ag] = L.a.c_a[ag]; a.off_a[ag] = L.a.off_a[ag]; }
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_policy_scores, dim3((unsigned)blocks), dim3(L.threads), L.lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

}  // extern "C"

// The argument checks, slices and tiles of sgw_policy_accumulate and sgw_policy_accumulate_softmax.  blocks == 0: nothing
// to launch.
static int accumulate_plan(sgw_engine* e, const sgw_policy* p, const char* who, const uint8_t* obs0_dev, const uint8_t* obs_dev,
                           int64_t obs_rows, int T, const int8_t* actions_dev, const double* coef_dev, int frac_bits, int64_t* acc_weights_dev,
                           int64_t* acc_bias_dev, AccArgs& a, long long& blocks) {
  blocks = 0;
  if (!e) return fail(SGW_ERR_ARG, "%s: null engine", who);
  if (T < 1) return fail(SGW_ERR_ARG, "%s: T < 1", who);
  if (!actions_dev || !coef_dev || !acc_weights_dev) return fail(SGW_ERR_ARG, "%s: actions, coef and acc_weights are required", who);
  if (frac_bits < 0 || frac_bits > 52) return fail(SGW_ERR_ARG, "%s: frac_bits outside 0..52", who);
  PolicyLaunch L;
  int rc = policy_plan(e, p, who, L);
  if (rc) return rc;
  rc = learn_observations(e, L, who, obs0_dev, obs_dev, obs_rows, T - 1);   // O[T] is not read
  if (rc) return rc;
  if (((uintptr_t)coef_dev | (uintptr_t)acc_weights_dev | (uintptr_t)acc_bias_dev) & 7)
    return fail(SGW_ERR_ARG, "%s: coef or an accumulator is not 8-byte aligned", who);
  const void* inputs[] = {obs0_dev, obs_dev, actions_dev, coef_dev, p->code_of, p->weights, p->bias, p->policy_of_env, p->step_dev};
  for (const void* in : inputs)
    if (in && (in == acc_weights_dev || in == acc_bias_dev)) return fail(SGW_ERR_ARG, "%s: an accumulator aliases an input", who);
  if (acc_weights_dev == acc_bias_dev) return fail(SGW_ERR_ARG, "%s: acc_weights and acc_bias are the same array", who);
  if ((long long)T * e->n_envs >= (1LL << 32)) return fail(SGW_ERR_ARG, "%s: T * n_envs >= 2^32 (an int64 sum could wrap)", who);
  memset(&a, 0, sizeof(a));
  const int A = L.a.A, G = L.a.G, NA = L.a.n_actions, P = L.a.P;
  // rows + code_of + (q[n_actions], p) per env + bins: under 64 KiB for every E <= 64 once the rows fit, so E is halved for the rows alone
  static_assert(LEARN_MAX_ROW_LDS + 256 + 64 * (POLICY_MAX_ACTIONS + 1) * 4 + LEARN_MAX_BIN_LDS <= 64 * 1024,
                "the tiles of k_policy_accumulate and k_policy_accumulate_softmax fit the default dynamic LDS");
  int E = 64;
  while (E > 16 && (long long)E * L.a.row_bytes > LEARN_MAX_ROW_LDS) E >>= 1;
  if ((long long)E * L.a.row_bytes > LEARN_MAX_ROW_LDS) return fail(SGW_ERR_UNSUPPORTED, "%s: the observation row is too long to stage", who);
  int max_c = 1;
  for (int ag = 0; ag < A; ++ag) max_c = L.a.c_a[ag] > max_c ? L.a.c_a[ag] : max_c;
  int R = max_c;                                                            // P > 1: no bins, one slice per agent
  if (P == 1) {
    const int fit = (LEARN_MAX_BIN_LDS - NA * 8) / (G * NA * 8);            // >= 2: G <= 64, NA <= 16
    R = fit < max_c ? fit : max_c;
  }
  int slices = 0;
  for (int ag = 0; ag < SGW_MAX_AGENTS; ++ag) {
    a.slice0[ag] = slices;
    if (ag < A) { const int k = (L.a.c_a[ag] + R - 1) / R; slices += k > 0 ? k : 1; }
    a.c_a[ag] = L.a.c_a[ag]; a.off_a[ag] = L.a.off_a[ag];
  }
  const long long groups = (e->n_envs + E - 1) / E, tiles = groups * T;
  if (tiles == 0) return SGW_OK;
  long long per_slice = LEARN_BLOCKS / slices;
  if (per_slice < 1) per_slice = 1;
  if (per_slice > tiles) per_slice = tiles;
  a.obs0 = obs0_dev; a.obs = obs_dev; a.code_of = p->code_of; a.policy_of_env = p->policy_of_env; a.actions = actions_dev; a.coef = coef_dev;
  a.acc_w = reinterpret_cast<unsigned long long*>(acc_weights_dev); a.acc_b = reinterpret_cast<unsigned long long*>(acc_bias_dev);
  a.n = e->n_envs; a.obs_rows = obs_rows; a.groups = groups; a.tiles = tiles; a.scale = ldexp(1.0, frac_bits);
  a.row_bytes = L.a.row_bytes; a.envs_per_block = E; a.A = A; a.P = P; a.G = G; a.C = L.a.C; a.n_actions = NA; a.action_lo = L.a.action_lo;
  a.R = R; a.blocks_per_slice = (int)per_slice;
  blocks = per_slice * slices;
  return SGW_OK;
}

extern "C" {

int sgw_policy_accumulate(sgw_engine* e, const sgw_policy* p, const uint8_t* obs0_dev, const uint8_t* obs_dev, int64_t obs_rows, int T,
                          const int8_t* actions_dev, const double* coef_dev, int frac_bits, int64_t* acc_weights_dev,
                          int64_t* acc_bias_dev, void* stream) {
  AccArgs a;
  long long blocks;
  const int rc = accumulate_plan(e, p, "sgw_policy_accumulate", obs0_dev, obs_dev, obs_rows, T, actions_dev, coef_dev, frac_bits, acc_weights_dev,
                                 acc_bias_dev, a, blocks);
  if (rc || blocks == 0) return rc;
  const size_t lds = ((size_t)a.envs_per_block * a.row_bytes + 15) / 16 * 16 + 256 + (size_t)a.envs_per_block * 12 +
                     (a.P == 1 ? ((size_t)a.R * a.G * a.n_actions + a.n_actions) * 8 : 0);
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_policy_accumulate, dim3((unsigned)blocks), dim3(LEARN_THREADS), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_policy_accumulate_softmax(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs0_dev, const uint8_t* obs_dev,
                                  int64_t obs_rows, int T, const int8_t* actions_dev, const double* coef_dev, int frac_bits,
                                  int64_t* acc_weights_dev, int64_t* acc_bias_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_policy_accumulate_softmax: null engine");
  if (!beta2_ok(beta2)) return fail(SGW_ERR_ARG, "sgw_policy_accumulate_softmax: beta2 must be finite and >= 0");
  SoftAccArgs s; memset(&s, 0, sizeof(s));
  long long blocks;
  const int rc = accumulate_plan(e, p, "sgw_policy_accumulate_softmax", obs0_dev, obs_dev, obs_rows, T, actions_dev, coef_dev, frac_bits,
                                 acc_weights_dev, acc_bias_dev, s.a, blocks);
  if (rc || blocks == 0) return rc;
  s.weights = p->weights; s.bias = p->bias; s.beta2 = beta2;
  const AccArgs& a = s.a;
  const size_t E = (size_t)a.envs_per_block, NA = (size_t)a.n_actions;
  const size_t lds = (E * a.row_bytes + 15) / 16 * 16 + 256 + E * NA * 4 + E * 4 + (a.P == 1 ? ((size_t)a.R * a.G * NA + NA) * 8 : 0);
  // the bytes requested == the bytes the kernel's own layout hands out
  if ((size_t)softmax_acc_lds(a.envs_per_block, a.row_bytes, a.n_actions, a.R, a.G, a.P == 1).total != lds || lds > 64 * 1024)
    return fail(SGW_ERR_ARG, "sgw_policy_accumulate_softmax: LDS footprint mismatch between the launcher and the kernel's layout");
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_policy_accumulate_softmax, dim3((unsigned)blocks), dim3(LEARN_THREADS), lds, (hipStream_t)stream, s);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

int sgw_policy_probs(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs0_dev, const uint8_t* obs_dev, int64_t obs_rows, int T,
                     const int8_t* actions_dev, float* probs_dev, double* p_chosen_dev, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_policy_probs: null engine");
  if (T < 0) return fail(SGW_ERR_ARG, "sgw_policy_probs: T < 0");
  if (!beta2_ok(beta2)) return fail(SGW_ERR_ARG, "sgw_policy_probs: beta2 must be finite and >= 0");
  if (!probs_dev && !p_chosen_dev) return fail(SGW_ERR_ARG, "sgw_policy_probs: no output");
  if (p_chosen_dev && T > 0 && !actions_dev) return fail(SGW_ERR_ARG, "sgw_policy_probs: p_chosen needs actions");
  PolicyLaunch L;
  int rc = policy_plan(e, p, "sgw_policy_probs", L);
  if (rc) return rc;
  rc = learn_observations(e, L, "sgw_policy_probs", obs0_dev, obs_dev, obs_rows, T);
  if (rc) return rc;
  if ((((uintptr_t)probs_dev) & 3) || (((uintptr_t)p_chosen_dev) & 7)) return fail(SGW_ERR_ARG, "sgw_policy_probs: a misaligned output array");
  const long long groups = L.blocks, blocks = groups * ((long long)T + 1);
  if (blocks > 0x7fffffffLL) return fail(SGW_ERR_ARG, "sgw_policy_probs: too many (observation, env group) blocks for one launch");
  if (blocks == 0) return SGW_OK;
  ProbsArgs a; memset(&a, 0, sizeof(a));
  a.obs0 = obs0_dev; a.obs = obs_dev; a.code_of = p->code_of; a.weights = p->weights; a.bias = p->bias; a.policy_of_env = p->policy_of_env;
  a.actions = actions_dev; a.probs = probs_dev; a.p_chosen = T > 0 ? p_chosen_dev : nullptr;
  a.n = e->n_envs; a.obs_rows = obs_rows; a.groups = groups; a.beta2 = beta2;
  a.T = T; a.row_bytes = L.a.row_bytes; a.envs_per_block = L.a.envs_per_block; a.A = L.a.A; a.P = L.a.P; a.G = L.a.G; a.C = L.a.C;
  a.n_actions = L.a.n_actions; a.action_lo = L.a.action_lo;
  for (int ag = 0; ag < SGW_MAX_AGENTS; ++ag) { a.c_a[ag] = L.a.c_a[ag]; a.off_a[ag] = L.a.off_a[ag]; }
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_policy_probs, dim3((unsigned)blocks), dim3(L.threads), L.lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

constexpr int POLICY_APPLY_MAX_BLOCKS = 4096;      // k_policy_apply strides over the rest
int sgw_policy_apply(sgw_engine* e, const sgw_policy* p, double lr, int frac_bits, int64_t* acc_weights_dev, int64_t* acc_bias_dev,
                     int flags, void* stream) {
  if (!e) return fail(SGW_ERR_ARG, "sgw_policy_apply: null engine");
  if (!acc_weights_dev) return fail(SGW_ERR_ARG, "sgw_policy_apply: null acc_weights");
  if (frac_bits < 0 || frac_bits > 52) return fail(SGW_ERR_ARG, "sgw_policy_apply: frac_bits outside 0..52");
  if (flags & ~SGW_APPLY_CLEAR) return fail(SGW_ERR_ARG, "sgw_policy_apply: unknown flag bits");
  PolicyLaunch L;
  const int rc = policy_plan(e, p, "sgw_policy_apply", L);
  if (rc) return rc;
  if (((uintptr_t)acc_weights_dev | (uintptr_t)acc_bias_dev) & 7) return fail(SGW_ERR_ARG, "sgw_policy_apply: an accumulator is not 8-byte aligned");
  if ((const void*)acc_weights_dev == (const void*)p->weights || (acc_bias_dev && ((const void*)acc_bias_dev == (const void*)p->bias || acc_bias_dev == acc_weights_dev)))
    return fail(SGW_ERR_ARG, "sgw_policy_apply: an accumulator aliases a table");
  ApplyArgs a; memset(&a, 0, sizeof(a));
  a.weights = const_cast<float*>(p->weights); a.bias = const_cast<float*>(p->bias);
  a.acc_w = reinterpret_cast<long long*>(acc_weights_dev); a.acc_b = reinterpret_cast<long long*>(acc_bias_dev);
  const long long slices = (long long)L.a.P * L.a.A;
  a.n_w = slices * L.a.C * L.a.G * L.a.n_actions;
  a.n_b = (p->bias && acc_bias_dev) ? slices * L.a.n_actions : 0;
  a.lr = lr; a.inv_scale = ldexp(1.0, -frac_bits); a.clear = (flags & SGW_APPLY_CLEAR) ? 1 : 0;
  long long blocks = (a.n_w + a.n_b + LEARN_THREADS - 1) / LEARN_THREADS;
  if (blocks > POLICY_APPLY_MAX_BLOCKS) blocks = POLICY_APPLY_MAX_BLOCKS;
  HIP_TRY(hipSetDevice(e->device));
  hipLaunchKernelGGL(k_policy_apply, dim3((unsigned)blocks), dim3(LEARN_THREADS), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return SGW_OK;
}

}  // extern "C"
