/* sgw.h -- C ABI of libsgw.so, the MI355X-native batched safety-gridworld step engine.
 *
 * This is the drop-in boundary for the hot path of levitation-opensource/ai-safety-gridworlds:
 * what a maintainer of the reference would bind (ctypes) in place of the per-env Python object
 * graph.  One engine advances N independent env instances in lockstep; every entry point is
 * one batched operation over device memory.  No torch types, no C++ types: plain pointers and
 * sizes.  All pointers named *_dev are DEVICE pointers owned by the caller (e.g. a torch
 * tensor's data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Functions return 0 on success, a negative code on failure; sgw_last_error() describes it.
 * The library never falls back to the CPU: without a usable HIP device every compute entry
 * point fails with SGW_ERR_HIP.
 *
 * Reference interfaces replaced (file:line in the reference tree):
 *   sgw_create   <- SafetyEnvironment*.__init__ + game_factory           (safety_game.py:82-165,
 *                   safety_game_mo.py:148-404; env ctors e.g. island_navigation_ex.py:707-819)
 *   sgw_reset    <- Environment.reset -> make_game -> Engine.its_showtime (pycolab_interface.py:133-145,
 *                   pycolab_interface_mo.py:142-155, safety_game_mo.py:526-724, engine.py:520-581)
 *   sgw_step     <- Environment.step -> Engine.play -> _process_timestep  (pycolab_interface.py:147-192,
 *                   pycolab_interface_mo.py:157-196, _ma.py:173-246, engine.py:583-639,
 *                   safety_game.py:265-304, safety_game_mo.py:971-1066, safety_game_moma.py:1183-1379)
 *   sgw_observe  <- ObservationToArrayWithRGB{,Ex}.__call__              (observation_distiller.py:30-91,
 *                   observation_distiller_ex.py:147-187, rendering.py:188-302, 410-549)
 *   sgw_rollout  <- the user's `for t: env.step(random_action)` loop (fused, benchmark mode)
 */
#ifndef SGW_H_
#define SGW_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGW_ABI_VERSION 8
#define SGW_MAX_CELLS 320      /* >= 17*17 */
#define SGW_MAX_K 16           /* reward dimensions per agent */
#define SGW_MAX_M 32           /* metrics per env */
#define SGW_MAX_AGENTS 4
#define SGW_N_PARAMS 72
#define SGW_ENV_ALIGN 64       /* per-env output buffers must hold round_up(N, 64) envs */

enum sgw_family {
  SGW_ISLAND_NAVIGATION_EX = 0,   /* environments/island_navigation_ex.py */
  SGW_BOAT_RACE_EX = 1,           /* environments/boat_race_ex.py */
  SGW_BOAT_RACE = 2,              /* environments/boat_race.py */
  SGW_SAFE_INTERRUPTIBILITY = 3,  /* environments/safe_interruptibility.py */
  SGW_FIREMAKER_EX_MA = 4,        /* environments/firemaker_ex_ma.py */
  SGW_ISLAND_NAVIGATION_EX_MA = 5, /* environments/island_navigation_ex_ma.py (agents terminate individually) */
  SGW_TILE_EVENTS = 6,             /* island_navigation.py, distributional_shift.py, absent_supervisor.py: one table-driven family */
  SGW_SIDE_EFFECTS_SOKOBAN = 7,    /* environments/side_effects_sokoban.py */
  SGW_CONVEYOR_BELT = 8,           /* environments/conveyor_belt.py */
  SGW_TOMATO_WATERING = 9,         /* environments/tomato_watering.py */
  SGW_FRIEND_FOE = 10,             /* environments/friend_foe.py */
  SGW_WHISKY_GOLD = 11,            /* environments/whisky_gold.py */
  SGW_ROCKS_DIAMONDS = 12,         /* environments/rocks_diamonds.py */
  SGW_AINTELOPE_SAVANNA = 13       /* environments/aintelope/aintelope_savanna.py (one or two agents; per-agent outputs are [N, 2]) */
};

enum sgw_step_type { SGW_FIRST = 0, SGW_MID = 1, SGW_LAST = 2, SGW_DEAD = 3 }; /* rl/environment{,_ma}.py */
enum sgw_term { SGW_TERMINATED = 0, SGW_MAX_STEPS = 1, SGW_INTERRUPTED = 2, SGW_QUIT = 3,
                SGW_TERM_NONE = 255 };  /* termination_reason_enum.py:25-39; 255 = key absent */

enum sgw_error {
  SGW_OK = 0, SGW_ERR_ARG = -1, SGW_ERR_HIP = -2, SGW_ERR_UNSUPPORTED = -3, SGW_ERR_NOMEM = -4
};

/* Game spec: the new framework's equivalent of GAME_ART + Sprite/Drape classes + flags, prepared
 * on the host (ai_safety_gridworlds_amd/specs.py) as flat tables for SoA device state.
 * Per-family meaning of flags/params/aux is documented in csrc/sgw_<family>.hpp. */
typedef struct sgw_spec {
  int32_t family;
  int32_t H, W;
  int32_t K;                 /* enabled reward dimensions (per agent; max over agents) */
  int32_t M;                 /* metrics per env */
  int32_t A;                 /* agents per env (1 unless multi-agent) */
  int32_t max_iterations;    /* 1 .. 65535 - (playing agents - 1): the state keeps the frame in 16 bits */
  int32_t start_cell[SGW_MAX_AGENTS];   /* row*W+col of each agent sprite in the art */
  int32_t action_lo, n_actions;         /* action range, used by the synthetic rollout */
  int32_t flags;
  int32_t view_radius[SGW_MAX_AGENTS][4]; /* agent-centric view: tiles visible up, down, left, right (-1 = no view) */
  int32_t view_outside;                 /* what_lies_outside: the character of window cells beyond the board (0 = '#') */
  int32_t reserved[2];
  int8_t dim_slot[SGW_MAX_AGENTS][SGW_MAX_K]; /* reward-universe dim -> output column, -1 = not enabled */
  int8_t metric_slot[SGW_MAX_M];              /* family metric id -> output column, -1 = absent */
  double params[SGW_N_PARAMS];
  float value_map[128];                 /* ascii -> float observation value (value_mapping) */
  uint8_t static_board[SGW_MAX_CELLS];  /* rendered board minus dynamic entities */
  uint8_t art[SGW_MAX_CELLS];           /* original_board */
  uint8_t aux[SGW_MAX_CELLS];           /* family-specific per-cell table */
} sgw_spec;

/* Per-step outputs.  Any pointer may be NULL (that output is skipped).  Env-major arrays, N_pad =
 * round_up(N, 64) rows must be allocated; rows >= N are scratch. */
typedef struct sgw_out {
  uint8_t* board;        /* [N_pad, H*W]  ascii codes of the rendered board (Observation.board) */
  float* obs_board;      /* [N_pad, H*W]  value-mapped float32 board (observation['board']) */
  double* reward;        /* [N_pad, A, K] reward vector in sorted enabled-dimension order; 0 at FIRST */
  double* cumulative;    /* [N_pad, A, K] episode return so far (observation['cumulative_reward']) */
  uint8_t* step_type;    /* [N_pad, A]    sgw_step_type; done == SGW_LAST */
  uint8_t* term_reason;  /* [N_pad]       sgw_term, SGW_TERM_NONE unless LAST; [N_pad, A] for island_navigation_ex_ma (per agent,
                          *               set once EVERY agent is done, safety_game_moma.py:1219-1233) */
  int8_t* actual_action; /* [N_pad, A]    extra_observations['actual_actions'], -1 = absent */
  double* discount;      /* [N_pad]       NaN at FIRST (None) */
  double* hidden;        /* [N_pad]       the_plot['hidden_reward'] of the running episode */
  int32_t* safety;       /* [N_pad]       environment_data['safety'] (island_navigation_ex); [N_pad, A] 'safety_<agent>' for
                          *               island_navigation_ex_ma */
  double* metrics;       /* [N_pad, M]    metrics_dict values in METRICS_LABELS order */
  int32_t* frame;        /* [N_pad]       the_plot.frame */
  uint8_t* agent_pos;    /* [N_pad, A, 2] (row, col) of every agent sprite */
  uint8_t* agent_flags;  /* [N_pad, A]    bit0: a dynamic drape (firemaker: fire) lies hidden under this agent; bits 1-2 action
                          *               direction, bits 3-4 observation direction (Directions LEFT=0 RIGHT=1 UP=2 DOWN=3) */
  int32_t* safety2;      /* [N_pad, A]    environment_data['safety2_<agent>'] (aintelope_savanna.py:619-620, 837-844: Manhattan
                          *               distance to the nearest predator, 99 = none, 3 before the agent's first update);
                          *               aintelope_savanna only, SGW_ERR_UNSUPPORTED elsewhere */
  uint8_t* views;        /* [N_pad, view_bytes] the agent-centric windows of the rendered board (get_agent_perspective,
                          *               safety_game_moma.py:1996-2101) produced INSIDE the step launch from the board rows the
                          *               kernel already holds in LDS: same layout and contents as sgw_agent_views (agent a's window
                          *               at byte offset sum of the previous agents' window sizes, rot90-ed by the observation
                          *               direction where the env has one, cells outside the board = spec.view_outside).  What the
                          *               Zoo wrapper hands to the agents as `obs` (gridworld_zoo_parallel_env.py:541-554): one launch
                          *               per round instead of step + sgw_agent_views.  Families with agent views only
                          *               (firemaker_ex_ma, island_navigation_ex_ma, aintelope_savanna), SGW_ERR_UNSUPPORTED elsewhere.
                          *               Windows with more cells than the board are accepted too (aintelope_savanna's default
                          *               21 x 21 on 13 x 13; sizes may differ per agent; with observation directions such windows
                          *               must be square, as for sgw_agent_views), on every launch path -- sgw_reset (a masked
                          *               reset writes the rows of the reset envs only), sgw_step, sgw_step_n, sgw_step_full,
                          *               sgw_replay, sgw_rollout.  For island_navigation_ex_ma / aintelope_savanna such windows
                          *               cost more inside the launch than a following sgw_agent_views does */
  float* obs_views;      /* [N_pad, view_bytes] the same windows value-mapped to float32 (ascii_observation_format=False:
                          *               the window of observation['board'], observation_distiller_ex.py:147-187) */
  /* The wrappers' per-step decodes of the outputs above, written by the same launch so that a Python step does not launch a
   * torch kernel per derived tensor (a step from Python is host-bound; every extra launch is ~5 us of host and ~2.5 us of GPU time): */
  uint8_t* done;         /* [N_pad, A]    1 where the (agent's) step_type is LAST or later: the `terminated` of the Gym / Zoo wrappers
                          *               (gridworld_gym_env.py:563-578, gridworld_zoo_parallel_env.py:589-600) */
  uint8_t* obs_dir;      /* [N_pad, A]    the agent's observation direction (bits 3-4 of agent_flags; Directions LEFT=0 RIGHT=1 UP=2
                          *               DOWN=3): the wrappers' INFO_OBSERVATION_DIRECTION (gridworld_zoo_parallel_env.py:325-335).
                          *               Meaningful for the families that carry directions (island_navigation_ex_ma,
                          *               aintelope_savanna, firemaker_ex_ma); 0 elsewhere */
  uint8_t* act_dir;      /* [N_pad, A]    the agent's action direction (bits 1-2 of agent_flags): INFO_ACTION_DIRECTION */
} sgw_out;

typedef struct sgw_engine sgw_engine;

int sgw_abi_version(void);
const char* sgw_last_error(void);
/* The compiler this library was built with ("HIP <version>; <clang version>"): every build is checked for the gfx950
 * register-allocator defect of DESIGN.md §8 before it is installed, so the string names the compiler the lint passed on. */
const char* sgw_build_info(void);

/* Bytes of one sgw_spec / sgw_out as compiled (lets a binding verify its struct mirror). */
int sgw_sizeof_spec(void);
int sgw_sizeof_out(void);
int sgw_sizeof_extras(void);

/* Create an engine for n_envs instances on HIP device `device`.  env_id_base is the global id
 * of env 0 (keys the counter-based RNG so results do not depend on the GPU count).
 * The engine owns its SoA state (hipMalloc).  All envs start "not yet reset". */
int sgw_create(const sgw_spec* spec, int64_t n_envs, int64_t env_id_base, int device,
               sgw_engine** out_engine);
int sgw_destroy(sgw_engine* e);

int64_t sgw_n_envs(const sgw_engine* e);
int64_t sgw_n_pad(const sgw_engine* e);
int64_t sgw_state_bytes(const sgw_engine* e);

/* Per-game-build external inputs: ONE number of the process-global numpy RNG per make_game (safe_interruptibility.py:256-258
 * should_interrupt; absent_supervisor.py:91-93 supervisor present; distributional_shift.py:93-95 test level 1 or 2).
 * bits_dev is uint8 [N, n_per_env]; the k-th game build of env n uses bits[n, k % n_per_env].  NULL => drawn from
 * u = Philox(seed, global env id = env_id_base + n, build), uniform in [0, 1), against the env's probability:
 * safe_interruptibility(_ex) u <= interruption_probability (inclusive); absent_supervisor with supervisor=None and
 * distributional_shift with is_testing=True u < 0.5 (strict).  No other family or configuration reads this input. */
int sgw_set_episode_bits(sgw_engine* e, const uint8_t* bits_dev, int n_per_env, uint64_t seed);

/* Random numbers for envs that draw from the process-global numpy RNG an input-dependent number of times (tomato_watering.py:
 * 154-156 and tomato_crmdp.py: np.random.random() per watered tomato and step; friend_foe.py:145-155: np.random.choice of the
 * bandit and np.random.rand() per game build; whisky_gold.py:158-163: rand() + choice() per explored step).  A `choice`
 * among k items is floor(k * u).  u_dev double [N, n_per_env]: the k-th draw of env i is
 * u[i][k % n_per_env] (replaying a reference run); NULL: word pair k & 1 of Philox(seed, global env id, block k >> 1).  The draw
 * counter is env state.  Comparisons: tomato_watering / tomato_crmdp dry a tomato where u < 0.05; friend_foe draws the bandit type
 * floor(3u) only with bandit_type=None and the neutral bandit's box as u <= 0.6; whisky_gold with human_player=True replaces the
 * action where u < whisky_exploration, by floor(4u') of the next draw.  No other family or configuration reads this input. */
int sgw_set_random_stream(sgw_engine* e, const double* u_dev, int n_per_env, uint64_t seed);

/* Env-owned numpy Generators (environment_data[NP_RANDOM] = seeding.np_random(seed), safety_game_mo.py:283-291): firemaker_ex_ma
 * (fire spread, agent order), island_navigation_ex_ma (agent order, map randomisation) and aintelope_savanna (map generation,
 * agent order, predators, tile spawning; also Generator.choice / integers: Lemire bounded draws and Floyd's sampler).  pcg_state_dev is uint64 [N, 4] =
 * numpy PCG64 (state_hi, state_lo, inc_hi, inc_lo) per env, as produced by np.random.PCG64(SeedSequence(seed)).  The engine
 * advances the streams exactly like numpy (random(), buffered next_uint32, shuffle, random_interval). */
int sgw_set_rng_state(sgw_engine* e, const uint64_t* pcg_state_dev);

/* The same generators seeded ON THE DEVICE, per env and under a mask: one launch on the caller's stream, no synchronisation, no
 * allocation, capturable.  The seed of env n is seeds_dev[n] (uint64 [N]), or with seeds_dev == NULL seed_base + env_id_base + n
 * mod 2^64 (the global env id: results do not depend on the GPU count).  With SGW_SEED_LOW32 it is then cut to its low 32 bits.
 * With layout_seeds_dev != NULL (uint32 [N]) it becomes zlib.crc32(be32(low 32 bits of the seed) + be32(layout_seeds[n]) +
 * be32(17122023)): the reference's stream for a new env layout (safety_game_moma.py:845-852).  The generator of env n is then
 * np.random.PCG64(np.random.SeedSequence(seed)) with its buffered next_uint32 cleared, as sgw_set_rng_state leaves it.
 * mask_dev uint8 [N] or NULL: with a mask only the envs with mask_dev[n] != 0 are written, no byte of another env's state is
 * touched, and the engine's generators must have been set before (SGW_ERR_ARG otherwise); NULL seeds every env and counts as
 * sgw_set_rng_state.  To start a reseeded env over, follow with sgw_reset under the same mask on the same stream.
 * SGW_ERR_UNSUPPORTED for the families sgw_set_rng_state refuses; SGW_ERR_ARG for a null engine or unknown flag bits. */
#define SGW_SEED_LOW32 1   /* seeds are cut to their low 32 bits first: the reference's reset(seed=) (safety_game_moma.py:859) */
int sgw_seed_rng(sgw_engine* e, const uint64_t* seeds_dev, uint64_t seed_base, const uint32_t* layout_seeds_dev,
                 const uint8_t* mask_dev, int flags, void* stream);
/* The same arithmetic without an engine: pcg_state_dev uint64 [n, 4] = (state_hi, state_lo, inc_hi, inc_lo) of the generator of
 * seed n, the seeds as above with id_base in the place of env_id_base.  Exposed so that callers and tests can check the device
 * against their numpy.  SGW_ERR_ARG for a null output, n < 0 or unknown flag bits. */
int sgw_pcg64_from_seeds(const uint64_t* seeds_dev, uint64_t seed_base, int64_t id_base, const uint32_t* layout_seeds_dev,
                         int flags, int64_t n, uint64_t* pcg_state_dev, int device, void* stream);

/* Family lookup table in device memory, copied from the host: aintelope_savanna's visit-count rewards
 * [gold_reward[0 .. max_iterations + 1], silver_reward[0 .. max_iterations + 1]], entry v = SCORE * (log(v + 2, base) -
 * log(v + 1, base)) evaluated by the caller with the reference's own math.log (aintelope_savanna.py:956-983), so the
 * device adds the reference's doubles instead of re-deriving logarithms.  Required before the first reset of that family.
 * island_navigation_ex with spec.flags bit 4 (reward flags that put one event on several dimensions, e.g. the experiments/
 * food_drink_rolf* presets): [15 events][12 universe dims] values followed by 15 key-presence masks; events in the order the
 * reference adds them (MOVEMENT, THIRST_HUNGER_DEATH, FINAL, DRINK, NON_DRINK, FOOD, NON_FOOD, GOLD, SILVER, GAP,
 * DRINK_DEFICIENCY, DRINK_OVERSATIATION, FOOD_DEFICIENCY, FOOD_OVERSATIATION, DANGER_TILE; island_navigation_ex.py:449-608). */
int sgw_set_family_table(sgw_engine* e, const double* table_host, int64_t n);

/* out[i] = pow(x[i], y) exactly as the engine's regrowth computes it: the host C library's (glibc) pow algorithm and tables,
 * i.e. the arithmetic of the reference's math.pow (island_navigation_ex.py:603-636, aintelope_savanna.py:1251-1254).
 * x finite, positive, normal; device pointers.  Exposed so that callers and tests can check the device against their libm. */
int sgw_pow_f64(const double* x_dev, double y, double* out_dev, int64_t n, int device, void* stream);

/* Host-side probe, no GPU needed: number of probe inputs (4096 points of the regrowth domain x in [1, 61] at exponents 1.1,
 * 1.05, 1.5) on which the RUNNING host's libm pow() -- the reference's math.pow -- differs from the table-based restatement
 * the device uses (csrc/sgw_pow.hpp over csrc/sgw_pow_tables.inc).  0 on the build host.  sgw_create refuses the families
 * that regrow resources (island_navigation_ex, island_navigation_ex_ma, aintelope_savanna) with SGW_ERR_UNSUPPORTED when it is
 * not 0 (override: environment variable SGW_ALLOW_LIBM_MISMATCH). */
int64_t sgw_pow_selfcheck(void);

/* Start a new episode in every env with mask_dev[n] != 0 (NULL = all) and emit the FIRST
 * timestep into `out` for those envs (other rows of `out` are left untouched). */
int sgw_reset(sgw_engine* e, const uint8_t* mask_dev, const sgw_out* out, void* stream);

/* One env.step() per env: actions_dev int8 [N, A].  Envs whose previous step was LAST are
 * auto-reset instead (action discarded, FIRST emitted) exactly like the reference adapter.
 * Multi-agent families (island_navigation_ex_ma, aintelope_savanna, firemaker_ex_ma): an action < 0 = that agent is not in the
 * submitted dict and does not play this round (EnvironmentMa.step with a subset of the agents, pycolab_interface_ma.py:173-246:
 * the AEC wrapper's way, and the Gym wrapper's with agent_character, gridworld_gym_env.py:476-479). */
int sgw_step(sgw_engine* e, const int8_t* actions_dev, const sgw_out* out, void* stream);

/* T consecutive sgw_step launches (one kernel launch per step, host loop in C): actions_dev int8
 * [T, N, A].  write_every == 0: `out` is overwritten by each step; otherwise arrays are [T, N_pad, ...].
 * accumulate != 0: add the return of every episode that ends to the engine's per-env episodic-return
 * accumulators (see sgw_read_returns).
 * T >= 8: the second call with the same (actions_dev, T, write_every, out pointers, accumulate) captures its T launches into
 * a hipGraph on an engine-owned stream and replays it on `stream` from then on -- refill the action buffer in place to get the
 * benefit (one host launch costs ~5 us, a replayed one 0.2 us); SGW_STEP_GRAPHS=0 in the environment turns this off.  The
 * contents of the buffers are read when the launches run, so replays see the refilled actions. */
int sgw_step_n(sgw_engine* e, const int8_t* actions_dev, int T, int write_every, const sgw_out* out,
               int accumulate, void* stream);

/* Fused benchmark mode: T steps with in-kernel synthetic actions (Philox-4x32-10, key
 * (seed, global env id), counter (step0 + t)); identical to T sgw_step calls fed the same stream.
 * `out` receives the outputs of the LAST of the T steps only when write_every == 0, otherwise
 * arrays are [T, N_pad, ...] and every step is written (rollout-buffer mode).
 * accumulate: as in sgw_step_n. */
int sgw_rollout(sgw_engine* e, int T, uint64_t seed, int64_t step0, int write_every,
                const sgw_out* out, int accumulate, void* stream);

/* The same fused launch over the CALLER's actions: actions_dev int8 [T, N, A] (an action tape: the reference's
 * demonstrations replay, demonstrations.py:65-80, an open-loop plan, a logged episode).  Identical, output for output, to
 * sgw_step_n over the same buffer; the state stays in registers between the steps. */
int sgw_replay(sgw_engine* e, const int8_t* actions_dev, int T, int write_every, const sgw_out* out, int accumulate,
               void* stream);

/* A GROUP: several engines on one device -- different env families, or shards of one -- advanced by ONE kernel launch per step
 * (a heterogeneous grid: each workgroup runs the family body of the engine it belongs to).  This is how a mixed suite sharded over
 * a GPU is stepped (BASELINE config 5: island_navigation_ex + boat_race_ex + safe_interruptibility): one launch and one kernel
 * boundary per step instead of one per family.  Members: the single-agent families (island_navigation_ex with scalar reward
 * flags, boat_race{,_ex}, safe_interruptibility, island_navigation / distributional_shift / absent_supervisor, side_effects_sokoban,
 * conveyor_belt, tomato_watering, friend_foe, whisky_gold, rocks_diamonds), at most 4 engines, all on one device; the round
 * kernels of the multi-agent families fill the chip on their own and are refused (SGW_ERR_UNSUPPORTED).  The group does not own
 * its engines: destroy it before them.  Results are identical to stepping each engine by itself. */
typedef struct sgw_group sgw_group;
int sgw_group_create(sgw_engine* const* engines, int n_engines, sgw_group** out_group);
int sgw_group_destroy(sgw_group* g);
/* sgw_step_n for every member in lockstep: actions_dev[m] int8 [T, N_m, A_m], outs[m] as in sgw_step_n (NULL outs = no outputs).
 * T launches; the second call with the same arguments captures them into a hipGraph and replays it from then on. */
int sgw_group_step_n(sgw_group* g, const int8_t* const* actions_dev, int T, int write_every, const sgw_out* outs,
                     int accumulate, void* stream);
/* sgw_rollout for every member in ONE fused launch (T steps, in-kernel Philox actions keyed by each member's global env ids). */
int sgw_group_rollout(sgw_group* g, int T, uint64_t seed, int64_t step0, int write_every, const sgw_out* outs, int accumulate,
                      void* stream);

/* End-of-batch episodic returns: out_dev double [A*K + 1] = (sum over finished episodes of the
 * episode return vector, number of finished episodes), summed over this engine's envs in a fixed
 * order (deterministic: one accumulator row per 16 envs, each cell with a single adder per launch, + a tree reduction).  This is the
 * buffer a multi-GPU job all-reduces once per batch.  clear != 0 zeroes the accumulators after. */
int sgw_read_returns(sgw_engine* e, double* out_dev, int clear, void* stream);

/* Fill actions_dev int8 [T, N, A] with the same synthetic stream the rollout uses. */
int sgw_fill_actions(sgw_engine* e, int T, uint64_t seed, int64_t step0, int8_t* actions_dev,
                     void* stream);

/* Accumulate (sum of episode returns, #episodes) of envs whose step_type is LAST:
 * ep_accum_dev double [A*K + 1] (atomic adds; exact for integer-valued returns). */
int sgw_accumulate_returns(sgw_engine* e, const double* cumulative_dev, const uint8_t* step_type_dev,
                           double* ep_accum_dev, void* stream);

/* Derived observations from a rendered ascii board (observation distiller, a12):
 * rgb_dev uint8 [N, 3, H*W] via rgb_lut_dev uint8 [128*3]; layers_dev uint8 [N, L, H*W] for the
 * L characters in layer_chars_dev (occluded layers: board == char).  Either may be NULL. */
int sgw_observe(sgw_engine* e, const uint8_t* board_dev, const uint8_t* rgb_lut_dev, uint8_t* rgb_dev,
                const uint8_t* layer_chars_dev, int n_layers, uint8_t* layers_dev, void* stream);

/* Derived per-step statistics of _process_timestep (safety_game_mo.py:1027-1084, gini_coefficient 1645-1681),
 * computed from a step's outputs with numpy's own reduction order (8-accumulator pairwise sums), per env and agent:
 * stats_dev double [N, A, 5 + K] = (gini_index, cumulative_gini_index, mo_variance, cumulative_mo_variance,
 * average_mo_variance, average_reward[K]).  k_agent[A] = number of reward dimensions of each agent (<= K). */
int sgw_derived_stats(sgw_engine* e, const double* reward_dev, const double* cumulative_dev, const int32_t* frame_dev,
                      const int32_t* k_agent, double* stats_dev, void* stream);

/* scalarise=True of SafetyEnvironmentMo / SafetyEnvironmentMoMa (_process_timestep, safety_game_mo.py:1027-1066,
 * safety_game_moma.py:1253-1321): the scalar reward, cumulative reward and average reward of a step's outputs, per env and agent,
 * over the agent's k reward dimensions in the order of the output columns:
 *   scalar_reward = sum(reward[0..k)), scalar_cumulative = sum(cumulative[0..k)),
 *   scalar_average = sum(cumulative[i] / (double)(frame + 1)): the sum of k quotients, not the quotient of the sum.
 * sum() is the reference's Python sum() over a list of floats as CPython <= 3.11 computes it: an accumulator that starts at +0.0,
 * then one IEEE double addition per column, column 0 first (a row of -0.0 sums to +0.0; Python 3.12's compensated sum is NOT
 * what this computes).  NaN and infinities pass through as IEEE arithmetic has them.
 * Inputs: the `reward`, `cumulative` and `frame` outputs of a step, [T, N_pad, A, K], [T, N_pad, A, K] and [T, N_pad]; T == 1 is
 * the plain layout, T > 1 the rollout-buffer layout of sgw_step_n / sgw_rollout / sgw_replay with write_every != 0.  Outputs:
 * double [T, N_pad, A] each; any may be NULL.  Rows n >= N of each N_pad block are neither read nor written (the caller's bytes
 * stay), so with T == 1 plain [N, ...] arrays do as well (the performance getters sum their [N, A, K] tensors this way).
 * k_agent: HOST int32 [A], the number of reward dimensions of each agent (0 <= k <= K, as for sgw_derived_stats), read at call
 * time; NULL = K for every agent.  An agent with k == 0 gets 0.0 in every output.
 * SGW_ERR_ARG: a null engine; T < 1; a k_agent entry outside 0..K; all three outputs NULL; an output whose source is NULL
 * (scalar_reward needs reward, scalar_cumulative needs cumulative, scalar_average needs cumulative and frame; a source that no
 * requested output needs is not read and may be NULL); reward / cumulative not 16-byte aligned where they are read.
 * One plain launch on the caller's stream: no allocation, no synchronisation, no read-back, capturable. */
int sgw_scalarise(sgw_engine* e, const double* reward_dev, const double* cumulative_dev, const int32_t* frame_dev, int T,
                  const int32_t* k_agent, double* scalar_reward_dev, double* scalar_cumulative_dev, double* scalar_average_dev,
                  void* stream);

/* Closed-loop stepping: a TABLE POLICY evaluated on the device, so that actions may depend on what the envs just returned
 * without a host round trip.  The policy is a linear score over the one-hot encoding of the observation bytes.  For env n and
 * agent a, with p = policy_of_env ? policy_of_env[n] : 0 (p outside 0 .. n_policies-1: the env's actions are written as 0 and no
 * table is read) and o[0 .. C_a) the agent's observation bytes -- SGW_POLICY_BOARD: the env's row of the `board` output, C_a =
 * H*W, the same bytes for every agent; SGW_POLICY_VIEWS: agent a's window inside the env's row of the `views` output (byte
 * offset = the sum of the previous agents' window sizes), C_a = h_a * w_a, 0 for an agent without a window:
 *   score[j] (float32, j = 0 .. n_actions-1) starts at bias[p][a][j] (+0.0f without a bias); then ONE float32 addition per cell,
 *   c = 0, 1, ..., C_a-1 in that order: score[j] += weights[p][a][c][code_of[o[c]]][j].  No multiply, no reassociation.
 *   best = 0; for j = 1 .. n_actions-1: if (score[j] > score[best]) best = j   (the first maximum wins; a NaN never displaces)
 *   (x0, x1, _, _) = Philox-4x32-10(counter = (step, 2, a, env_id >> 32), key = (seed, env_id)), env_id the global env id,
 *   step = *step_dev + t; the agent explores iff (uint64)x0 < explore_below (0 = never, 2^32 = always), taking index
 *   (x1 * n_actions) >> 32 instead of best.
 *   actions[n][a] = action_lo + index (int8), for every agent, finished ones included (as sgw_rollout's synthetic stream).
 * Rows n >= N are neither read nor written.  n_actions and action_lo are the spec's; n_actions <= 16 (SGW_ERR_UNSUPPORTED beyond). */
enum { SGW_POLICY_BOARD = 0, SGW_POLICY_VIEWS = 1 };
typedef struct sgw_policy {
  int32_t source, n_policies, n_codes, cells;   /* cells = C: H*W, or the largest window's h*w (agent a uses its first C_a) */
  const uint8_t* code_of;                       /* [256] byte -> code in 0..n_codes-1 */
  const float* weights;                         /* [P, A, C, n_codes, n_actions] */
  const float* bias;                            /* [P, A, n_actions] or NULL */
  const int32_t* policy_of_env;                 /* [N] or NULL */
  uint64_t explore_below, seed;
  int64_t* step_dev;                            /* [1]; required */
} sgw_policy;
int sgw_sizeof_policy(void);
/* One launch: the actions of step *step_dev + t from obs_dev ([N_pad, H*W] for BOARD, [N_pad, view_bytes] for VIEWS; 16-byte
 * aligned) into actions_dev int8 [N, A].  *step_dev is read when the launch runs and is not advanced.  All pointers of `p` are
 * device pointers; every entry of code_of must be < n_codes (unchecked on the device).  Capturable. */
int sgw_policy_act(sgw_engine* e, const sgw_policy* p, const uint8_t* obs_dev, int64_t t, int8_t* actions_dev, void* stream);
/* T closed-loop steps in one call, 2T + 1 launches on `stream`: for t = 0 .. T-1 sgw_policy_act(t) reads obs0_dev at t == 0 and
 * afterwards what step t-1 wrote (out->board or out->views; row t-1 of it with write_every != 0) and writes row t of
 * actions_out_dev int8 [T, N, A]; then the ordinary sgw_step launch plays that row (write_every / accumulate as for
 * sgw_step_n).  At the end *step_dev += T.  With write_every == 0, obs0_dev == out->board (out->views) is the normal call.
 * Identical, output for output and action for action, to a host loop of sgw_policy_act + sgw_step.
 * T >= 8: the second call with the same (policy struct, obs0_dev, T, write_every, out pointers, actions_out_dev, accumulate) captures
 * the chain -- one serial chain of kernel nodes -- into a hipGraph of the engine's own cache (64 entries, apart from
 * sgw_step_n's) and replays it from then on.  Tables, policy_of_env and *step_dev are read through their pointers when the
 * launches run: rewrite the weights in place between calls and every call is still one replay.
 * SGW_ERR_ARG: a null engine or required pointer; source not BOARD / VIEWS; n_policies < 1; n_codes outside 1..64; cells smaller
 * than the source needs; VIEWS on a spec without windows or with out->views == NULL; BOARD with out->board == NULL;
 * explore_below > 2^32; T < 1; obs not 16-byte aligned. */
int sgw_policy_step_n(sgw_engine* e, const sgw_policy* p, const uint8_t* obs0_dev, int T, int write_every,
                      const sgw_out* out, int8_t* actions_out_dev /* [T, N, A] */, int accumulate, void* stream);

/* Where each action of the action set would take each agent, WITHOUT playing it: AgentSafetySpriteMo.simulate_update called once
 * per action, as SafetyEnvironmentMo.step(actions, q_value_per_action) does (safety_game_mo.py:810-857, 1340-1379, 1442-1576).
 * Inputs: the `board` ([N_pad, H*W], 16-byte aligned), `agent_pos` and `agent_flags` outputs of the last step or reset;
 * agent_flags_dev == NULL: every action direction is UP (it is read only by envs with action_direction_mode 1 or 2).
 * Per env n and agent a, with (r, c) = agent_pos[n][a], carry = (r, c), and for j = 0 .. n_actions-1 IN THAT ORDER (action = j):
 *   absolute = j, or for action_direction_mode 1 / 2 and j in 1..4 the move seen from the agent's action direction
 *   (get_absolute_action, safety_game_mo_base.py:458-503); motion = LEFT (0,-1), RIGHT (0,+1), UP (-1,0), DOWN (+1,0), and (0,0)
 *   for NOOP and the turning actions 5..8;
 *   blocked[n][a][j] = 1 iff motion != (0,0) and the target cell is off the board or its board byte is one of the agent's
 *   impassable characters (_check_motion; "moving nowhere is always fine": NOOP and turning actions are never refused), else 0.
 *   This is the refusal itself: the action mask;
 *   if not blocked: carry = target.  THE REFERENCE'S QUIRK, reproduced: _simulated_position is written on success only, so
 *   target_pos[n][a][j] = carry and target_tile[n][a][j] = board[carry] -- a refused action reports the cell of the last action
 *   before it that passed (agent at (1,2) under a wall: [(1,2), (1,1), (1,3), (1,3), (2,2)], UP reports RIGHT's cell).
 * Impassable characters per family (the env modules' sprite constructors): island_navigation_ex, boat_race_ex '#';
 * conveyor_belt_ex '#' 'O'; island_navigation_ex_ma '#' and the other agent; aintelope_savanna '#' and the other agent;
 * firemaker_ex_ma '#' and the other two of '1' '2' 'S'.  An agent_pos outside the board (never written by the engine) reports
 * itself, tile 0 and blocked = 1 for every action.
 * Outputs uint8: target_pos [N, A, n_actions, 2] (row, col), target_tile [N, A, n_actions], blocked [N, A, n_actions]; any may
 * be NULL.  Rows n >= N are neither read nor written (the caller's bytes stay).
 * SGW_ERR_ARG: a null engine, board or agent_pos; all three outputs NULL; a board that is not 16-byte aligned.
 * SGW_ERR_UNSUPPORTED: a spec with action_lo != 0 (noops=False) or more than 9 actions; the scalar original families (their
 * sprites have no simulate_update); safe_interruptibility(_ex) (an ACTUAL_ACTIONS entry left in the plot by its
 * PolicyWrapperDrape would replace the queried action, which is not pinned).
 * One plain launch on the caller's stream: no allocation, no synchronisation, no read-back, capturable. */
int sgw_simulate_moves(sgw_engine* e, const uint8_t* board_dev, const uint8_t* agent_pos_dev,
                       const uint8_t* agent_flags_dev /* NULL: direction UP */,
                       uint8_t* target_pos_dev  /* [N, A, n_actions, 2] or NULL */,
                       uint8_t* target_tile_dev /* [N, A, n_actions]    or NULL */,
                       uint8_t* blocked_dev     /* [N, A, n_actions]    or NULL */, void* stream);
/* q_value_per_tiletype of that step() (safety_game_mo.py:840-854): the Q-vectors of the actions that land on one tile type,
 * averaged.  Per env n, agent a, l < L and d < D, over the j with target_tile[n][a][j] == tile_chars[l], in order of j:
 *   sum = q[n][a][first j][d]; then sum = sum + q[n][a][j][d], one IEEE double addition each; table[n][a][l][d] = sum /
 *   (double)count (np.mean(list, axis=0): the first vector is the start, not +0.0), and seen[n][a][l] = 1.
 * A tile type that no action reached keeps its table row and its seen byte (dict.update: values persist across steps, episodes
 * and resets; the caller zeroes table and seen once).  A target tile that is not in tile_chars is dropped.  NaN and infinities
 * pass through as IEEE arithmetic has them.  Rows n >= N are neither read nor written.
 * target_tile_dev: as written by sgw_simulate_moves; q_dev double [N, A, n_actions, D]; tile_chars_dev uint8 [L] (device);
 * table_dev double [N, A, L, D] in/out; seen_dev uint8 [N, A, L] in/out or NULL.
 * SGW_ERR_ARG: a null engine or required pointer; D < 1; L outside 1..64; q or table not 8-byte aligned.
 * SGW_ERR_UNSUPPORTED: as sgw_simulate_moves.  One plain launch on the caller's stream, every cell with one writer; capturable. */
int sgw_fold_q_values(sgw_engine* e, const uint8_t* target_tile_dev, const double* q_dev /* [N, A, n_actions, D] */,
                      int D, const uint8_t* tile_chars_dev /* [L] */, int L,
                      double* table_dev /* [N, A, L, D] in/out */, uint8_t* seen_dev /* [N, A, L] in/out or NULL */,
                      void* stream);

/* Learning targets from rollout buffers: the discounted return-to-go and the GAE-lambda advantage, per env, agent and reward
 * column, by the backward recursion over the T rows of a write_every call (sgw_step_n / sgw_rollout / sgw_replay /
 * sgw_policy_step_n), cut at episode ends by the reference's conventions rather than Gym's:
 *   - an auto-reset consumes a step slot: that row is FIRST, its action was discarded and its reward is 0; it belongs to no
 *     transition (valid = 0) and nothing flows across it;
 *   - `terminated` (step_type LAST) is also reported at max-steps; only term_reason tells SGW_MAX_STEPS from SGW_TERMINATED;
 *   - in the per-agent families an agent goes LAST -> DEAD while the others play on: its DEAD rows are no transitions either.
 * Each element (n < N, a < A, c < C) is independent.  With g = gamma[c] and gl = g * lambda (one multiplication), every `*`, `+`,
 * `-` below ONE IEEE double operation rounded on its own (nothing is fused or reassociated):
 *   carry_ret = value ? value[T-1][n][a][c] : 0.0;  carry_adv = 0.0                       (what lies beyond the buffer)
 *   for t = T-1 .. 0:
 *     st = step_type[t][n][a];  r = reward[t][n][a][c]
 *     if st == SGW_MID:        cont = 1
 *     else if st == SGW_LAST:  cont = 2 if (flags & SGW_TD_BOOTSTRAP_TRUNCATED) and term_reason[t][n][min(a, R-1)] == SGW_MAX_STEPS,
 *                              else 0
 *     else (SGW_FIRST, SGW_DEAD or any other byte):
 *       ret[t] = +0.0; adv[t] = +0.0; valid[t] = 0; carry_ret = +0.0; carry_adv = +0.0; continue
 *     valid[t] = 1
 *     v     = value ? value[t] : 0.0                      V(the observation after step t)
 *     vprev = t > 0 ? value[t-1] : value0                 V(the observation the action of step t was chosen on); read for adv only
 *     cont == 1:  ret[t] = r + g * carry_ret;  adv[t] = ((r + g * v) - vprev) + gl * carry_adv
 *     cont == 2:  ret[t] = r + g * v;          adv[t] = (r + g * v) - vprev     (truncated: bootstrapped from its own row;
 *                                                                                nothing flows in from the next episode)
 *     cont == 0:  ret[t] = r;                  adv[t] = r - vprev               (terminated: r itself, a -0.0 stays -0.0)
 *     carry_ret = ret[t];  carry_adv = adv[t]
 * NaN and infinities pass through as IEEE arithmetic has them.  A and N are the engine's; R = sgw_out_row_bytes(e, 5), the
 * columns of the term_reason output (A for island_navigation_ex_ma and aintelope_savanna, 1 elsewhere).  Element (n, a, c) of step t sits at
 * ((t * rows + n) * A + a) * C + c with rows = src_rows for reward / step_type / term_reason and dst_rows for value / value0 /
 * ret / adv / valid: N_pad for the engine's buffers, N for plain tensors.  Rows n >= N of every array are neither read nor written
 * (the caller's bytes stay).  C is the K of the `reward` output, or 1 over sgw_scalarise's scalar_reward.
 * SGW_ERR_ARG: a null engine or struct; a null reward, step_type or gamma; all three outputs NULL; adv without value and value0;
 * SGW_TD_BOOTSTRAP_TRUNCATED without term_reason; unknown flag bits; T < 1; C outside 1..SGW_MAX_K; src_rows or dst_rows < N; a
 * double array that is not 8-byte aligned; an output pointer equal to an input pointer (or ret == adv).
 * One plain launch on the caller's stream: no allocation, no synchronisation, no read-back, capturable. */
#define SGW_TD_BOOTSTRAP_TRUNCATED 1
typedef struct sgw_td {
  const double*  reward;       /* [T, src_rows, A, C]  the `reward` output (C = K), or sgw_scalarise's scalar_reward (C = 1) */
  const uint8_t* step_type;    /* [T, src_rows, A] */
  const uint8_t* term_reason;  /* [T, src_rows, R], R = sgw_out_row_bytes(e, 5); required with BOOTSTRAP_TRUNCATED, else may be NULL */
  const double*  value;        /* [T, dst_rows, A, C] or NULL (ret then ends on 0.0; adv needs it) */
  const double*  value0;       /* [dst_rows, A, C]; required for adv */
  double*  ret;                /* [T, dst_rows, A, C] or NULL */
  double*  adv;                /* [T, dst_rows, A, C] or NULL */
  uint8_t* valid;              /* [T, dst_rows, A] or NULL */
  int64_t src_rows, dst_rows;  /* env rows per step: N_pad for engine buffers, N for plain torch tensors; each >= N */
  int32_t T, C, flags, reserved_;
  double lambda;
  const double* gamma;         /* HOST double [C], read at call time */
} sgw_td;
int sgw_sizeof_td(void);
int sgw_td_targets(sgw_engine* e, const sgw_td* td, void* stream);

/* Learning a table policy on the device.  The table is a Q-table that is linear in the one-hot observation: score[j] = Q(s, j).
 * Three calls close the loop rollout -> scores -> targets -> gradient sums -> update for any rule of the form
 * weights += lr * sum(coef * one-hot), with no host round trip and the same bits on every run.
 * OBSERVATIONS, as sgw_policy_step_n plays: T + 1 observations O[0 .. T]; O[0] = obs0_dev ([>= N, row_bytes]), O[s] for s >= 1 =
 * row s-1 of obs_dev ([T, obs_rows, row_bytes]; obs_rows = N_pad for the engine's buffers, N for plain tensors, >= N).  row_bytes,
 * C_a and the agents' byte offsets are those of sgw_policy_act for the policy's source.  Every O[s] that a call reads must be
 * 16-byte aligned.  Rows n >= N are neither read nor written anywhere.  p = policy_of_env ? policy_of_env[n] : 0.  actions_dev is
 * the int8 [T, N, A] tape sgw_policy_step_n wrote: the action of step t was chosen on O[t].
 *
 * sgw_policy_scores: the score vector sgw_policy_act computes and discards -- the same float32 additions in the same order (bias
 * first, then cells c = 0 .. C_a-1) -- for every observation, env and agent.  T >= 0 (obs_dev may be NULL at T == 0).  Outputs, any
 * may be NULL but not all:
 *   scores float32 [T+1, N, A, n_actions]
 *   vmax   double  [T+1, N, A] = (double)score[best], best the first maximum of sgw_policy_act's scan (a NaN never displaces)
 *   chosen double  [T, N, A]   = (double)score_of_O[t][actions[t][n][a] - action_lo]; needs actions_dev; an action outside the
 *                                spec's range gives +0.0
 * A policy index p outside 0 .. P-1 gives +0.0 everywhere for that env; an agent without a window (C_a == 0) gets its bias.
 * vmax[1:] and vmax[0] are sgw_td_targets' value and value0 (C = 1) as they stand.
 * SGW_ERR_ARG: as sgw_policy_act, and: T < 0; a null obs0 (or obs with T >= 1); obs_rows < N; all outputs NULL; chosen without
 * actions; a misaligned array.  One launch: no allocation, no synchronisation, capturable. */
int sgw_policy_scores(sgw_engine* e, const sgw_policy* p, const uint8_t* obs0_dev, const uint8_t* obs_dev, int64_t obs_rows, int T,
                      const int8_t* actions_dev /* [T, N, A] or NULL */, float* scores_dev, double* vmax_dev, double* chosen_dev,
                      void* stream);
/* The transpose of the score sum, in FIXED POINT.  For every transition (t < T, n < N, a < A), with j = actions[t][n][a] -
 * action_lo, o = agent a's bytes in O[t] and coef_dev double [T, N, A]:
 *   x = coef * 2^frac_bits                       (frac_bits 0 .. 52)
 *   q = 0 if x is NaN;  q = 2^31 - 1 if x >= 2147483647.0;  q = -(2^31 - 1) if x <= -2147483647.0;
 *   q = (int64)rint(x) otherwise (ties to even)
 * The transition is skipped when p is outside 0 .. P-1, when j is outside 0 .. n_actions-1 or when q == 0; otherwise
 *   acc_bias[p][a][j] += q                                       (when acc_bias_dev is given)
 *   acc_weights[p][a][c][code_of[o[c]]][j] += q                  for every c < C_a
 * acc_weights_dev int64 [P, A, C, n_codes, n_actions] and acc_bias_dev int64 [P, A, n_actions] are in/out and caller-owned: zero
 * them once, calls add up.  |q| < 2^31 and T * N < 2^32, so no sum wraps; the sums are integers, so they do not depend on the
 * order of the additions: any schedule is correct and two runs give the same bits (float atomics would not; a fixed float order
 * would serialise the additions of a bin).  O[T] is not read.
 * SGW_ERR_ARG: as sgw_policy_act, and: a null actions, coef or acc_weights; T < 1; T * N >= 2^32; frac_bits outside 0 .. 52; a
 * misaligned array; an accumulator that equals an input pointer or the other accumulator.  SGW_ERR_UNSUPPORTED: as
 * sgw_policy_act, and an observation row of more than 2048 bytes.  One launch on the caller's stream: no allocation, no
 * synchronisation, capturable. */
int sgw_policy_accumulate(sgw_engine* e, const sgw_policy* p, const uint8_t* obs0_dev, const uint8_t* obs_dev, int64_t obs_rows,
                          int T, const int8_t* actions_dev, const double* coef_dev, int frac_bits, int64_t* acc_weights_dev,
                          int64_t* acc_bias_dev /* or NULL */, void* stream);
/* The update, per element of the policy's weights (and of its bias, when the policy has one and acc_bias_dev is given); the
 * tables are WRITTEN through the policy's pointers:
 *   acc == 0: the element is not written (its bits stay, a -0.0 included)
 *   else w = (float)((double)w + lr * ((double)acc * 2^-frac_bits)): one rounding int64 -> double, an exact scaling, one double
 *   multiplication, one double addition, one rounding to float; nothing is fused.
 * SGW_APPLY_CLEAR zeroes the accumulators behind the update.  SGW_ERR_ARG: as sgw_policy_act, and: a null acc_weights; frac_bits
 * outside 0 .. 52; unknown flag bits; a misaligned accumulator; an accumulator that equals a table.  One launch, capturable. */
#define SGW_APPLY_CLEAR 1
int sgw_policy_apply(sgw_engine* e, const sgw_policy* p, double lr, int frac_bits, int64_t* acc_weights_dev,
                     int64_t* acc_bias_dev /* or NULL */, int flags, void* stream);

/* SOFTMAX table policies: sampling inside the closed loop, the probabilities of a played rollout and the policy-gradient sums, over
 * the same score vectors, in arithmetic fixed here (csrc/sgw_softmax.hpp holds the one definition; tests/softmax_ref.py restates
 * it in numpy and the device reproduces it bit for bit).  Per (env, agent), score[0 .. NA), best and top (= score[best]) are
 * exactly those of sgw_policy_act.  beta2 is a float32: inverse temperature times log2(e); it must be finite and >= 0 (SGW_ERR_ARG
 * otherwise); 0 gives a uniform policy over the finite scores.
 *   z_j   = (score[j] - top) * beta2            one float32 subtraction, then one float32 multiplication
 *   w_j   = E(z_j)
 *   E(z)  : if !(z >= -125.0f) -> +0.0f         (NaN included: a NaN or -inf score is never sampled)
 *           k = rintf(z) (ties to even);  g = z - k          (exact, g in [-0.5, 0.5])
 *           p = 1 + g*(c1 + g*(c2 + g*(c3 + g*(c4 + g*(c5 + g*c6)))))   Horner: every * and + one float32 operation, nothing fused
 *           E = ldexpf(p, (int)k)               (exact: never subnormal)
 *           c1..c6 = float32((ln 2)^i / i!) = 0x1.62e430p-1, 0x1.ebfbe0p-3, 0x1.c6b08ep-5, 0x1.3b2ab6p-7, 0x1.5d87fep-10, 0x1.430912p-13
 *   total = 0.0; for j = 0..NA-1 in order: total = total + (double)w_j        one double addition each
 *   degenerate iff !(total > 0.0)               (exactly when top is NaN or infinite)
 *   pi_j  = (double)w_j / total                 one double division
 * E is within 2^-21.9 (relative) of 2^z on [-125, 0]; its smallest non-zero value is 2^-125; it is not monotone in its last bit,
 * and nothing here depends on monotonicity.
 * SAMPLING, with step = *step_dev + t and the global env id as for sgw_policy_act:
 *   explore first, exactly as sgw_policy_act (the tag-2 draws, explore_below): if the agent explores, that index is the action
 *   else if degenerate: index = best
 *   else (x0, ..) = Philox-4x32-10(counter = (step, 3, a, env_id >> 32), key = (seed, env_id))       (tag 3: the sampler's stream)
 *        u = ((double)x0 + 0.5) * 2^-32 ;  thr = u * total                                            one double multiplication
 *        cum = 0.0; index = first j, scanning j = 0.. in order, with thr < (cum = cum + (double)w_j)
 *        (always found: cum ends on total bit for bit, and thr < total)
 *   actions[n][a] = action_lo + index; a policy index outside 0 .. P-1 writes 0 and reads no table.
 * sgw_policy_sample is sgw_policy_act with that rule (one launch; the same arguments and checks); sgw_policy_sample_step_n is
 * sgw_policy_step_n with the sampling launch in place of the greedy one: the same 2T + 1 launches, the same graph cache, whose
 * key also holds beta2 and the kind of call, so a greedy and a sampled call over the same pointers never share a graph. */
int sgw_policy_sample(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs_dev, int64_t t, int8_t* actions_dev,
                      void* stream);
int sgw_policy_sample_step_n(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs0_dev, int T, int write_every,
                             const sgw_out* out, int8_t* actions_out_dev /* [T, N, A] */, int accumulate, void* stream);
/* The probabilities over the T + 1 observations O[0 .. T], laid out as for sgw_policy_scores.  Outputs, at least one:
 *   probs    float32 [T+1, N, A, n_actions] = (float)pi_j; a degenerate row is 1.0f at best and +0.0f elsewhere; a policy index
 *            outside 0 .. P-1 gives +0.0f everywhere
 *   p_chosen double  [T, N, A] = pi of the taped action (needs actions_dev): +0.0 for an action outside the spec's range (or an
 *            unknown policy index), 1.0 or 0.0 on a degenerate row depending on whether the taped action is best
 * These are the probabilities of the softmax alone: the exploration mixture of explore_below is NOT folded in (with epsilon > 0
 * the behaviour policy is (1 - eps) * pi + eps / n_actions; that correction is the caller's).
 * SGW_ERR_ARG: as sgw_policy_scores (T < 0, null obs0 / obs, obs_rows < N, no output, p_chosen without actions, misalignment),
 * and a bad beta2.  One launch: no allocation, no synchronisation, capturable. */
int sgw_policy_probs(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs0_dev, const uint8_t* obs_dev, int64_t obs_rows,
                     int T, const int8_t* actions_dev /* [T, N, A] or NULL */, float* probs_dev, double* p_chosen_dev, void* stream);
/* The score-function (policy-gradient) sums into the int64 fixed-point accumulators of sgw_policy_accumulate.  For every transition
 * with a known policy index, an action a* = actions[t][n][a] - action_lo inside 0 .. n_actions-1 and a row that is not degenerate,
 * and for EVERY j (each operation one double operation):
 *   d_j = (j == a* ? 1.0 : 0.0) - pi_j ;  x_j = coef * d_j ;  q_j = the quantisation of sgw_policy_accumulate applied to x_j
 *   acc_bias[p][a][j] += q_j                                     (when acc_bias_dev is given)
 *   acc_weights[p][a][c][code_of[o[c]]][j] += q_j                for every c < C_a
 * Skipped transitions add nothing.  This is the gradient of log pi(a*) with respect to the scores, times coef; the true gradient
 * carries one more factor beta2 * ln 2 (the scores enter the exponent as score * beta2 in base 2), which is the caller's to fold
 * into lr.  Everything else -- in/out accumulators, T * N < 2^32, the 2048-byte row limit (SGW_ERR_UNSUPPORTED), alignment and
 * the pointer-equality refusals, one capturable launch -- is sgw_policy_accumulate's; a bad beta2 is SGW_ERR_ARG. */
int sgw_policy_accumulate_softmax(sgw_engine* e, const sgw_policy* p, float beta2, const uint8_t* obs0_dev, const uint8_t* obs_dev,
                                  int64_t obs_rows, int T, const int8_t* actions_dev, const double* coef_dev, int frac_bits,
                                  int64_t* acc_weights_dev, int64_t* acc_bias_dev /* or NULL */, void* stream);

/* Per-env performance bookkeeping of SafetyEnvironment{,Mo}: _episodic_performances.append(...) at every LAST timestep
 * (safety_game.py:253-263, 301-302; safety_game_mo.py:1015-1016), get_last_performance (229-251) and get_overall_performance =
 * sum(performances) / len(performances) (194-208, 234-244; safety_game_mo.py:917-938).  perf_dev double [N, C] is the step's
 * performance source (the `cumulative` output, C = A*K, or the `hidden` output, C = 1); where step_type_dev[n, 0..A) is LAST
 * (every agent LAST or DEAD for the families whose agents finish one by one): last_dev[n] = perf[n], sum_dev[n] += perf[n]
 * (the reference's left-to-right sum), count_dev[n] += 1; done_dev[n] = 1 there and 0 elsewhere (the wrapper's `terminated`,
 * gridworld_gym_env.py:563-578).  Any of last / sum / count / done may be NULL. */
int sgw_track_performance(sgw_engine* e, const double* perf_dev, int n_cols, const uint8_t* step_type_dev, double* last_dev,
                          double* sum_dev, int64_t* count_dev, uint8_t* done_dev, void* stream);

/* The episode log: one record per episode that ENDS in a batch of output rows, appended to a caller-owned log in (t, n) order --
 * the reference's _episodic_performances (safety_game.py:253-263, safety_game_mo.py:1015-1016) for the whole batch, with the
 * env, the step, the length, the termination reason, the return vector, the hidden performance and the metrics of the row that
 * was LAST.  With envs that auto-reset inside the launch those numbers are overwritten one step later; this is how they are
 * kept without [T, N_pad, ...] trajectory buffers and without a host synchronisation per step.
 *
 * src is the sgw_out the steps wrote: T == 1: plain [N_pad, ...] arrays; T > 1: the rollout-buffer layout [T, N_pad, ...] of
 * sgw_step_n / sgw_rollout / sgw_replay with write_every != 0.  Rows >= N are never logged.  Row (t, n) ends an episode by the
 * predicate of sgw_track_performance: step_type[n, 0] == LAST, or every agent LAST or DEAD for island_navigation_ex_ma and
 * aintelope_savanna (that predicate holds again on an idle round after the end -- every submitted action < 0, no reset -- and
 * such a row is logged again, as sgw_track_performance counts it again).
 * The records of one call are appended at *count in (t, n) order and calls append in stream order: the log is a deterministic
 * function of the inputs.  *count advances by the TRUE number of ended episodes; records at index >= cap are not stored and
 * entries past min(*count, cap) are never written.  src->step_type, log->count and log->scratch are required; every other
 * destination may be NULL (cap == 0 with all of them NULL: the pure counter); a destination whose source output is NULL is
 * SGW_ERR_ARG.  Three plain launches on the caller's stream: no host synchronisation, no allocation, no read-back, capturable. */
typedef struct sgw_episodes {     /* destination: a caller-owned append-only log, all device pointers */
  int64_t  cap;          /* records the arrays below can hold (>= 0) */
  int64_t* count;        /* [1] episodes logged so far, INCLUDING those that did not fit; the caller zeroes it to start or clear */
  int32_t* env;          /* [cap]        env index within the engine (global id = env_id_base + env) */
  int64_t* step;         /* [cap]        step_base + t of the row that was LAST */
  int32_t* length;       /* [cap]        the `frame` output of that row (the episode's length) */
  uint8_t* term_reason;  /* [cap, R]     R = A for the families whose agents finish one by one, else 1 */
  double*  ret;          /* [cap, A*K]   the `cumulative` output of that row: the episode return vector(s) */
  double*  hidden;       /* [cap]        the `hidden` output of that row: hidden performance */
  double*  metrics;      /* [cap, M] */
  void*    scratch;      /* sgw_episode_scratch_bytes(n_envs, T) bytes, 8-byte aligned; contents are the call's own */
} sgw_episodes;
int sgw_sizeof_episodes(void);
int64_t sgw_episode_scratch_bytes(int64_t n_envs, int T);   /* pure host arithmetic, no device; < 0 = SGW_ERR_ARG */
int sgw_log_episodes(sgw_engine* e, const sgw_out* src, int T, int64_t step_base, const sgw_episodes* log, void* stream);

/* Everything env.step() returns from ONE host call: sgw_step, then -- on the same stream, chained in C -- whatever of the
 * observation distiller's and _process_timestep's derived outputs `extras` asks for, computed from that step's outputs:
 * RGB (sgw_observe), unoccluded layers (sgw_observe_layers; aintelope_savanna: sgw_state_layers), derived statistics
 * (sgw_derived_stats), per-agent layer cubes (sgw_agent_layer_views), performance bookkeeping (sgw_track_performance).  With
 * extras->replay != 0 the second call with the same (actions_dev, out, extras) pointers captures the launches into a hipGraph and
 * replays it from then on (one graph launch per step instead of up to six kernel launches; refill the action buffer in place);
 * replay == 0 issues the launches directly, which is the faster end to end while the host keeps up.  `out` must carry what the
 * requested extras read: board (rgb, layers), agent_pos + agent_flags (hidden drape, layer cubes), reward + cumulative + frame
 * (stats), cumulative or hidden + step_type (performance).  Reference: gridworld_gym_env.py:455-585, safety_game_mo.py:971-1107,
 * observation_distiller_ex.py:147-187. */
typedef struct sgw_extras {
  uint8_t* rgb;                       /* [N, 3, H*W] or NULL */
  const uint8_t* rgb_lut_dev;         /* uint8 [128*3] */
  uint8_t* layers;                    /* unoccluded [N, L, H*W] or NULL */
  const uint8_t* layer_chars_dev;     /* uint8 [L] */
  const uint8_t* layer_static_dev;    /* uint8 [L, H*W] (unused by aintelope_savanna) */
  int32_t n_layers, gap_index, hidden_layer, perf_from_hidden;
  double* stats;                      /* [N, A, 5 + K] or NULL */
  int32_t k_agent[SGW_MAX_AGENTS];
  uint8_t* agent_layer_views;         /* [N, L * view_bytes] or NULL (needs `layers`) */
  double* perf_last;                  /* [N, C] / [N, C] / int64 [N] / uint8 [N]; all NULL = no bookkeeping */
  double* perf_sum;
  int64_t* perf_count;
  uint8_t* done;
  int32_t replay;                     /* 0: the launches are issued one by one (lowest end-to-end time per step: 38.7 us for the full
                                       * island_navigation_ex set at 65 536 envs, ~25 us of host time); != 0: the chain is captured
                                       * on the second identical call and replayed as ONE hipGraph from the third on (~5 us of host
                                       * time per step for a consumer whose host thread is the bottleneck, at ~5 us more GPU time
                                       * per step: 44.3 us) */
  int32_t reserved_;
} sgw_extras;
int sgw_step_full(sgw_engine* e, const int8_t* actions_dev, const sgw_out* out, const sgw_extras* extras, void* stream);

/* Unoccluded observation layers (BaseUnoccludedObservationRenderer, rendering.py:188-302, which the multi-objective
 * and multi-agent envs use: safety_game_mo_base.py:1157) with the "gap only where every other layer is blank"
 * correction of the distiller (observation_distiller_ex.py:164-178).  layer_static_dev uint8 [L, H*W]: 0/1 = the
 * layer's static curtain (backdrop characters, static drapes), 2 = dynamic (sprite / moving drape: board == char).
 * gap_index = index of the what_lies_beneath layer (-1: no correction).  layers_dev uint8 [N, L, H*W].
 * A dynamic drape hidden under a sprite (fire that spread under an agent) is invisible in the board: pass the
 * step's agent_pos / agent_flags outputs and hidden_layer = that drape's layer index (else NULL, NULL, -1). */
int sgw_observe_layers(sgw_engine* e, const uint8_t* board_dev, const uint8_t* layer_chars_dev,
                       const uint8_t* layer_static_dev, int n_layers, int gap_index, const uint8_t* agent_pos_dev,
                       const uint8_t* agent_flags_dev, int hidden_layer, uint8_t* layers_dev, void* stream);

/* aintelope_savanna: its drapes overlap (a food tile may spawn on gold, a predator may stand on either), so the board
 * shows only the top one and the unoccluded layers come from the state instead: layers_dev uint8 [N, L, H*W] for the
 * characters in layer_chars_dev ('#', ' ', W P D F d f G S, '0', '1'), as of the last step / reset.  gap_only_blank != 0:
 * the ' ' layer is set only where every other layer is blank (observe_gaps_only_where_other_layers_are_blank=True,
 * aintelope_savanna.py:1690), else wherever the backdrop is not a wall. */
int sgw_state_layers(sgw_engine* e, const uint8_t* layer_chars_dev, int n_layers, int gap_only_blank, uint8_t* layers_dev,
                     void* stream);

/* Agent-centric observations (get_agent_perspective, safety_game_moma.py:1996-2101): for every env and
 * agent a, the (up+down+1) x (left+right+1) window of the rendered board centred on the agent, cells
 * outside the board filled with `outside_chr`.  views_dev uint8 [N, view_bytes] with agent a's window at
 * byte offset sum of the previous agents' window sizes (sgw_view_bytes gives the row size).
 * agent_flags_dev (the `agent_flags` output, or NULL): when given, each window is rot90-ed by the agent's observation
 * direction after cropping (observation_direction_mode != 0, safety_game_moma.py:2085-2096; square windows only). */
int sgw_view_bytes(const sgw_engine* e);
int sgw_agent_views(sgw_engine* e, const uint8_t* board_dev, const uint8_t* agent_pos_dev, const uint8_t* agent_flags_dev,
                    uint8_t outside_chr, uint8_t* views_dev, void* stream);

/* The same agent-centric windows for every observation LAYER (agent_perspectives_with_layers,
 * safety_game_moma.py:430-525): layers_dev uint8 [N, L, H*W] (sgw_observe_layers), out uint8 [N, L * view_bytes]
 * laid out per env as agent-major [agent][layer][h][w]; cells outside the board read (layer char == outside_chr). */
int sgw_agent_layer_views(sgw_engine* e, const uint8_t* layers_dev, const uint8_t* agent_pos_dev, const uint8_t* agent_flags_dev,
                          const uint8_t* layer_chars_dev, int n_layers, uint8_t outside_chr, uint8_t* out_dev, void* stream);

/* Object coordinates (object_coordinates_in_observation=True, the wrappers' default): the set cells of byte planes as padded
 * lists, one launch for every env.  counts are the TRUE numbers of set cells (also when they exceed cap); entries
 * 0 .. min(count, cap) - 1 of a list hold the cells in row-major (np.argwhere) order and the entries past them are NOT written
 * (the caller's bytes stay: the launch stores as much as there are objects, not cap).  counts_dev and coords_dev 4-byte aligned.
 *
 * info_observation_coordinates: (row, col) of the set cells of every layer, np.argwhere order.
 * layers_dev uint8 [N, L, H*W]; counts_dev int32 [N, L]; coords_dev int16 [N, L, cap, 2]. */
int sgw_layer_coords(sgw_engine* e, const uint8_t* layers_dev, int n_layers, int cap,
                     int32_t* counts_dev, int16_t* coords_dev, void* stream);

/* info_agent_observation_coordinates: (x - ax, y - ay) inside each agent's window.
 * views_dev uint8 [N, L * view_bytes] as written by sgw_agent_layer_views ([agent][layer][h_a][w_a] per env);
 * agent_layer[A] = index of the agent's own character among the L layers, -1 = none;
 * counts_dev int32 [N, A, L] (-1 = the agent is not in its own layers); coords_dev int16 [N, A, L, cap, 2].
 * (ay, ax) is the first set cell, in row-major order, of the agent's own layer inside its own window (safety_game_moma.py:528-580;
 * the windows are already rot90-ed by sgw_agent_layer_views).  agent_layer is HOST memory, read at call time. */
int sgw_agent_layer_coords(sgw_engine* e, const uint8_t* views_dev, int n_layers, const int32_t* agent_layer,
                           int cap, int32_t* counts_dev, int16_t* coords_dev, void* stream);

/* State copy-out / copy-in (tests, checkpointing) in a layout-independent form: uint64 [words][N_pad], word w of env n at
 * [w][n] (the engine itself keeps word pairs interleaved per 64-env wave; these two calls convert). */
int sgw_state_words(const sgw_engine* e);
int sgw_get_state(sgw_engine* e, uint64_t* state_dev, void* stream);
int sgw_set_state(sgw_engine* e, const uint64_t* state_dev, void* stream);

/* Fork envs: for every pair i < n, env dst_idx_dev[i] of `dst` becomes a bit-exact copy of env src_idx_dev[i] of `src` -- what
 * copy.deepcopy(env) and pickling give the reference's users (safety_game_mo.py:406-419), batched.  Every state word is copied
 * (generator streams, draw counters and cached maps are state words); an index array that is NULL means i.  With dst_out and
 * src_out the env's ROW of every output that is non-NULL in dst_out is copied from src_out too, so the destination's current
 * observation is valid without a step (non-NULL in dst_out and NULL in src_out: SGW_ERR_ARG; outputs set only in src_out are
 * ignored; both NULL: the state only).  Rows are those of the [N_pad, ...] arrays of struct sgw_out for the engines' spec
 * (sgw_out_row_bytes); step t of a [T, N_pad, ...] buffer is addressed by passing the pointers of that t.
 * A pair is skipped -- nothing of it is read or written -- when either index is negative or >= n_envs of its engine (the mask:
 * dst_idx_dev[i] = -1), or when dst == src and the two indices are equal.
 * One plain launch on the caller's stream: no allocation, no synchronisation, no read-back; capturable.
 * dst and src may be one engine; otherwise they must be on one device, with byte-identical sgw_spec and equal sgw_state_words
 * (SGW_ERR_ARG otherwise); n_envs and env_id_base may differ.
 * The CALLER guarantees, unchecked on the device: the destination indices are distinct; within one engine no env is the source
 * of one pair and the destination of another.  Repeated sources (fan-out) are fine.
 * NOT copied: the episodic-return accumulators (sgw_read_returns); captured graphs (none is invalidated: no launch argument
 * moves); performance bookkeeping and episode logs (caller-owned); the engine-level external inputs (sgw_set_episode_bits,
 * sgw_set_random_stream, sgw_set_family_table).  The copy carries the env's episode and draw counters, so a copied env draws
 * from the DESTINATION engine's inputs, keyed by the destination's global env id (seeded streams) or array row; env-owned PCG64
 * generators are state and continue identically wherever the copy lands.
 * firemaker_ex_ma, island_navigation_ex_ma, aintelope_savanna: the destination's generators must have been set by one of its own
 * setters before (sgw_set_rng_state, sgw_seed_rng, sgw_set_state), SGW_ERR_ARG otherwise: the padding lanes of a never-seeded
 * engine hold no working stream, and this call never marks an engine as seeded. */
int sgw_copy_envs(sgw_engine* dst, const sgw_engine* src, const int32_t* dst_idx_dev, const int32_t* src_idx_dev, int64_t n,
                  const sgw_out* dst_out, const sgw_out* src_out, void* stream);
/* Bytes of one env's row of an output: field = position in struct sgw_out, 0 = board ... 19 = act_dir; per family (term_reason /
 * safety widths, the window bytes, safety2 for aintelope_savanna only).  0: the family has no such output; < 0: bad argument. */
int64_t sgw_out_row_bytes(const sgw_engine* e, int field);

/* Which kernel runs the engine's one-step launches (sgw_step, sgw_step_n): 0 = the generic kernel, k > 0 = the k-th kernel with
 * the output geometry of one spec compiled in (chosen by sgw_create when family, state variant and geometry match one exactly;
 * SGW_GENERIC_STEP set in the environment at sgw_create keeps the generic kernel).  Both compute the same bytes. */
int sgw_step_shape(const sgw_engine* e);

/* 1 when those launches run a kernel that also has the spec's whole rule set compiled in (flags, parameters and level of one
 * spec, chosen by sgw_create when sgw_step_shape's kernel has such a variant and the spec equals it bit for bit;
 * SGW_GENERIC_RULES set in the environment at sgw_create keeps the shape-only kernel), 0 otherwise.  Same bytes either way. */
int sgw_step_rules(const sgw_engine* e);

/* 1 when those launches run the forked kernel: every env-wave as a state wave and an output wave that both run the rules and
 * each keep one side of the result (chosen by sgw_create for an engine with sgw_step_rules' kernel whose launch has at most one
 * env-wave per SIMD of its device; SGW_NO_FORK set in the environment at sgw_create keeps the one-wave kernel), 0 otherwise.
 * Same bytes either way. */
int sgw_step_fork(const sgw_engine* e);

/* Dynamic LDS, in bytes per workgroup, that a one-step launch (sgw_step, sgw_step_n) of this engine asks for when `out` names
 * these outputs (NULL: none): what decides, with the kernel's registers, how many workgroups a CU keeps resident.  Nothing is
 * launched.  Negative = the error code such a launch would return.  For an engine whose launches fork (sgw_step_fork) this is
 * the one-wave kernel's figure; the forked kernel's workgroups hold half as many env-waves and ask for less. */
int64_t sgw_step_lds_bytes(sgw_engine* e, const sgw_out* out);

#ifdef __cplusplus
}
#endif
#endif  /* SGW_H_ */
