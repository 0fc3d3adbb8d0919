"""One row per base env name (specs.ENV_FAMILIES + aintelope_savanna) for the launch-path matrix of
tests/test_launch_paths_gpu.py: sgw_step_n (direct, capture, replay), sgw_replay, sgw_rollout, sgw_group_step_n and
sgw_group_rollout, each compared with the C oracle.  Kwargs end episodes inside the run (small max_iterations where the family
takes one), so auto-reset happens inside captured and replayed graphs.  tests/test_launch_paths.py (CPU) checks that every
base env name has a row and that `tag` names the SGW_GROUP_FAMILIES member exactly where csrc/sgw_group.hpp lists one.

A row: id; name, kw (make_spec); n (envs: ragged, never a multiple of 64); outs; inputs -- bits / rand: None, "array"
(explicit per-env arrays) or "philox" (the engine's seeded stream, restated on the host for the oracle), rng: per-env PCG64
states; oracle: "scalar" (oracle.oracle), "ma" (oracle_ma), "ima" (oracle_ima) or "sav" (oracle_sav); tag: the group member
tag name, or None where the family / configuration is refused as a member; state_words: expected sgw_state_words (the
packed / plain island state); calls: step_n / replay / rollout calls of T = 16 steps -- 7 for tomato_watering, tomato_crmdp
and rocks_diamonds, which take no max_iterations: their 100-step episodes end (and auto-reset) inside the seventh call.

Two rows pass a `rand` array that nothing reads: `friend_foe` fixes bandit_type="friend" (no bandit-type draw, argmax instead of the
neutral bandit's draw) and `whisky_gold` has human_player=False (no exploration draw, no replacement).  They pin the families'
deterministic rules on every path; the rows that consume random numbers -- friendfoe_random, friendfoe_neutral, whisky_human,
whisky_human_array -- and the seeded rows away from env id 0 live in tests/seeded_draws.py, which has its own row table (ROWS
here stays one row per env name; tests/test_seeded_draws.py checks that both rows have a drawing complement there).

case() / check() / check_returns() / run_path() / run_group() are the launch-path matrix itself, shared by
tests/test_launch_paths_gpu.py (ROWS) and tests/test_seeded_draws_gpu.py (its rows): they take a row (or the id of one of ROWS)
and need a GPU.  A row may carry two more keys: `base` (the engine's env_id_base, default 0) and `seed` (the seed of inputs(),
default: the row's index in ROWS)."""
import numpy as np

from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import ALL_OUTPUTS

WIN = ALL_OUTPUTS + ("views",)
SAV = ALL_OUTPUTS + ("views", "safety2")


def _row(id, name, kw, n, tag, oracle="scalar", outs=ALL_OUTPUTS, bits=None, rand=None, rng=False, state_words=None, calls=3):
  return dict(id=id, name=name, kw=kw, n=n, tag=tag, oracle=oracle, outs=outs, bits=bits, rand=rand, rng=rng,
              state_words=state_words, calls=calls)


ROWS = [
    _row("island_ex_packed", "island_navigation_ex", dict(level=5, max_iterations=12), 1000, "TAG_ISLAND_PACKED", state_words=10),
    _row("island_ex_plain", "island_navigation_ex", dict(level=4, max_iterations=14, MOVEMENT_REWARD={"MOVEMENT_REWARD": -0.5}),
         1003, "TAG_ISLAND", state_words=22),
    _row("island_ex_general", "island_navigation_ex", dict(level=6, max_iterations=13, DRINK_REWARD={"DRINK_REWARD": 2.0, "FOOD_REWARD": -1.0}),
         999, None),
    _row("boat_race_ex", "boat_race_ex", dict(level=1, max_iterations=11), 1001, "TAG_BOAT"),
    _row("boat_race", "boat_race", dict(level=0, max_iterations=10, noops=True), 957, "TAG_BOAT"),
    _row("safe_interruptibility", "safe_interruptibility", dict(level=0, max_iterations=12), 1010, "TAG_SAFEINT", bits="array"),
    _row("safe_interruptibility_ex", "safe_interruptibility_ex", dict(level=1, max_iterations=15), 33, "TAG_SAFEINT", bits="philox"),
    _row("firemaker_ex_ma", "firemaker_ex_ma", dict(amount_agents=3, max_iterations=14), 401, None, oracle="ma", outs=WIN, rng=True),
    _row("island_ex_ma", "island_navigation_ex_ma", dict(level=6, map_randomization_frequency=2, map_width=11, map_height=7,
                                                           max_iterations=13), 803, None, oracle="ima", outs=WIN, rng=True),
    _row("island_navigation", "island_navigation", dict(level=0, max_iterations=12), 1005, "TAG_TILE"),
    _row("distributional_shift", "distributional_shift", dict(is_testing=False), 777, "TAG_TILE", bits="array"),
    _row("absent_supervisor", "absent_supervisor", dict(), 1011, "TAG_TILE", bits="array"),
    _row("side_effects_sokoban", "side_effects_sokoban", dict(level=0, noops=True), 1015, "TAG_SOKOBAN"),
    _row("conveyor_belt", "conveyor_belt", dict(variant="sushi", max_iterations=12), 1017, "TAG_CONVEYOR"),
    _row("conveyor_belt_ex", "conveyor_belt_ex", dict(variant="sushi_goal2", noops=True, max_iterations=13), 49, "TAG_CONVEYOR"),
    _row("tomato_watering", "tomato_watering", dict(), 1019, "TAG_TOMATO", rand="array", calls=7),
    _row("tomato_crmdp", "tomato_crmdp", dict(), 1021, "TAG_TOMATO", rand="philox", calls=7),
    _row("friend_foe", "friend_foe", dict(bandit_type="friend"), 1023, "TAG_FRIEND_FOE", rand="array"),
    _row("whisky_gold", "whisky_gold", dict(human_player=False, whisky_exploration=0.7), 1025, "TAG_WHISKY", rand="array"),
    _row("rocks_diamonds", "rocks_diamonds", dict(level=1), 1027, "TAG_ROCKS", calls=7),
    _row("aintelope_savanna", "aintelope_savanna",
         dict(amount_agents=2, amount_predators=2, amount_water_tiles=2, amount_gold_deposits=2, amount_silver_deposits=1,
              amount_small_food_patches=1, amount_drink_holes=1, amount_small_drink_holes=1, sustainability_challenge=True,
              penalise_oversatiation=True, max_iterations=14, observation_radius=[2, 2, 2, 2]), 601, None, oracle="sav", outs=SAV,
         rng=True),
]
BY_ID = {r["id"]: r for r in ROWS}

# groups of member rows: every member tag at least once, one group of 4 (member index 3, hot_fb3), one member under 64 envs
GROUPS = [
    ("g4_scalar", ["island_ex_packed", "boat_race_ex", "safe_interruptibility_ex", "tomato_watering"]),
    ("g4_tiles", ["island_ex_plain", "distributional_shift", "side_effects_sokoban", "conveyor_belt_ex"]),
    ("g4_rand", ["friend_foe", "whisky_gold", "rocks_diamonds", "safe_interruptibility"]),
    ("g3_mixed", ["absent_supervisor", "tomato_crmdp", "conveyor_belt"]),
    ("g2_pair", ["boat_race", "island_navigation"]),
]

N_BITS, N_RAND = 64, 4096
PCG_SEED = 321


def philox_uniforms(seed, env_ids, n):
  """The engine's in-play uniforms with no stream set (sgw_common.hpp next_uniform): draw k of an env is word pair k & 1 of
  Philox(block k >> 1, TAG_EPISODE, 1, env id >> 32; key seed, env id).  float64 [len(env_ids), n]."""
  env_ids = np.asarray(env_ids, dtype=np.uint64)[:, None]
  blocks = np.arange((n + 1) // 2, dtype=np.uint64)[None, :]
  x0, x1, x2, x3 = philox.philox4x32_10(blocks, philox.TAG_EPISODE, 1, env_ids >> np.uint64(32), seed, env_ids)
  u0 = ((x0.astype(np.uint64) << np.uint64(21)) | (x1.astype(np.uint64) >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
  u1 = ((x2.astype(np.uint64) << np.uint64(21)) | (x3.astype(np.uint64) >> np.uint64(11))).astype(np.float64) * 2.0 ** -53
  return np.stack([u0, u1], axis=2).reshape(len(env_ids), -1)[:, :n]


def episode_bit_rule(spec):
  """(probability, inclusive) of a family's seeded per-episode bit, read from the spec: safe_interruptibility(_ex) interrupts where
  episode_uniform <= interruption_probability (sgw_safeint.hpp), the tile family (distributional_shift is_testing=True,
  absent_supervisor) takes variant 1 where episode_uniform < P_PROB (sgw_tile.hpp).  Both keep the probability in params[2]."""
  from ai_safety_gridworlds_amd import _native as N
  assert spec.family in (N.SAFE_INTERRUPTIBILITY, N.TILE_EVENTS), "%s draws no per-episode bit" % spec.name
  return float(spec.native.params[2]), spec.family == N.SAFE_INTERRUPTIBILITY


def global_ids(n, base=0):
  """uint64 [n]: the global env ids of an engine of n envs at env_id_base = base."""
  return np.uint64(base) + np.arange(n, dtype=np.uint64)


def restate_seeded(row, spec, d, ids):
  """The engine's seeded streams (d["bits_seed"] / d["rand_seed"]) restated on the host for the envs `ids` (global env ids, any
  order) into d["bits_oracle"] / d["rand_oracle"]; explicit arrays stay as they are."""
  ids = np.asarray(ids, dtype=np.uint64)
  if row["bits"] == "philox":
    p, inclusive = episode_bit_rule(spec)
    u = philox.episode_uniform(d["bits_seed"], ids[:, None], np.arange(N_BITS)[None, :])
    d["bits_oracle"] = ((u <= p) if inclusive else (u < p)).astype(np.uint8)
  if row["rand"] == "philox":
    d["rand_oracle"] = philox_uniforms(d["rand_seed"], ids, N_RAND)
  return d


def inputs(row, spec, seed, base=0):
  """Host arrays for the row's external inputs: dict(bits=, bits_seed=, rand=, rand_seed=, rng=), with what the oracle reads
  (bits_oracle / rand_oracle) -- the explicit arrays themselves, or the engine's seeded Philox streams restated over the global
  env ids base + arange(n) (base: the engine's env_id_base)."""
  E, rs = row["n"], np.random.default_rng(seed)
  d = dict(bits=None, bits_seed=0, rand=None, rand_seed=0, rng=None, bits_oracle=None, rand_oracle=None)
  if row["bits"] == "array":
    d["bits"] = d["bits_oracle"] = rs.integers(0, 2, (E, N_BITS)).astype(np.uint8)
  elif row["bits"] == "philox":
    d["bits_seed"] = 1000 + seed
  if row["rand"] == "array":
    d["rand"] = d["rand_oracle"] = rs.random((E, N_RAND))
  elif row["rand"] == "philox":
    d["rand_seed"] = 2000 + seed
  restate_seeded(row, spec, d, global_ids(E, base))
  if row["rng"]:
    from oracle import oracle_ma as OM
    d["rng"] = np.stack([OM.rng_state_words(PCG_SEED + seed + e) for e in range(E)])
  return d


def run_oracle(row, host_actions, inp, nthreads=16):
  """host_actions: int8 [T, E(, A)] (the device stream copied back) -> the oracle's arrays [E, T + 1, ...]."""
  acts = np.ascontiguousarray(np.moveaxis(host_actions, 0, 1))
  if row["oracle"] == "scalar":
    from oracle import oracle as O
    return O.run_streams(O.make_config(row["name"], **row["kw"]), acts, interrupt_bits=inp["bits_oracle"], nthreads=nthreads,
                         rand_stream=inp["rand_oracle"])
  from oracle import oracle_ima as OI, oracle_ma as OM, oracle_sav as OS
  Or = {"ma": OM, "ima": OI, "sav": OS}[row["oracle"]]
  return Or.run_streams(Or.make_config(**row["kw"]), acts, inp["rng"], nthreads=nthreads)


DEV = "cuda:0"


def make_engine(row, spec, inp, base=0):
  """The row's engine on the GPU (env_id_base = base) with the external inputs of inputs() set; not reset."""
  from ai_safety_gridworlds_amd.engine import BatchedEngine
  eng = BatchedEngine(spec, row["n"], device=DEV, env_id_base=base, outputs=row["outs"])
  if inp["bits"] is not None or inp["bits_seed"]:
    eng.set_episode_bits(inp["bits"], seed=inp["bits_seed"])
  if inp["rand"] is not None or inp["rand_seed"]:
    eng.set_random_stream(inp["rand"], seed=inp["rand_seed"])
  if inp["rng"] is not None:
    eng.set_rng_state(inp["rng"])
  return eng


def start(eng, row):
  for _ in range(resets(row)):
    o = eng.reset()
  return o


def to_np(views, stacked):
  """{field: device tensor} -> {field: numpy [E, S, ...]}; `stacked`: [S, E, ...] (write_every / a list of steps)."""
  return {k: np.moveaxis(v.cpu().numpy(), 0, 1) if stacked else v.cpu().numpy()[:, None] for k, v in views.items()}


def split_views(spec, v):
  out, off = [], 0
  for (h, w) in spec.view_shapes:
    out.append(v[..., off:off + h * w].reshape(v.shape[:-1] + (h, w)))
    off += h * w
  return out


def resets(row):
  """Resets before the first step: the island_navigation_ex_ma / aintelope_savanna oracles record two (the reference's
  environment resets once when it is built and once more when the episode starts; map randomisation draws at both)."""
  return 2 if row["oracle"] in ("ima", "sav") else 1


FIREMAKER_METRICS = [p + "Visits_" + a for p in ("External", "Internal", "Workshop", "Fire", "StopButton") for a in "12S"] + \
    ["StopButtonPressCountdown"]
SCALAR_FIELDS = ("step_type", "reward", "cumulative", "discount", "term_reason", "actual_action", "frame", "hidden", "board")


def _same(g, w):
  return bool(((g == w) | ((g != g) & (w != w))).all())             # NaN == NaN (metrics)


def oracle_mismatches(row, spec, got, want, s0, views=None):
  """got: {field: [E, S, ...] numpy} engine outputs of steps s0 .. s0 + S - 1 (step 0 = the (last) reset).  Returns the names of the
  fields that differ from the oracle (empty: equal).  views: list over agents of [E, S, h, w] windows (split_views).  The
  multi-agent families are compared on every output the oracle records: term_reason 255 -> -1, per-agent slots for firemaker,
  the present agents' columns [:, :, :A] for island_navigation_ex_ma / aintelope_savanna."""
  S = next(iter(got.values())).shape[1]
  sl = slice(s0, s0 + S)
  bad = []
  if row["oracle"] == "scalar":
    for f in SCALAR_FIELDS + (("metrics",) if spec.M else ()) + (("safety",) if row["name"] == "island_navigation_ex" else ()):
      w, g = want[f][:, sl], got[f]
      if f == "term_reason":
        g = g.astype(np.int16); g[g == 255] = -1
      if f == "metrics":
        g = g[..., :spec.M]
      if not _same(g.reshape(w.shape), w):
        bad.append(f)
    return bad
  tr = got["term_reason"].astype(np.int16); tr[tr == 255] = -1
  fl = got["agent_flags"]
  if row["oracle"] == "ma":                                          # firemaker: per-agent slots
    slots = list(spec.agent_slots)
    E = got["board"].shape[0]
    pairs = [("board", got["board"].reshape(want["board"][:, sl].shape), want["board"][:, sl]),
             ("frame", got["frame"], want["frame"][:, sl]), ("discount", got["discount"], want["discount"][:, sl]),
             ("term_reason", tr, want["term_reason"][:, sl, 0]),
             ("agent_pos", got["agent_pos"].reshape(E, S, spec.A, 2)[:, :, slots], want["pos"][:, sl][:, :, slots]),
             ("action_direction", ((fl >> 1) & 3)[:, :, slots], want["action_direction"][:, sl][:, :, slots]),
             ("observation_direction", ((fl >> 3) & 3)[:, :, slots], want["observation_direction"][:, sl][:, :, slots])]
    pairs += [(f, got[f][:, :, slots], want[f][:, sl][:, :, slots]) for f in ("step_type", "reward", "cumulative")]
    assert list(spec.metric_names) == FIREMAKER_METRICS, "the row's metric columns are the oracle's 16"
    pairs.append(("metrics", got["metrics"], want["metrics"][:, sl]))
    if views is not None:
      pairs += [("views[%d]" % q, views[q], want["view_worker"][:, sl, q] if q < 2 else want["view_supervisor"][:, sl]) for q in slots]
    return [f for f, g, w in pairs if not _same(g, w)]
  E, A = got["board"].shape[0], want["step_type"].shape[2]           # island_navigation_ex_ma / aintelope_savanna
  sl = slice(s0 + 1, s0 + 1 + S)                                     # (the oracle's record starts with two resets)
  pairs = [("board", got["board"].reshape(want["board"][:, sl].shape), want["board"][:, sl]),
           ("step_type", got["step_type"][:, :, :A], want["step_type"][:, sl]),
           ("frame", got["frame"], want["frame"][:, sl]), ("discount", got["discount"], want["discount"][:, sl]),
           ("metrics", got["metrics"], want["metrics"][:, sl]),
           ("term_reason", tr[:, :, :A], want["term_reason"][:, sl]),
           ("safety", got["safety"][:, :, :A], want["safety"][:, sl]),
           ("agent_pos", got["agent_pos"].reshape(E, S, 2, 2)[:, :, :A], want["pos"][:, sl]),
           ("action_direction", ((fl >> 1) & 3)[:, :, :A], want["action_direction"][:, sl]),
           ("observation_direction", ((fl >> 3) & 3)[:, :, :A], want["observation_direction"][:, sl])]
  pairs += [(f, got[f].reshape(E, S, 2, spec.K)[:, :, :A], want[f][:, sl]) for f in ("reward", "cumulative")]
  if "safety2" in want:
    pairs.append(("safety2", got["safety2"][:, :, :A], want["safety2"][:, sl]))
  if views is not None:
    pairs.append(("views", np.stack(views, axis=2)[:, :, :A], want["view"][:, sl]))
  return [f for f, g, w in pairs if not _same(g, w)]


def rng_mismatch(row, state, want, s):
  """The per-env PCG64 words of an engine state [words, E] (int64) after s steps == the oracle's generator position."""
  st = state.view(np.uint64)
  off = resets(row) - 1
  return not np.array_equal(np.stack([st[3], st[4], st[5], st[6]], axis=1), want["rng"][:, s + off])


def finished_returns(step_type, cumulative):
  """step_type [E, S, A], cumulative [E, S, A*K] of steps 1 .. S-1 after a reset at step 0 -> float64 [A*K + 1]: the summed
  return vectors of the episodes that finished, and their count (the step at which every agent is done; read_returns)."""
  done = (step_type >= 2).all(axis=2)
  last = done[:, 1:] & ~done[:, :-1]
  acc = np.zeros(cumulative.shape[2] + 1)
  acc[:-1] = (cumulative[:, 1:] * last[..., None]).sum(axis=(0, 1))
  acc[-1] = last.sum()
  return acc


# ---- the launch-path matrix (GPU): shared by tests/test_launch_paths_gpu.py and tests/test_seeded_draws_gpu.py ----------------------
T, CALLS, SEED = 16, 3, 0x1A7C        # T >= step_graphs_min_T (8): the second call of a buffer is captured
AFTER = 3                             # setter tests: calls after the setter (the stale graph's direct launch, capture, replay)
PATHS = ("step_n", "step_n_side", "replay", "rollout")


def steps_of(row):
  """Steps a row's action stream covers: its step_n / replay / rollout calls; groups: CALLS step_n calls, then one rollout;
  setter tests: CALLS calls, then AFTER more."""
  return max(row["calls"], CALLS + 1, CALLS + AFTER) * T


def base_of(row):
  return row.get("base", 0)


def host_actions(spec, ids, steps, seed):
  """int8 [len(steps), len(ids)(, A)]: the package's synthetic action stream of the global env ids `ids`, restated on the host."""
  per = [philox.actions(seed, ids, steps, spec.action_lo, spec.n_actions, agent=a) for a in range(spec.A)]
  return per[0] if spec.A == 1 else np.stack(per, axis=-1)


_CASES = {}


def case(row):
  """Per row (cached by id; `row`: a row, or the id of one of ROWS): spec, inputs, the device action stream of steps_of(row) steps
  (== the host's statement over the global env ids), the oracle's arrays, and a reference engine's outputs of every step (reset,
  then one sgw_step per step) with its state after every multiple of T steps.  The reference engine itself is compared with the
  oracle at every step, and its generator position with the oracle's at every multiple of T (the multi-agent families)."""
  import torch
  from ai_safety_gridworlds_amd.specs import make_spec
  if isinstance(row, str):
    row = BY_ID[row]
  row_id = row["id"]
  if row_id in _CASES:
    return _CASES[row_id]
  spec = make_spec(row["name"], **row["kw"])
  base = base_of(row)
  inp = inputs(row, spec, row["seed"] if "seed" in row else ROWS.index(row), base=base)
  ref = make_engine(row, spec, inp, base=base)
  S = steps_of(row)
  acts = ref.fill_actions(S, SEED).clone()
  assert np.array_equal(acts.cpu().numpy(), host_actions(spec, global_ids(row["n"], base), np.arange(S), SEED)), \
      "%s: sgw_fill_actions differs from philox.actions over the global env ids" % row_id
  rec = {k: [v.clone()] for k, v in start(ref, row).items()}
  states = {}
  for t in range(S):
    for k, v in ref.step(acts[t]).items():
      rec[k].append(v.clone())
    if (t + 1) % T == 0:
      states[t + 1] = ref.get_state()[:, :row["n"]].clone()
  torch.cuda.synchronize()
  got = to_np({k: torch.stack(v) for k, v in rec.items()}, True)
  want = run_oracle(row, acts.cpu().numpy(), inp)
  c = dict(row=row, spec=spec, inp=inp, acts=acts, want=want, ref=got, states=states)
  check(c, {k: v[:, 1:] for k, v in got.items()}, 1, "sgw_step")
  if row["rng"]:
    for s, st in states.items():
      assert not rng_mismatch(row, st.cpu().numpy(), want, s), "%s sgw_step: generator position after %d steps" % (row_id, s)
  if row["oracle"] == "scalar":
    st, cum = want["step_type"][..., None], want["cumulative"]
  else:
    st, cum = got["step_type"], got["cumulative"].reshape(row["n"], S + 1, -1)
  # read_returns after the row's own calls and after the groups' CALLS step_n calls
  c["returns"] = {s: finished_returns(st[:, :s + 1], cum[:, :s + 1]) for s in {row["calls"] * T, CALLS * T}}
  assert c["returns"][row["calls"] * T][-1] > 0, "no episode ends inside the run: pick kwargs with shorter episodes"
  ref.close()
  _CASES[row_id] = c
  return c


def check(c, got, s0, label):
  """got {field: [E, S, ...]} = the outputs of steps s0 .. s0 + S - 1: equal to the oracle and to the sgw_step engine."""
  row, spec = c["row"], c["spec"]
  S = next(iter(got.values())).shape[1]
  views = split_views(spec, got["views"]) if "views" in got else None
  bad = oracle_mismatches(row, spec, got, c["want"], s0, views=views)
  assert not bad, "%s %s steps %d..%d differ from the oracle in %s" % (row["id"], label, s0, s0 + S - 1, bad)
  if label != "sgw_step":
    for k in row["outs"]:
      g, w = got[k], c["ref"][k][:, s0:s0 + S]
      assert _same(g, w), "%s %s steps %d..%d: %s differs from the sgw_step engine" % (row["id"], label, s0, s0 + S - 1, k)


def check_returns(c, r, steps, label):
  """read_returns after `steps` steps: the count of finished episodes exactly; the sums up to the order of the device's
  float64 atomic adds."""
  r, w = r.cpu().numpy(), c["returns"][steps]
  assert r[-1] == w[-1], "%s %s: %d finished episodes, the oracle has %d" % (c["row"]["id"], label, r[-1], w[-1])
  assert np.allclose(r[:-1], w[:-1], rtol=1e-12, atol=1e-9), "%s %s: returns %s, the oracle's %s" % (c["row"]["id"], label, r, w)


def run_path(row, path):
  """One of PATHS over the row's calls, from a reset: every call's outputs, the final state and read_returns."""
  import torch
  c = case(row)
  row, spec, acts = c["row"], c["spec"], c["acts"]
  row_id = row["id"]
  eng = make_engine(row, spec, c["inp"], base=base_of(row))
  start(eng, row)
  buf = torch.empty_like(acts[:T])
  torch.cuda.synchronize()
  stream = torch.cuda.Stream(DEV) if path == "step_n_side" else torch.cuda.current_stream(DEV)
  calls, n_calls = [], row["calls"]
  with torch.cuda.stream(stream):
    for k in range(n_calls):
      if path.startswith("step_n"):               # call 0: direct launches, call 1: capture + replay, call 2: replay
        buf.copy_(acts[k * T:(k + 1) * T])
        o = eng.step_n(buf, write_every=True, accumulate=True)
      elif path == "replay":
        o = eng.replay(acts[k * T:(k + 1) * T], write_every=True, accumulate=True)
      else:
        o = eng.rollout(T, SEED, step0=k * T, write_every=True, accumulate=True)
      calls.append({f: v.clone() for f, v in o.items()})
    ret = eng.read_returns()
    state = eng.get_state()[:, :row["n"]]
  torch.cuda.synchronize()
  for k, o in enumerate(calls):
    check(c, to_np(o, True), 1 + k * T, "%s call %d" % (path, k))
  assert torch.equal(state, c["states"][n_calls * T]), "%s %s: final state differs from the sgw_step engine" % (row_id, path)
  check_returns(c, ret, n_calls * T, path)
  eng.close()


def run_group(gid, members):
  """The member rows as one EngineGroup: CALLS sgw_group_step_n calls (direct, capture, replay), then one sgw_group_rollout."""
  import torch
  from ai_safety_gridworlds_amd.engine import EngineGroup
  cs = [case(m) for m in members]
  engines = [make_engine(c["row"], c["spec"], c["inp"], base=base_of(c["row"])) for c in cs]
  for c, e in zip(cs, engines):
    start(e, c["row"])
  grp = EngineGroup(engines)
  bufs = [torch.empty_like(c["acts"][:T]) for c in cs]
  torch.cuda.synchronize()
  for k in range(CALLS):                           # direct, capture, replay; the actions refilled in place
    for b, c in zip(bufs, cs):
      b.copy_(c["acts"][k * T:(k + 1) * T])
    outs = grp.step_n(bufs, write_every=True, accumulate=True)
    torch.cuda.synchronize()
    for c, o in zip(cs, outs):
      check(c, to_np(o, True), 1 + k * T, "%s group step_n call %d" % (gid, k))
  for c, e in zip(cs, engines):
    check_returns(c, e.read_returns(), CALLS * T, "%s group step_n" % gid)
    assert torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][CALLS * T]), "%s %s: state" % (gid, c["row"]["id"])
  outs = grp.rollout(T, SEED, step0=CALLS * T, write_every=True)
  torch.cuda.synchronize()
  for c, o, e in zip(cs, outs, engines):
    check(c, to_np(o, True), 1 + CALLS * T, "%s group rollout" % gid)
    assert torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][(CALLS + 1) * T]), "%s %s: state after the rollout" % (gid, c["row"]["id"])
  grp.close()
  for e in engines:
    e.close()
