"""Randomised configuration cases, HIP engine vs the C oracle, for the flag-rich families (island_navigation_ex,
island_navigation_ex_ma, aintelope_savanna, firemaker_ex_ma): random levels / flags / tile amounts / map sizes / direction modes /
single-agent rounds / explicit resets; every output every step, metrics and the numpy generator position.  Used by
tests/test_fuzz_gpu.py (a bounded fixed-seed slice, in the GPU tier) and by tools/diag/fuzz_parity.py (open-ended sweeps).
A case returns (family, kwargs, True | False | reason) or None when the drawn configuration is one the reference refuses.

numeric=True also draws the numeric rule parameters and reward values (the flags tests/flag_fixtures.py pins to reference runs)
from the ranges stated in NUMERIC_*, and an observation window with four different radii where the window does not rotate
(observation_direction_mode 0).  Those draws come after every other draw of the configuration and only then: with numeric=False
a seed selects exactly the configurations it always did (tests/test_fuzz_draws.py holds their digests).  draw_only=True returns
(family, kwargs, None) once the configuration is accepted, before anything runs: what a seed selects, without a GPU."""
import numpy as np
import torch

from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec
from oracle import oracle as O, oracle_ima as OI, oracle_ma as OM, oracle_sav as OS


# numeric=True: every listed flag is drawn with probability 1/2, uniformly from its values.  The values stay inside what the
# engine accepts (specs._check_regrowth_exponent, growth limits <= 60, the packed island state's ranges or the plain state where
# a value is not integral) and include each default, values on both sides of it, and for the drink growth limit both sides of
# the constant 20 that the reference's drink drapes compare with.
_RATES = dict(EXTRACTION_RATE=[1.0, 2.5, 5.0, 7.0, 10.0, 15.0], DEFICIENCY_RATE=[-0.25, -0.5, -1.0, -1.5, -2.0],
              OVERSATIATION_LIMIT=[1.0, 2.5, 4.0, 7.0], DEFICIENCY_LIMIT=[-4.0, -7.5, -12.0, -20.0],
              DEFICIENCY_INITIAL=[-3.0, -1.5, 0.0, 1.5, 3.0], GROWTH_LIMIT=[8.0, 14.0, 20.0, 26.0, 40.0, 60.0],
              REGROWTH_EXPONENT=[1.02, 1.1, 1.25, 1.6, 2.0], AVAILABILITY_INITIAL=[0.0, 5.0, 12.0, 20.0, 22.0, 30.0])
_THRESHOLDS = dict(OVERSATIATION_THRESHOLD=[0.0, 0.5, 2.0, 3.5], DEFICIENCY_THRESHOLD=[-6.5, -3.0, -1.5, 0.0])
NUMERIC_ISLAND = {res + "_" + k: v for res in ("DRINK", "FOOD") for k, v in _RATES.items()}
NUMERIC_ISLAND_MA = dict(NUMERIC_ISLAND, **{res + "_" + k: v for res in ("DRINK", "FOOD") for k, v in _THRESHOLDS.items()})
NUMERIC_ISLAND_REWARDS = dict(     # flag -> values of its own dimension
    MOVEMENT_REWARD=[-2.0, -1.0, -0.25], FINAL_REWARD=[31.5, 50.0], DRINK_DEFICIENCY_REWARD=[-3.0, -1.0, -0.5],
    FOOD_DEFICIENCY_REWARD=[-3.0, -1.0, -0.5], DRINK_REWARD=[5.0, 11.5, 20.0], FOOD_REWARD=[5.0, 13.0, 20.0],
    GOLD_REWARD=[12.5, 40.0], SILVER_REWARD=[7.0, 30.0], DANGER_TILE_REWARD=[-50.0, -33.0, -8.0],
    THIRST_HUNGER_DEATH_REWARD=[-50.0, -17.5], DRINK_OVERSATIATION_REWARD=[-2.5, -1.0], FOOD_OVERSATIATION_REWARD=[-1.0, -0.75])
NUMERIC_SAVANNA = {k: v for k, v in NUMERIC_ISLAND_MA.items() if "DEFICIENCY_LIMIT" not in k and "AVAILABILITY_INITIAL" not in k}
NUMERIC_SAVANNA.update(
    DRINK_EXTRACTION_RATE=[0.5, 1.0, 2.0], FOOD_EXTRACTION_RATE=[0.5, 1.0, 1.5], SMALL_DRINK_EXTRACTION_RATE=[0.25, 0.5, 0.75],
    SMALL_FOOD_EXTRACTION_RATE=[0.25, 0.5, 0.75], DRINK_DEFICIENCY_RATE=[-0.5, -0.2, -0.125], FOOD_DEFICIENCY_RATE=[-0.375, -0.2, -0.125],
    GOLD_VISITS_LOG_BASE=[1.5, 2.0, 3.0], SILVER_VISITS_LOG_BASE=[1.5, 2.0, 3.0], PREDATOR_MOVEMENT_PROBABILITY=[0.0, 0.25, 0.5, 0.8, 1.0])
NUMERIC_SAVANNA_SCORES = dict(     # flag -> (its dimension, values)
    MOVEMENT_SCORE=("MOVEMENT", [-1.0, -0.25]), DRINK_SCORE=("DRINK", [11.5, 20.0]), SMALL_DRINK_SCORE=("DRINK", [4.5, 10.0]),
    FOOD_SCORE=("FOOD", [13.0, 20.0]), SMALL_FOOD_SCORE=("FOOD", [6.5, 10.0]), GOLD_SCORE=("GOLD", [12.5, 40.0]),
    SILVER_SCORE=("SILVER", [7.0, 30.0]), DANGER_TILE_SCORE=("INJURY", [-50.0, -20.5]), PREDATOR_NPC_SCORE=("INJURY", [-100.0, -40.0]),
    COOPERATION_SCORE=("COOPERATION", [60.0, 100.0]), SMALL_COOPERATION_SCORE=("COOPERATION", [25.0, 50.0]),
    DRINK_DEFICIENCY_SCORE=("DRINK_DEFICIENCY", [-1.5, -1.0]), FOOD_DEFICIENCY_SCORE=("FOOD_DEFICIENCY", [-3.0, -1.0]),
    DRINK_OVERSATIATION_SCORE=("DRINK_OVERSATIATION", [-2.5, -1.0]), FOOD_OVERSATIATION_SCORE=("FOOD_OVERSATIATION", [-1.0, -0.75]))
NUMERIC_FIREMAKER = dict(STOP_BUTTON_PRESS_EFFECT_DURATION=[0, 1, 3, 7], FIRE_CONTINUATION_PROBABILITY=[0.8, 0.9, 0.95, 1.0])
NUMERIC_FIREMAKER_REWARDS = dict(
    AGENT_MOVEMENT_REWARD=("ENERGY", [-2.0, -1.0]), AGENT_WORKSHOP_WORK_REWARD=("WORKSHOP", [7.5, 10.0]),
    AGENT_WORKSHOP_ENERGY_REWARD=("ENERGY", [-1.0, -0.5]), SUPERVISOR_MOVEMENT_REWARD=("ENERGY", [-3.0, -1.0]),
    SUPERVISOR_EXTERNAL_FIRE_REWARD=("EXTERNAL_FIRE", [-10.0, -4.5]), SUPERVISOR_TRESPASSING_REWARD=("TRESPASSING", [-2.0, -1.0]),
    SUPERVISOR_STOP_BUTTON_REWARD=("TRESPASSING", [-5.0, -1.0]), SUPERVISOR_WORKSHOP_REWARD=("TRESPASSING", [-1.0, -0.25]))


def _draw_numeric(rnd, kw, floats, rewards):
  """Into kw: each flag of `floats` {flag: values} and `rewards` {flag: values of its own dimension | (dimension, values)} with
  probability 1/2."""
  for flag, values in floats.items():
    if rnd.integers(2):
      v = values[int(rnd.integers(len(values)))]
      kw[flag] = v if isinstance(v, int) else float(v)
  for flag, values in rewards.items():
    dim, values = values if isinstance(values, tuple) else (flag, values)
    if rnd.integers(2):
      kw[flag] = {dim: float(values[int(rnd.integers(len(values)))])}


def _draw_radii(rnd, top):
  """[left, right, up, down], each 0..top, no side equal to its opposite."""
  while True:
    r = [int(v) for v in rnd.integers(0, top + 1, 4)]
    if r[0] != r[1] and r[2] != r[3]:
      return r


def island_case(rnd, E=1500, T=160, nthreads=16, numeric=False, draw_only=False):
  level = int(rnd.choice([2, 3, 4, 5, 6, 7, 8, 9]))
  kw = dict(level=level, sustainability_challenge=bool(rnd.integers(2)), thirst_hunger_death=bool(rnd.integers(2)),
            penalise_oversatiation=bool(rnd.integers(2)), use_satiation_proportional_reward=bool(rnd.integers(2)),
            max_iterations=int(rnd.integers(15, 120)))
  acts = philox.actions(int(rnd.integers(1 << 30)), np.arange(E), np.arange(T), 0, 5).T.copy()
  if numeric:
    _draw_numeric(rnd, kw, NUMERIC_ISLAND, NUMERIC_ISLAND_REWARDS)
  try:
    spec = make_spec("island_navigation_ex", **kw)
  except ValueError:
    return None
  if draw_only:
    return ("island", kw, None)
  want = O.run_streams(O.make_config("island_navigation_ex", **kw), acts, nthreads=nthreads)
  eng = BatchedEngine(spec, E, outputs=("board", "reward", "cumulative", "step_type", "metrics", "frame"))
  a = torch.from_numpy(np.ascontiguousarray(acts.T)).to("cuda:0")
  rec = {k: [eng.reset()[k].clone()] for k in ("board", "reward", "cumulative", "step_type", "metrics", "frame")}
  for t in range(T):
    o = eng.step(a[t])
    for k in rec: rec[k].append(o[k].clone())
  got = {k: torch.stack(v, 1).cpu().numpy() for k, v in rec.items()}
  eng.close()
  ok = True
  for k in ("reward", "cumulative", "step_type", "frame", "metrics"):
    g, w = got[k].reshape(want[k].shape) if k != "metrics" else got[k][..., :spec.M], want[k]
    ok &= bool(((g == w) | ((g != g) & (w != w))).all())
  ok &= bool((got["board"].reshape(want["board"].shape) == want["board"]).all())
  return ("island", kw, ok)

def ma_case(rnd, which, E=800, T=150, nthreads=16, strict=False, numeric=False, draw_only=False):
  seed = int(rnd.integers(1 << 30))
  modes = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 2)][int(rnd.integers(6))]     # (action, observation) direction modes
  n_act = 9 if modes[0] == 2 else 5                          # mode 2: the turning actions 5-8 join the action set
  actions = np.stack([philox.actions(seed, np.arange(E), np.arange(T), 0, n_act, agent=a) for a in range(2)], axis=-1)
  actions = np.transpose(actions, (1, 0, 2)).astype(np.int8).copy()
  for t in rnd.choice(T, 3, replace=False): actions[:, int(t), :] = -128
  if rnd.integers(2):                                      # some single-agent rounds
    for t in range(0, T, 4):
      if actions[0, t, 0] != -128: actions[:, t, int(rnd.integers(2))] = -1
  rng = np.stack([OM.rng_state_words(int(seed % 100000) + e) for e in range(E)])
  if which == "ima":
    kw = dict(level=int(rnd.choice([2, 3, 4, 5, 6, 7, 8, 9, 10])), sustainability_challenge=bool(rnd.integers(2)),
              penalise_oversatiation=bool(rnd.integers(2)), use_satiation_proportional_reward=bool(rnd.integers(2)),
              map_randomization_frequency=int(rnd.integers(4)), action_direction_mode=modes[0],
              observation_direction_mode=modes[1], max_iterations=int(rnd.integers(12, 80)))
    if kw["map_randomization_frequency"] >= 1 and rnd.integers(3) == 0:      # resized island: up to 128 cells (> 64: the 8-word map kernels)
      w = int(rnd.integers(4, 17)); kw.update(map_width=w, map_height=int(rnd.integers(4, min(13, 128 // w + 1))))
    name, Or = "island_navigation_ex_ma", OI
  else:
    two = bool(rnd.integers(2))
    kw = dict(amount_agents=2 if two else 1, sustainability_challenge=bool(rnd.integers(2)), penalise_oversatiation=bool(rnd.integers(2)),
              use_satiation_proportional_reward=bool(rnd.integers(2)), map_randomization_frequency=int(rnd.integers(1, 4)),
              amount_food_patches=int(rnd.integers(1, 4)), amount_drink_holes=int(rnd.integers(0, 3)), amount_small_food_patches=int(rnd.integers(0, 3)),
              amount_small_drink_holes=int(rnd.integers(0, 3)), amount_gold_deposits=int(rnd.integers(0, 4)), amount_silver_deposits=int(rnd.integers(0, 4)),
              amount_water_tiles=int(rnd.integers(0, 5)), amount_predators=int(rnd.integers(0, 5)), max_iterations=int(rnd.integers(20, 120)),
              observation_radius=[2, 2, 2, 2], action_direction_mode=modes[0], observation_direction_mode=modes[1])
    if rnd.integers(3) == 0: kw.update(map_width=int(rnd.integers(7, 14)), map_height=int(rnd.integers(7, 13)))
    if not two: actions[:, :, 1] = np.where(actions[:, :, 0:1].repeat(1, 2)[:, :, 0] == -128, actions[:, :, 1], 0)
    name, Or = "aintelope_savanna", OS
  if numeric:
    if which == "ima":
      _draw_numeric(rnd, kw, NUMERIC_ISLAND_MA, {k: v for k, v in NUMERIC_ISLAND_REWARDS.items()
                                                 if k not in ("FINAL_REWARD", "THIRST_HUNGER_DEATH_REWARD")})
    else:
      _draw_numeric(rnd, kw, NUMERIC_SAVANNA, NUMERIC_SAVANNA_SCORES)
    if modes[1] == 0:
      kw["observation_radius"] = _draw_radii(rnd, 4)
  try:
    spec = make_spec(name, **kw)
  except (ValueError, NotImplementedError, AssertionError, RuntimeError):
    return None
  if draw_only:
    return (which, kw, None)
  if name == "aintelope_savanna" and kw["amount_agents"] == 1:
    actions[:, :, 0] = np.where(actions[:, :, 0] == -1, 0, actions[:, :, 0])
  try:
    want = Or.run_streams(Or.make_config(**kw), actions, rng, nthreads=nthreads)
  except ValueError as ex:
    return (which, kw, "oracle refused: %s" % ex)
  from ai_safety_gridworlds_amd.engine import fused_views
  fused = fused_views(spec)
  outs = ("board", "reward", "cumulative", "step_type", "frame", "metrics", "agent_pos", "agent_flags") + (("views",) if fused else ())
  eng = BatchedEngine(spec, E, outputs=outs); eng.set_rng_state(rng)
  a = torch.from_numpy(np.ascontiguousarray(np.transpose(actions, (1, 0, 2)))).to("cuda:0")
  rec = {k: [] for k in outs}
  views_ok = [True]
  windows = []
  def grab(o):
    for k in outs: rec[k].append(o[k].clone())
    if numeric:      # the windows themselves against the oracle's (lopsided radii: [left, right, up, down] -> rows x columns)
      windows.append(torch.stack(list(eng.agent_views())[:len(spec.agent_chars)], 1).clone())
    # the windows written by the round's launch == the separate window kernel on the same board (rot90-ed by the observation direction)
    if fused:
      for f, w in zip(eng.split_views(o["views"]), eng.agent_views()):
        views_ok[0] &= bool(torch.equal(f, w))
  grab(eng.reset()); grab(eng.reset())
  for t in range(T):
    grab(eng.reset() if actions[0, t, 0] == -128 else eng.step(a[t]))
  st = eng.get_state()[:, :E].cpu().numpy().view(np.uint64)
  got = {k: torch.stack(v, 1).cpu().numpy() for k, v in rec.items()}
  eng.close()
  A = want["step_type"].shape[2]
  S = T + 2
  # Rounds on a FINISHED episode: the agents that count are the DEAD ones when there is one (the reference raises for a LAST
  # agent next to a DEAD one), everybody otherwise; with none of them submitted nothing resets and LAST turns into DEAD.
  # Engine and oracle follow the same rule; `strict` as 4th argument leaves such streams out of the comparison
  done_before = (want["step_type"][:, 1:S - 1] >= 2).all(axis=2)                      # [E, T]: status when tick t is submitted
  partial = (actions[:, :, :A] == -1).any(axis=2)
  valid = ~(done_before & partial).any(axis=1) if strict else np.ones(E, bool)
  v = valid
  ok = views_ok[0] and bool((got["board"][v, 1:].reshape(want["board"][v, 1:].shape) == want["board"][v, 1:]).all())
  ok &= bool((got["step_type"][v, 1:, :A] == want["step_type"][v, 1:]).all())
  g = got["reward"][v, 1:].reshape(int(v.sum()), S - 1, 2, spec.K)[:, :, :A]; ok &= bool((g == want["reward"][v, 1:]).all())
  g = got["cumulative"][v, 1:].reshape(int(v.sum()), S - 1, 2, spec.K)[:, :, :A]; ok &= bool((g == want["cumulative"][v, 1:]).all())
  g, w = got["metrics"][v, 1:], want["metrics"][v, 1:]; ok &= bool(((g == w) | ((g != g) & (w != w))).all())
  rngw = np.stack([st[3], st[4], st[5], st[6]], axis=1); ok &= bool((rngw[v] == want["rng"][v, -1]).all())
  if numeric:
    g, w = torch.stack(windows, 1).cpu().numpy()[v, 1:, :A], want["view"][v, 1:]
    ok &= g.shape == w.shape and bool((g == w).all())
  return (which, dict(kw, _valid_streams=int(v.sum())), ok)


def firemaker_case(rnd, E=400, T=120, nthreads=16, numeric=False, draw_only=False):
  """firemaker_ex_ma: agent set, fire probabilities, episode length, action-order shuffle; engine vs the multi-agent oracle incl.
  the windows written by the step launch and the generator position."""
  seed = int(rnd.integers(1 << 30))
  kw = dict(amount_agents=int(rnd.integers(1, 4)), max_iterations=int(rnd.integers(20, 200)),
            FIRE_SPREAD_PROBABILITY_AT_DISTANCE_ONE=float(rnd.choice([0.01, 0.02, 0.05, 0.08])),
            FIRE_CONTINUATION_PROBABILITY=float(rnd.choice([0.9, 0.95, 0.97])))
  adm, odm = [(0, 0), (0, 0), (1, 1), (2, 2), (2, 0), (1, 0), (0, 1)][int(rnd.integers(7))]      # the combinations the reference survives
  kw.update(action_direction_mode=adm, observation_direction_mode=odm)
  kw["FIRE_SPREAD_EXCLUSIVE_MAX_DISTANCE"] = float(rnd.choice([3.0, 3.0, 3.0, 2.5, 3.5, 4.0, 4.5, 5.0]))      # > 3: the WIDE kernels
  actions = np.stack([philox.actions(seed, np.arange(E), np.arange(T), 0, 9 if adm == 2 else 5, agent=a) for a in range(3)], axis=-1)
  actions = np.transpose(actions, (1, 0, 2)).copy()
  rng = np.stack([OM.rng_state_words(int(seed % 100000) + e) for e in range(E)])
  if numeric:
    _draw_numeric(rnd, kw, NUMERIC_FIREMAKER, NUMERIC_FIREMAKER_REWARDS)
    if odm == 0:
      kw.update(agent_observation_radius=_draw_radii(rnd, 4), supervisor_observation_radius=_draw_radii(rnd, 8))
  spec = make_spec("firemaker_ex_ma", **kw)
  if draw_only:
    return ("firemaker", kw, None)
  want = OM.run_streams(OM.make_config(**kw), actions, rng, nthreads=nthreads)
  outs = ("board", "reward", "cumulative", "step_type", "frame", "metrics", "agent_pos", "agent_flags", "views")
  eng = BatchedEngine(spec, E, outputs=outs); eng.set_rng_state(rng)
  a = torch.from_numpy(np.ascontiguousarray(np.transpose(actions, (1, 0, 2)))).to("cuda:0")
  rec = {k: [eng.reset()[k].clone()] for k in outs}
  for t in range(T):
    o = eng.step(a[t])
    for k in outs: rec[k].append(o[k].clone())
  st = eng.get_state()[:, :E].cpu().numpy().view(np.uint64)
  got = {k: torch.stack(v, 1).cpu() for k, v in rec.items()}
  views = [w.numpy() for w in eng.split_views(got["views"])]
  got = {k: v.numpy() for k, v in got.items()}
  eng.close()
  slots = list(spec.agent_slots)
  ok = bool((got["board"] == want["board"]).all()) and bool((got["frame"] == want["frame"]).all())
  for f in ("step_type", "reward", "cumulative"):
    ok &= bool((got[f][:, :, slots] == want[f][:, :, slots]).all())
  ok &= bool((got["agent_pos"][:, :, slots] == want["pos"][:, :, slots]).all())
  ok &= bool((((got["agent_flags"] >> 1) & 3)[:, :, slots] == want["action_direction"][:, :, slots]).all())
  ok &= bool((((got["agent_flags"] >> 3) & 3)[:, :, slots] == want["observation_direction"][:, :, slots]).all())
  for q in slots:
    ok &= bool((views[q] == (want["view_worker"][:, :, q] if q < 2 else want["view_supervisor"])).all())
  ok &= bool((np.stack([st[3], st[4], st[5], st[6]], axis=1) == want["rng"][:, -1]).all())
  return ("firemaker", kw, ok)
