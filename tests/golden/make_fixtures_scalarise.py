#!/usr/bin/env python3
"""Golden values for scalarise=True, produced by RUNNING the reference (build container only).

    python tests/golden/make_fixtures_scalarise.py

For each config the reference's L4 environment is run twice over the same Philox action tape (ai_safety_gridworlds_amd/philox.py,
the stream the other generators use): once with scalarise=False and once with scalarise=True, T steps with an explicit reset in
the middle.  Stored as data in tests/golden/scalarise_<config>.npz, one row per returned timestep (the first reset, every step,
the explicit reset):

    actions int8 [T], reset_at
    frame int32 [S], step_type uint8 [S], reward_none bool [S]        (the same in both runs; the generator asserts it)
    reward / cumulative_reward / average_reward float64 [S, K]        of the scalarise=False run
    scalar_reward / scalar_cumulative_reward / scalar_average_reward float64 [S]    of the scalarise=True run
    last_performance / overall_performance float64 [S, K], scalar_last_performance / scalar_overall_performance float64 [S]:
        get_last_performance() / get_overall_performance() after that timestep, NaN while the reference returns None

Two-agent configs (firemaker_ex_ma, aintelope_savanna; the constructions, seeds and the one documented patch of make_fixtures_ma.py /
make_fixtures_sav.py): the same arrays with an agent axis in the batched framework's column layout -- [S, A, K] / [S, A], the
columns of absent agents and the dimensions past an agent's own left at zero -- plus k_agent [A], the generator state to start
from (rng_state uint64 [4]) and constructor_resets (engine resets before the first recorded one).  The reference's MoMa
get_last_performance raises under scalarise (safety_game_moma.py:1175), so these files carry get_overall_performance only.

The scalar columns are Python's sum() over the vector columns as the interpreter that ran this file computes it: a
left-to-right chain of IEEE additions from 0 up to Python 3.11 (3.12 compensates the sum; the generator refuses to run there).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

# name -> (family of make_fixtures.make_env, ctor kwargs, T steps, explicit reset before step, action lo, n_actions)
CONFIGS = {
    "island_L9": ("island_ex", dict(level=9), 60, 23, 0, 5),
    # boat_race_ex ends an episode at max_iterations = 100 only: long enough for one LAST after the explicit reset
    "boat_ex_L3": ("boat_race_ex", dict(level=3), 130, 23, 0, 5),
}


def run(np, MF, family, kw, acts, reset_at, scalarise):
  env, _ = MF.make_env(family, dict(kw, scalarise=scalarise))
  K = len(env.enabled_reward_dimension_keys)
  rows = dict(frame=[], step_type=[], reward_none=[], reward=[], cumulative=[], average=[], last=[], overall=[])
  nan = np.float64("nan") if scalarise else np.full(K, np.nan)

  def record(ts):
    rows["frame"].append(env.current_game.the_plot.frame)
    rows["step_type"].append(int(ts.step_type))
    rows["reward_none"].append(ts.reward is None)
    rows["reward"].append(np.zeros(() if scalarise else K) if ts.reward is None else np.asarray(ts.reward, np.float64))
    rows["cumulative"].append(np.asarray(ts.observation["cumulative_reward"], np.float64))
    rows["average"].append(np.asarray(ts.observation["average_reward"], np.float64))
    lp, op = env.get_last_performance(default=None), env.get_overall_performance(default=None)
    rows["last"].append(nan if lp is None else np.asarray(lp, np.float64))
    rows["overall"].append(nan if op is None else np.asarray(op, np.float64))

  record(env.reset())
  for t in range(len(acts)):
    if t == reset_at:
      record(env.reset())
    record(env.step(int(acts[t])))
  out = {k: np.asarray(v) for k, v in rows.items()}
  for k in ("reward", "cumulative", "average", "last", "overall"):
    assert out[k].shape == ((len(acts) + 2,) if scalarise else (len(acts) + 2, K)), (k, out[k].shape)
  return out, list(env.enabled_reward_dimension_keys)


RICH = dict(amount_predators=2, amount_water_tiles=3, amount_gold_deposits=2, amount_silver_deposits=2,
            amount_small_food_patches=2, amount_drink_holes=2, amount_small_drink_holes=1)
# name -> (family, ctor kwargs, env seed, T, explicit reset before step, agent characters, their columns, A)
MA_CONFIGS = {
    "firemaker_a2": ("firemaker_ex_ma", dict(amount_agents=2, FIRE_SPREAD_PROBABILITY_AT_DISTANCE_ONE=0.03, max_iterations=25),
                     1000, 60, 23, ['1', 'S'], [0, 2], 3),
    "savanna_a2": ("aintelope_savanna", dict(amount_agents=2, sustainability_challenge=True, penalise_oversatiation=True,
                                             max_iterations=30, observation_radius=[2, 2, 2, 2], **RICH),
                   2000, 60, 23, ['0', '1'], [0, 1], 2),
}


def _words(st):
  mask = (1 << 64) - 1
  return [st['state']['state'] >> 64, st['state']['state'] & mask, st['state']['inc'] >> 64, st['state']['inc'] & mask]


def run_ma(np, family, kw, seed, acts, reset_at, agents, slots, A, scalarise):
  if family == "firemaker_ex_ma":
    from ai_safety_gridworlds.environments import firemaker_ex_ma as m
    env = m.FiremakerExMa(seed=seed, scalarise=scalarise, **kw)
    rng_state, ctor_resets = _words(env.environment_data['np_random'].bit_generator.state), 0
  else:
    from gymnasium.utils import seeding
    from ai_safety_gridworlds.environments.aintelope import aintelope_savanna as m
    m.AIntelopeSavannaEnvironmentMa(seed=1, **kw)        # the first construction in a process reseeds differently (make_fixtures_sav.py)
    env = m.AIntelopeSavannaEnvironmentMa(seed=seed, scalarise=scalarise, **kw)
    rng_state, ctor_resets = _words(seeding.np_random(seed)[0].bit_generator.state), 1
  ks = [0] * A
  for ch, q in zip(agents, slots):
    ks[q] = len(env.enabled_agents_reward_dimensions[ch])
  K = max(ks)
  rows = dict(frame=[], step_type=[], reward_none=[], reward=[], cumulative=[], average=[], overall=[])

  def per_agent(d, fill):
    out = np.full((A,) if scalarise else (A, K), fill, np.float64)
    for ch, q in zip(agents, slots):
      if d is not None and d.get(ch) is not None:
        v = np.asarray(d[ch], np.float64)
        if scalarise:
          out[q] = v
        else:
          out[q] = 0.0
          out[q, :len(v)] = v
    return out

  def record(ts):
    rows["frame"].append(env.current_game.the_plot.frame)
    st = np.zeros(A, np.uint8)
    for ch, q in zip(agents, slots):
      st[q] = int(ts.step_type[ch])
    rows["step_type"].append(st)
    rows["reward_none"].append(ts.reward is None)
    rows["reward"].append(per_agent(ts.reward, 0.0))
    rows["cumulative"].append(per_agent(ts.observation["cumulative_reward"], 0.0))
    rows["average"].append(per_agent(ts.observation["average_reward"], 0.0))
    op = env.get_overall_performance(default=None)
    rows["overall"].append(per_agent(op, np.nan) if op is not None else np.full((A,) if scalarise else (A, K), np.nan))

  record(env.reset())
  for t in range(len(acts)):
    if t == reset_at:
      record(env.reset())
    record(env.step({ch: {"step": int(acts[t, q])} for ch, q in zip(agents, slots)}))
  return {k: np.asarray(v) for k, v in rows.items()}, ks, rng_state, ctor_resets


def _ma_actions(np, MF, philox, T, A):
  return np.stack([philox.actions(MF.SEED, np.arange(1), np.arange(T), 0, 5, agent=a)[:, 0] for a in range(A)], axis=-1).astype(np.int8)


def ma_child(np, MF, philox, name, scalarise, out_path):
  """One run in a process of its own: the reference keeps episode and layout counters in class attributes, so a second env of one
  process does not repeat the first; two fresh processes with the same history do."""
  from ai_safety_gridworlds.environments.shared.rl import pycolab_interface_ma
  _orig = pycolab_interface_ma.EnvironmentMa._update_for_game_step

  def _patched(self, observations, reward, discount):      # the documented patch of make_fixtures_ma.py
    if self._last_reward is None:
      self._last_reward = self._default_reward
    return _orig(self, observations, reward, discount)
  pycolab_interface_ma.EnvironmentMa._update_for_game_step = _patched
  family, kw, seed, T, reset_at, agents, slots, A = MA_CONFIGS[name]
  rows, ks, rng_state, ctor_resets = run_ma(np, family, kw, seed, _ma_actions(np, MF, philox, T, A), reset_at, agents, slots, A, scalarise)
  np.savez(out_path, ks=np.array(ks), rng_state=np.array(rng_state, np.uint64), ctor_resets=np.array(ctor_resets), **rows)


def main_ma(np, MF, philox):
  import subprocess
  import tempfile
  tmp = tempfile.mkdtemp(prefix="sgw_fixtures_ma_")
  for name, (family, kw, seed, T, reset_at, agents, slots, A) in MA_CONFIGS.items():
    acts = _ma_actions(np, MF, philox, T, A)
    runs = []
    for flag in (0, 1):
      out = os.path.join(tmp, "%s_%d.npz" % (name, flag))
      subprocess.check_call([sys.executable, os.path.abspath(__file__), "--ma-run", name, str(flag), out],
                            env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
      with np.load(out) as z:
        runs.append({k: z[k] for k in z.files})
    vec, sca = runs
    ks, rng_state, ctor_resets = vec["ks"].tolist(), vec["rng_state"].tolist(), int(vec["ctor_resets"])
    assert ks == sca["ks"].tolist() and rng_state == sca["rng_state"].tolist()
    for k in ("frame", "step_type", "reward_none"):
      assert (vec[k] == sca[k]).all(), (name, k)
    n_last = int((vec["step_type"][:, slots] == 2).all(axis=1).sum())
    assert n_last >= 1, "%s: no episode ends on this tape" % name
    rec = dict(actions=acts, reset_at=np.array(reset_at), frame=vec["frame"].astype(np.int32), step_type=vec["step_type"],
               reward_none=vec["reward_none"].astype(np.bool_),
               reward=vec["reward"], cumulative_reward=vec["cumulative"], average_reward=vec["average"],
               scalar_reward=sca["reward"], scalar_cumulative_reward=sca["cumulative"], scalar_average_reward=sca["average"],
               overall_performance=vec["overall"], scalar_overall_performance=sca["overall"],
               k_agent=np.array(ks, np.int32), rng_state=np.array(rng_state, np.uint64), constructor_resets=np.array(ctor_resets),
               meta_family=np.array(family), meta_kwargs=np.array(repr(sorted(kw.items()))), meta_agents=np.array("|".join(agents)),
               meta_slots=np.array(slots, np.int32), meta_seed=np.array(seed))
    MF.save_reproducibly(np, os.path.join(HERE, "scalarise_%s.npz" % name), rec)
    d = (vec["frame"] + 1.0)[:, None]
    naive = vec["cumulative"].sum(axis=2) / d
    print("%-12s k_agent=%s rows=%d LAST=%d nonzero rewards=%d rows where sum(cumulative) / (frame + 1) != scalar average: %d" % (
        name, ks, len(vec["frame"]), n_last, int((sca["reward"] != 0).sum()), int((naive != sca["average"]).sum())))


def main():
  import tempfile
  if sys.version_info >= (3, 12):
    sys.exit("Python >= 3.12 compensates sum() over floats; the fixtures pin the plain left-to-right sum (run under <= 3.11)")
  os.chdir(tempfile.mkdtemp(prefix="sgw_fixtures_"))
  import make_fixtures as MF
  MF._setup_path()
  import numpy as np
  from ai_safety_gridworlds_amd import philox
  if sys.argv[1:2] == ["--ma-run"]:
    return ma_child(np, MF, philox, sys.argv[2], bool(int(sys.argv[3])), sys.argv[4])
  for name, (family, kw, T, reset_at, lo, n_act) in CONFIGS.items():
    acts = philox.actions(MF.SEED, np.arange(1), np.arange(T), lo, n_act)[:, 0].astype(np.int8)
    vec, dims = run(np, MF, family, kw, acts, reset_at, False)
    sca, dims2 = run(np, MF, family, kw, acts, reset_at, True)
    assert dims == dims2
    for k in ("frame", "step_type", "reward_none"):
      assert (vec[k] == sca[k]).all(), (name, k)
    n_last = int((vec["step_type"] == 2).sum())
    assert n_last >= 1, "%s: no episode ends on this tape" % name
    rec = dict(actions=acts, reset_at=np.array(reset_at), frame=vec["frame"].astype(np.int32), step_type=vec["step_type"].astype(np.uint8),
               reward_none=vec["reward_none"].astype(np.bool_),
               reward=vec["reward"], cumulative_reward=vec["cumulative"], average_reward=vec["average"],
               scalar_reward=sca["reward"], scalar_cumulative_reward=sca["cumulative"], scalar_average_reward=sca["average"],
               last_performance=vec["last"], overall_performance=vec["overall"],
               scalar_last_performance=sca["last"], scalar_overall_performance=sca["overall"],
               meta_family=np.array(family), meta_kwargs=np.array(repr(sorted(kw.items()))), meta_dim_names=np.array("|".join(dims)))
    MF.save_reproducibly(np, os.path.join(HERE, "scalarise_%s.npz" % name), rec)
    naive = vec["cumulative"].sum(axis=1) / (vec["frame"] + 1.0)
    print("%-12s K=%d rows=%d LAST=%d rows where sum(cumulative) / (frame + 1) != scalar average: %d" % (
        name, len(dims), len(vec["frame"]), n_last, int((naive != sca["average"]).sum())))
  main_ma(np, MF, philox)


if __name__ == "__main__":
  main()
