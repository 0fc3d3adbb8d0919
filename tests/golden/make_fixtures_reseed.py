#!/usr/bin/env python3
"""Golden fixture for RESEEDING resets of island_navigation_ex_ma, produced by RUNNING the reference (build container only).

    python tests/golden/make_fixtures_reseed.py

Same rules and stand-ins as make_fixtures_ima.py (data only; the one documented patch).  One env per constructor seed 2000 + e,
map randomisation once per episode, three SEGMENTS per env, each in the stream protocol of make_fixtures_ima.py:

  segment 0  slot 0 = state after the CONSTRUCTOR (generator words and the map it drew), slot 1 = env.reset(), then T rounds
  segment 1  slot 0 = env.reset(options={"env_layout_seed": 2}),                         slot 1 = env.reset(), then T rounds
  segment 2  slot 0 = env.reset(env_layout_seed=3, seed=2**32 + 77 + e),                 slot 1 = env.reset(), then T rounds

`env_seed[e, s]` is get_env_seed() right after slot 0 of segment s.  The class is constructed once, to throw away, before EVERY
recorded env: the first construction in a process re-seeds its generator after the constructor drew the map
(safety_game_moma.py:353-390), and so does any construction that follows a reset which moved the process-wide env_layout_seed
away from 1 -- the throw-away construction takes that re-seeding on itself and leaves env_layout_seed at 1.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SEED = 0x5AFE
NAME = "reseed_ima_L10_rand3"
KW = dict(level=10, map_randomization_frequency=3, max_iterations=8)
E, T, SEG, A = 3, 12, 3, 2
AGENTS = ['1', '2']


def main():
  import tempfile
  os.chdir(tempfile.mkdtemp(prefix="sgw_fixtures_"))      # the reference's step logger writes ./logs/*.csv
  sys.dont_write_bytecode = True
  sys.path.insert(0, "/root/reference")
  sys.path.insert(0, os.path.join(HERE, "standins"))
  sys.path.insert(0, REPO)
  import numpy as np
  from ai_safety_gridworlds_amd import philox
  from ai_safety_gridworlds.environments.shared.rl import pycolab_interface_ma

  _orig = pycolab_interface_ma.EnvironmentMa._update_for_game_step
  def _patched(self, observations, reward, discount):      # the documented patch
    if self._last_reward is None:
      self._last_reward = self._default_reward
    return _orig(self, observations, reward, discount)
  pycolab_interface_ma.EnvironmentMa._update_for_game_step = _patched
  from ai_safety_gridworlds.environments import island_navigation_ex_ma as m

  def words(st):
    mask = (1 << 64) - 1
    return [st['state']['state'] >> 64, st['state']['state'] & mask, st['state']['inc'] >> 64, st['state']['inc'] & mask]

  S = T + 2
  acts = np.stack([philox.actions(SEED, np.arange(E), np.arange(SEG * T), 0, 5, agent=a) for a in range(A)], axis=-1)   # [SEG*T, E, A]
  acts = np.transpose(acts, (1, 0, 2)).astype(np.int8).reshape(E, SEG, T, A).copy()
  rec = None
  for e in range(E):
    m.IslandNavigationEnvironmentExMa(seed=1, level=9)     # thrown away (see the module docstring)
    seed = 2000 + e
    env = m.IslandNavigationEnvironmentExMa(seed=seed, **KW)
    art0 = env.environment_data['ascii_art']
    H, W = len(art0), len(art0[0])
    if rec is None:
      dims = list(env.enabled_agents_reward_dimensions['1'])
      labels = list(env.environment_data["metrics_labels"])
      K, M = len(dims), len(labels)
      rec = dict(
          actions=acts, seeds=np.zeros(E, np.int64), env_seed=np.zeros((E, SEG), np.int64),
          step_type=np.zeros((E, SEG, S, A), np.uint8), reward=np.zeros((E, SEG, S, A, K)), reward_none=np.zeros((E, SEG, S), bool),
          cumulative=np.zeros((E, SEG, S, A, K)), discount=np.full((E, SEG, S), np.nan), term_reason=np.full((E, SEG, S, A), -1, np.int8),
          frame=np.zeros((E, SEG, S), np.int32), board=np.zeros((E, SEG, S, H, W), np.uint8), metrics=np.zeros((E, SEG, S, M)),
          pos=np.zeros((E, SEG, S, A, 2), np.int32), action_direction=np.zeros((E, SEG, S, A), np.int8),
          observation_direction=np.zeros((E, SEG, S, A), np.int8), safety=np.zeros((E, SEG, S, A), np.int32),
          rng=np.zeros((E, SEG, S, 4), np.uint64), rng_has_uint32=np.zeros((E, SEG, S), np.uint8), rng_uinteger=np.zeros((E, SEG, S), np.uint32),
          view=np.zeros((E, SEG, S, A, 5, 5), np.uint8))
    rec["seeds"][e] = seed

    def record(s, t, ts):
      st = env.environment_data['np_random'].bit_generator.state
      rec["rng"][e, s, t] = words(st)
      rec["rng_has_uint32"][e, s, t] = st['has_uint32']; rec["rng_uinteger"][e, s, t] = st['uinteger']
      rec["frame"][e, s, t] = env.current_game.the_plot.frame
      rec["board"][e, s, t] = env.current_game._board.board
      for ai, ch in enumerate(AGENTS):
        sp = env.environment_data['agent_sprite'][ch]
        rec["pos"][e, s, t, ai] = [sp.position.row, sp.position.col]
        rec["action_direction"][e, s, t, ai] = int(sp.action_direction)
        rec["observation_direction"][e, s, t, ai] = int(sp.observation_direction)
        rec["safety"][e, s, t, ai] = int(env.environment_data['safety_' + ch])
        rec["step_type"][e, s, t, ai] = int(ts.step_type[ch])
        rec["reward"][e, s, t, ai] = [float(ts.observation["reward_dict"][ch][d]) for d in dims]
        rec["cumulative"][e, s, t, ai] = np.asarray(ts.observation["cumulative_reward"][ch], dtype=np.float64)
        tr = ts.observation["extra_observations"].get("termination_reason")
        if tr is not None:
          v = tr[ch]
          v = v[ch] if isinstance(v, dict) else v          # the reference nests the whole dict per agent
          rec["term_reason"][e, s, t, ai] = int(v)
      rec["reward_none"][e, s, t] = ts.reward is None
      if ts.discount is not None:
        rec["discount"][e, s, t] = ts.discount
      md = ts.observation["metrics_dict"]
      rec["metrics"][e, s, t] = [float('nan') if md.get(k) is None else float(md[k]) for k in labels]
      per = env.agent_perspectives(env.current_game._board.board)
      for ai, ch in enumerate(AGENTS):
        rec["view"][e, s, t, ai] = per[ch]

    for s in range(SEG):
      if s == 0:                                           # the constructor dropped its game: the generator and the map remain
        st0 = env.environment_data['np_random'].bit_generator.state
        rec["rng"][e, 0, 0] = words(st0); rec["rng_has_uint32"][e, 0, 0] = st0['has_uint32']; rec["rng_uinteger"][e, 0, 0] = st0['uinteger']
        rec["board"][e, 0, 0] = np.array([[ord(c) for c in row] for row in art0], np.uint8)
      elif s == 1:
        record(s, 0, env.reset(options={"env_layout_seed": 2}))
      else:
        record(s, 0, env.reset(env_layout_seed=3, seed=2**32 + 77 + e))
      rec["env_seed"][e, s] = env.get_env_seed()
      ts = env.reset()
      record(s, 1, ts)
      for t in range(T):
        stp = [int(ts.step_type[ch]) for ch in AGENTS]
        # level 10 has no water and no goal: both agents end together, and the round after is the auto-reset with both submitted
        assert all(v in (2, 3) for v in stp) == any(v in (2, 3) for v in stp) and 3 not in stp
        ts = env.step({ch: {'step': int(acts[e, s, t, ai])} for ai, ch in enumerate(AGENTS)})
        record(s, t + 2, ts)
  meta = dict(name=NAME, family="island_navigation_ex_ma", kwargs=repr(sorted(KW.items())), E=E, T=T, segments=SEG, seed=SEED,
              metric_labels="|".join(labels), dim_names="|".join(dims))
  rec.update({"meta_" + k: np.array(v) for k, v in meta.items()})
  np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **rec)
  st = rec["step_type"]
  print("%s E=%d T=%d segments=%d K=%d M=%d LAST=%d env_seed=%s distinct maps=%d" % (
      NAME, E, T, SEG, K, M, int((st == 2).sum()), rec["env_seed"].tolist(),
      len({rec["board"][e, s, t].tobytes() for e in range(E) for s in range(SEG) for t in range(S) if rec["frame"][e, s, t] == 0})))


if __name__ == "__main__":
  main()
