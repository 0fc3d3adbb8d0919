#!/usr/bin/env python3
"""Which (action_direction_mode, observation_direction_mode) pairs of the three multi-agent families survive the turning
actions 5..8 in the reference (build container only; prints the table that DESIGN.md records).

    python tests/golden/probe_turn_pairs.py

Every pair runs in a child process of its own (a failed assert must not leave a half-stepped game behind): 40 rounds in which
every agent submits a value of 5..8 on two rounds out of three and a move on the third.  "survives" = no exception.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
FAMILIES = ("firemaker_ex_ma", "island_navigation_ex_ma", "aintelope_savanna")


def one(family, am, om):
  import tempfile
  os.chdir(tempfile.mkdtemp(prefix="sgw_probe_"))
  sys.dont_write_bytecode = True
  sys.path.insert(0, "/root/reference")
  sys.path.insert(0, os.path.join(HERE, "standins"))
  from ai_safety_gridworlds.environments.shared.rl import pycolab_interface_ma
  _orig = pycolab_interface_ma.EnvironmentMa._update_for_game_step
  def _patched(self, observations, reward, discount):      # the documented patch of the fixture generators
    if self._last_reward is None:
      self._last_reward = self._default_reward
    return _orig(self, observations, reward, discount)
  pycolab_interface_ma.EnvironmentMa._update_for_game_step = _patched
  kw = dict(action_direction_mode=am, observation_direction_mode=om, max_iterations=100)
  if family == "firemaker_ex_ma":
    from ai_safety_gridworlds.environments import firemaker_ex_ma as m
    env, agents = m.FiremakerExMa(seed=1, amount_agents=2, **kw), ['1', 'S']
  elif family == "island_navigation_ex_ma":
    from ai_safety_gridworlds.environments import island_navigation_ex_ma as m
    env, agents = m.IslandNavigationEnvironmentExMa(seed=1, level=10, **kw), ['1', '2']
  else:
    from ai_safety_gridworlds.environments.aintelope import aintelope_savanna as m
    env, agents = m.AIntelopeSavannaEnvironmentMa(seed=1, amount_agents=2, **kw), ['0', '1']
  env.reset()
  for t in range(40):
    env.step({ch: {'step': (5 + (t + i) % 4) if t % 3 else 1 + (t + i) % 4} for i, ch in enumerate(agents)})


def main():
  if len(sys.argv) == 4:
    return one(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
  for family in FAMILIES:
    for am in range(3):
      for om in range(3):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), family, str(am), str(om)], capture_output=True, text=True)
        last = p.stderr.strip().splitlines()[-1] if p.returncode else ""
        print("%-24s action mode %d observation mode %d: %s" % (family, am, om, "survives" if p.returncode == 0 else "raises  " + last[:90]))


if __name__ == "__main__":
  main()
