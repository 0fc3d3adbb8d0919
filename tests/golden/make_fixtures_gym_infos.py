#!/usr/bin/env python3
"""gym_firemaker_infos.npz: what GridworldGymEnv("firemaker_ex_ma", agent_character=...) returns over a reset and a dozen steps
(tests/facade_infos.py), recorded on an MI355X from this project's own facade.

    python tests/golden/make_fixtures_gym_infos.py [out.npz]

Recorded in front of the move of the layer-derived info entries into helpers/_shared.py; regenerate only for a change
that is meant to alter what the facade returns.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np                     # noqa: E402
from tests import facade_infos         # noqa: E402


def main():
  out = {}
  for agent in facade_infos.AGENTS:
    out.update(facade_infos.record(agent))
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "gym_firemaker_infos.npz")
  np.savez_compressed(path, **out)
  print("%d arrays -> %s" % (len(out), path))


if __name__ == "__main__":
  main()
