"""BatchedEngine.layer_coords / agent_layer_coords against what the reference itself put in info_observation_coordinates and
info_agent_observation_coordinates (the `coords_json` / `agent_coords_json` entries of tests/golden/wrapper_island_L9.npz and
tests/golden/zoo_island_ma_L9.npz, recorded by running the reference): the recorded action streams are replayed through the
one-env facades and the kernels run on the facade's engine at every step."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lists(counts, coords):
  """(counts [L], coords [L, cap, 2]) of one env -> a list per layer of [a, b] pairs."""
  counts, coords = counts.cpu().numpy(), coords.cpu().numpy()
  assert (counts <= coords.shape[1]).all(), "the default cap is lossless"
  return [coords[l, :counts[l]].tolist() for l in range(len(counts))]


def test_layer_coords_match_the_wrapper_fixture():
  from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldGymEnv
  fx = np.load(os.path.join(GOLDEN, "wrapper_island_L9.npz"))
  acts, reset_at = fx["actions"], int(fx["reset_at"])
  coords = json.loads(str(fx["coords_json"]))
  env = GridworldGymEnv("island_navigation_ex", level=9)
  eng, chars = env._env.engine, list(env._env.spec.layer_chars)
  k = [0]

  def check():
    i = k[0]; k[0] += 1
    got = dict(zip(chars, _lists(*(t[0] for t in eng.layer_coords()))))
    assert {c: sorted(map(tuple, v)) for c, v in got.items()} == {c: sorted(map(tuple, v)) for c, v in coords[i].items()}, i

  env.reset(); check()
  for t in range(len(acts)):
    if t == reset_at:
      env.reset(); check()
    env.step(int(acts[t])); check()
  assert k[0] == len(coords)
  env.close()


def test_layer_and_agent_coords_match_the_zoo_fixture():
  from ai_safety_gridworlds_amd.helpers import gridworld_zoo_parallel_env as Z
  fx = np.load(os.path.join(GOLDEN, "zoo_island_ma_L9.npz"))
  coords, agent_coords = json.loads(str(fx["coords_json"])), json.loads(str(fx["agent_coords_json"]))
  acts = fx["actions"]
  names = ["agent_1", "agent_2"]
  env = Z.GridworldZooParallelEnv("island_navigation_ex_ma", level=9, max_iterations=100, seed=int(fx["seed"]))
  eng, chars = env._env.engine, list(env._env.spec.layer_chars)

  def check(t):
    assert dict(zip(chars, _lists(*(x[0] for x in eng.layer_coords())))) == coords[t], t          # order matters
    per_agent = eng.agent_layer_coords()
    for i, a in enumerate(names):
      counts, lists = per_agent[env._slots[i]]
      want = agent_coords[t][a[-1]]
      if (counts[0] < 0).any():
        assert (counts[0] == -1).all() and want == [], (t, a)
      else:
        assert dict(zip(chars, _lists(counts[0], lists[0]))) == want, (t, a)

  env.reset(); check(0)
  for t in range(acts.shape[0]):
    env.step({n: int(acts[t, i]) for i, n in enumerate(names)})
    check(t + 1)
  env.close()
