"""object_coordinates=True on the batched surfaces: GridworldVectorEnv(full_info=True) and GridworldZooVectorEnv carry the
reference's info_observation_coordinates / info_agent_observation_coordinates as padded device tensors.  Every step's lists are
compared with np.argwhere of the same step's layers (global) and of engine.agent_layer_views() with the facades' centre rule
(gridworld_zoo_parallel_env.py:190-196), env by env and layer by layer."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldVectorEnv
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv

pytestmark = pytest.mark.gpu


def _check_global(counts, coords, layers, what):
  """counts [N, L], coords [N, L, cap, 2] == argwhere of layers [N, L, H, W], per env and layer."""
  counts, coords, layers = counts.cpu().numpy(), coords.cpu().numpy(), layers.cpu().numpy()
  n, L = counts.shape
  assert layers.shape[:2] == (n, L) and coords.shape[:2] == (n, L)
  for i in range(n):
    for l in range(L):
      at = np.argwhere(layers[i, l])
      assert counts[i, l] == len(at), (what, i, l)
      assert np.array_equal(coords[i, l, :len(at)], at), (what, i, l)


def _check_agent(counts, coords, cube, own, what):
  """One agent: counts [N, L], coords [N, L, cap, 2] against its layer windows cube [N, L, h, w]; own = its own layer's index."""
  counts, coords, cube = counts.cpu().numpy(), coords.cpu().numpy(), cube.cpu().numpy()
  n, L = counts.shape
  for i in range(n):
    me = np.argwhere(cube[i, own]) if own >= 0 else []
    if len(me) == 0:
      assert (counts[i] == -1).all(), (what, i)
      continue
    ay, ax = me[0]
    for l in range(L):
      at = np.argwhere(cube[i, l])
      assert counts[i, l] == len(at), (what, i, l)
      assert np.array_equal(coords[i, l, :len(at)], np.stack([at[:, 1] - ax, at[:, 0] - ay], axis=1).reshape(-1, 2)), (what, i, l)


def test_vector_env_coordinates_equal_argwhere_of_the_layers():
  n = 130
  env = GridworldVectorEnv("island_navigation_ex", n, full_info=True, object_coordinates=True)
  plain = GridworldVectorEnv("island_navigation_ex", n, full_info=True)
  env.reset(); plain.reset()
  rng = np.random.default_rng(3)
  sp = env.spec_
  for t in range(20):
    acts = torch.from_numpy(rng.integers(0, 5, n).astype(np.int8)).to("cuda:0")
    info = env.step(acts)[4]
    info0 = plain.step(acts)[4]
    assert set(info) == set(info0) | {"coordinates", "coordinates_count"}, "object_coordinates=False keeps today's keys"
    assert info["coordinates"].shape == (n, len(env.layers_order), sp.H * sp.W, 2) and info["coordinates"].dtype == torch.int16
    assert info["coordinates_count"].dtype == torch.int32
    assert torch.equal(info["layers"], info0["layers"])
    _check_global(info["coordinates_count"], info["coordinates"], info["layers"], t)
  with pytest.raises(ValueError):
    GridworldVectorEnv("island_navigation_ex", 4, object_coordinates=True)
  env.close(); plain.close()


@pytest.mark.parametrize("name,kw,n", [
    ("island_navigation_ex_ma", dict(level=9), 65),
    ("firemaker_ex_ma", dict(amount_agents=3), 64),
    ("aintelope_savanna", dict(amount_agents=2, amount_predators=1, amount_water_tiles=2, observation_radius=[2, 2, 2, 2]), 65)])
def test_zoo_vector_env_coordinates(name, kw, n):
  env = GridworldZooVectorEnv(name, num_envs=n, seed=5, object_coordinates=True, **kw)
  plain = GridworldZooVectorEnv(name, num_envs=n, seed=5, **kw)
  eng = env._env.engine
  own = eng.agent_layer_index()
  rng = np.random.default_rng(9)
  sp = env.spec_
  obs, infos = env.reset()
  _, infos0 = plain.reset()
  for t in range(13):
    layers = eng.observe_layers()                                 # (aintelope_savanna: sgw_state_layers)
    cubes = eng.agent_layer_views(layers=layers)
    for i, a in enumerate(env.possible_agents):
      info = infos[a]
      assert set(info) == set(infos0[a]) | {"info_observation_coordinates", "info_observation_coordinates_count",
                                            "info_agent_observation_coordinates", "info_agent_observation_coordinates_count"}
      q = env._slots[i]
      if i == 0:
        _check_global(info["info_observation_coordinates_count"], info["info_observation_coordinates"], layers, (name, t))
      assert info["info_observation_coordinates"] is infos[env.possible_agents[0]]["info_observation_coordinates"]      # shared
      _check_agent(info["info_agent_observation_coordinates_count"], info["info_agent_observation_coordinates"], cubes[q], own[q], (name, t, a))
    if t == 12:
      break
    acts = torch.from_numpy(rng.integers(sp.action_lo, sp.action_lo + sp.n_actions, (n, sp.A)).astype(np.int8)).to("cuda:0")
    step = {a: acts[:, env._slots[i]] for i, a in enumerate(env.possible_agents)}
    obs, _, _, _, infos = env.step(step)
    infos0 = plain.step(step)[4]
  env.close(); plain.close()
