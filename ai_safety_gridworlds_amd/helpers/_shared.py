"""What GridworldGymEnv and GridworldZooParallelEnv both compute for one logical env: the env-generator seeding and the
layer-derived info entries of the reference wrappers (gridworld_gym_env.py:397-450, gridworld_zoo_parallel_env.py:286-359)."""
import numpy as np


def seed_env(engine, spec, seed):
  """environment_data[NP_RANDOM] = seeding.np_random(seed)[0]: the PCG64 state words of the seed become env 0's generator."""
  if spec.needs_rng:
    st = np.random.PCG64(np.random.SeedSequence(seed)).state["state"]
    m = (1 << 64) - 1
    engine.set_rng_state(np.array([[st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m]], dtype=np.uint64))


def layers_dict(spec, cube):
  """{layer character: bool [h, w]} of env 0 of a device layer cube [N, L, h, w] (the board's, or one agent's window)."""
  planes = cube[0].cpu().numpy().astype(bool)
  return {c: planes[i] for i, c in enumerate(spec.layer_chars)}


def coordinates(layers):
  """calculate_observation_coordinates (safety_game_mo.py:422-457, safety_game_moma.py:583-603): (row, col) per layer."""
  return {c: [tuple(x) for x in np.argwhere(layers[c]).tolist()] for c in layers}


def relative_coordinates(layers, ch):
  """calculate_agents_observation_coordinates (safety_game_moma.py:528-580): (x, y) relative to agent `ch`; [] without it."""
  me = np.argwhere(layers[ch]) if ch in layers else []
  if len(me) == 0:
    return []
  ay, ax = int(me[0][0]), int(me[0][1])
  return {c: [(int(x) - ax, int(y) - ay) for y, x in np.argwhere(layers[c]).tolist()] for c in layers}


def ordered_cube(layers, order):
  """get_layers_order / calculate_observation_layers_cube (safety_game_mo.py:460-520, safety_game_moma.py:621-672).  An empty
  order: every layer, sorted; absent layers read as zeros (cross-environment cubes)."""
  order = list(order) or sorted(layers.keys())
  zero = np.zeros_like(next(iter(layers.values())))
  return order, np.stack([layers.get(c, zero) for c in order], axis=0)
