"""Shared by the table-policy GPU tests: the geometries, random tables, and the host-side mirror of a TablePolicy for
tests/policy_ref.py."""
import numpy as np

from tests import policy_ref

DEV = "cuda:0"
WIN = "Z"          # a byte no board holds; the tables make it win, and the rows n >= N of synthetic observations are full of it

# id -> (env name, kwargs, source)
GEOMETRIES = {
    "island_l9_board": ("island_navigation_ex", dict(level=9), "board"),                      # 6 x 8, A = 1
    "sokoban_board": ("side_effects_sokoban", dict(), "board"),                               # 6 x 6, actions 1..4
    "firemaker_board": ("firemaker_ex_ma", dict(amount_agents=2), "board"),                   # 17 x 17, three agent columns
    "firemaker_views": ("firemaker_ex_ma", dict(amount_agents=2), "views"),                   # windows 5 x 5, none, 33 x 33
    "island_ma_board": ("island_navigation_ex_ma", dict(), "board"),                          # 6 x 8, A = 2
}
GENERATOR_ENVS = ("firemaker_ex_ma", "island_navigation_ex_ma")


def outputs_for(spec, source):
  outs = ["board", "reward", "cumulative", "step_type", "term_reason", "frame", "actual_action"]
  if source == "views":
    outs.append("views")
  return tuple(outs)


def random_tables(rng, P, A, C, G, NA, mixed):
  """weights [P, A, C, G, NA], bias [P, A, NA]: small integers (ties, cancellations), or magnitudes 1e-3 .. 1e6 (the order of the
  additions shows); the last code (WIN's) always wins action NA - 1."""
  w = rng.integers(-3, 4, size=(P, A, C, G, NA)).astype(np.float32)
  if mixed:
    w = (np.sign(w + 0.5) * 10.0 ** rng.uniform(-3.0, 6.0, size=w.shape)).astype(np.float32)
  w[:, :, :, G - 1, :] = 0.0
  w[:, :, :, G - 1, NA - 1] = 1e9
  b = rng.integers(-2, 3, size=(P, A, NA)).astype(np.float32)
  return w, b


def fill_policy(pol, rng, mixed, with_index=True):
  """Random tables (and a random policy_of_env with entries out of range) into a TablePolicy; returns their host copies."""
  import torch
  sp = pol.spec
  w, b = random_tables(rng, pol.n_policies, sp.A, pol.cells, pol.n_codes, pol.n_actions, mixed)
  pol.weights.copy_(torch.from_numpy(w))
  pol.bias.copy_(torch.from_numpy(b))
  idx = None
  if with_index:
    idx = rng.integers(0, pol.n_policies, size=pol.n_envs).astype(np.int32)
    if pol.n_envs > 1:
      idx[0] = pol.n_policies                     # out of range: that env's actions are 0
    if pol.n_envs > 2:
      idx[2] = -1
    pol.set_policy_of_env(torch.from_numpy(idx))
  return w, b, idx


def ref_actions(pol, obs, w, b, idx, env_id_base, step):
  """policy_ref.act for a TablePolicy's configuration on host observation rows [N, row]."""
  c_a, off_a, _ = policy_ref.geometry(pol.spec, pol.source)
  ids = env_id_base + np.arange(obs.shape[0])
  return policy_ref.act(obs, pol.code_of.cpu().numpy(), w, b, idx, c_a, off_a, pol.n_actions, pol.action_lo, pol.explore_below,
                        pol.seed, ids, step)
