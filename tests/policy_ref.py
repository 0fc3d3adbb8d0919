"""The numpy statement of a table policy (include/sgw.h, sgw_policy): what sgw_policy_act must write, byte for byte.

Per env n and agent a: the float32 score starts at the bias (or +0.0) and takes ONE float32 addition per cell in cell order -- an
explicit loop, not np.sum (which is pairwise) --, the greedy action is the first maximum (a NaN never displaces the incumbent),
and the exploration draw is philox.py's stream with tag 2."""
import numpy as np

from ai_safety_gridworlds_amd import philox


def geometry(spec, source):
  """(cells per agent, byte offset per agent, bytes per row) of a source for this spec, as BatchedEngine.split_views cuts it."""
  A = spec.A
  if source == "board":
    hw = spec.H * spec.W
    return [hw] * A, [0] * A, hw
  c_a, off_a, off = [], [], 0
  for (h, w) in spec.view_shapes:
    c_a.append(h * w); off_a.append(off)
    off += h * w
  return c_a, off_a, off


def scores(o, code_of, w, b):
  """o uint8 [n, C_a]; w float32 [n, C, G, NA] indexable per row (the row's table); b float32 [n, NA] or None -> float32 [n, NA]."""
  n = o.shape[0]
  s = np.zeros((n, w.shape[-1]), np.float32) if b is None else np.array(b, dtype=np.float32, copy=True)
  rows = np.arange(n)
  with np.errstate(invalid="ignore", over="ignore"):
    for c in range(o.shape[1]):
      s = (s + w[rows, c, code_of[o[:, c]], :]).astype(np.float32)
  return s


def greedy(s):
  best = np.zeros(s.shape[0], np.int64)
  top = s[:, 0].copy()
  with np.errstate(invalid="ignore"):
    for j in range(1, s.shape[1]):
      m = s[:, j] > top
      best[m] = j
      top = np.where(m, s[:, j], top)
  return best


def explore(best, n_actions, explore_below, seed, env_ids, step, agent):
  env_ids = np.asarray(env_ids, dtype=np.uint64)
  x0, x1, _, _ = philox.philox4x32_10(np.uint64(step & 0xFFFFFFFF), philox.TAG_POLICY, agent, env_ids >> np.uint64(32), seed, env_ids)
  go = x0.astype(np.uint64) < np.uint64(explore_below) if explore_below < 2 ** 64 else np.ones(len(env_ids), bool)
  pick = (x1.astype(np.uint64) * np.uint64(n_actions)) >> np.uint64(32)
  return np.where(go, pick.astype(np.int64), best)


def act(obs, code_of, weights, bias, policy_of_env, c_a, off_a, n_actions, action_lo, explore_below, seed, env_ids, step):
  """obs uint8 [N, row]; weights float32 [P, A, C, G, NA]; bias [P, A, NA] or None; policy_of_env int [N] or None -> int8 [N, A]."""
  obs = np.asarray(obs)
  n, (P, A) = obs.shape[0], weights.shape[:2]
  p = np.zeros(n, np.int64) if policy_of_env is None else np.asarray(policy_of_env, dtype=np.int64)
  valid = (p >= 0) & (p < P)
  pc = np.where(valid, p, 0)
  out = np.zeros((n, A), np.int8)
  for a in range(A):
    o = obs[:, off_a[a]:off_a[a] + c_a[a]]
    s = scores(o, code_of, weights[pc, a], None if bias is None else bias[pc, a])
    idx = explore(greedy(s), n_actions, explore_below, seed, env_ids, step, a)
    out[:, a] = np.where(valid, action_lo + idx, 0).astype(np.int8)
  return out
