"""The numpy statement of the three learning rules of include/sgw.h (sgw_policy_scores, sgw_policy_accumulate, sgw_policy_apply):
what the device must write, bit for bit.  The scores reuse tests/policy_ref.py (one float32 addition per cell, in cell order); the
gradient sums are np.add.at on int64; the update is np.float64 arithmetic, then astype(np.float32)."""
import numpy as np

from tests import policy_ref

Q_MAX = 2 ** 31 - 1


def observations(obs0, obs, n):
  """[T + 1, n, row]: O[0] = obs0, O[s] = obs[s - 1] (rows n.. of either dropped)."""
  rows = [np.asarray(obs0)[:n]]
  if obs is not None:
    rows += [np.asarray(o)[:n] for o in obs]
  return np.stack(rows)


def scores(O, code_of, weights, bias, policy_of_env, c_a, off_a, actions=None, action_lo=0):
  """O uint8 [T+1, n, row]; weights float32 [P, A, C, G, NA]; bias [P, A, NA] or None; actions int8 [T, n, A] or None ->
  scores float32 [T+1, n, A, NA], vmax float64 [T+1, n, A], chosen float64 [T, n, A] (None without actions)."""
  S, n = O.shape[:2]
  P, A, NA = weights.shape[0], weights.shape[1], weights.shape[-1]
  p = np.zeros(n, np.int64) if policy_of_env is None else np.asarray(policy_of_env, dtype=np.int64)
  ok = (p >= 0) & (p < P)
  pc = np.where(ok, p, 0)
  sc = np.zeros((S, n, A, NA), np.float32)
  vmax = np.zeros((S, n, A), np.float64)
  chosen = None if actions is None else np.zeros((S - 1, n, A), np.float64)
  rows = np.arange(n)
  for s in range(S):
    for a in range(A):
      o = O[s][:, off_a[a]:off_a[a] + c_a[a]]
      v = policy_ref.scores(o, code_of, weights[pc, a], None if bias is None else bias[pc, a])
      v[~ok] = 0.0
      sc[s, :, a] = v
      vmax[s, :, a] = v[rows, policy_ref.greedy(v)].astype(np.float64)
      if chosen is not None and s < S - 1:
        j = actions[s, :, a].astype(np.int64) - action_lo
        inside = (j >= 0) & (j < NA) & ok
        chosen[s, :, a] = np.where(inside, v[rows, np.clip(j, 0, NA - 1)].astype(np.float64), 0.0)
  return sc, vmax, chosen


def quantise(coef, frac_bits):
  """int64 q of float64 coefficients: x = coef * 2^frac_bits; NaN -> 0; saturated at +-(2^31 - 1); else rint (ties to even)."""
  with np.errstate(all="ignore"):
    x = np.asarray(coef, np.float64) * np.float64(2.0 ** frac_bits)
    q = np.zeros(x.shape, np.int64)
    hi, lo, nan = x >= 2147483647.0, x <= -2147483647.0, np.isnan(x)
    mid = ~(hi | lo | nan)
    q[mid] = np.rint(x[mid]).astype(np.int64)
  q[hi] = Q_MAX
  q[lo] = -Q_MAX
  return q


def accumulate(acc_w, acc_b, O, code_of, policy_of_env, c_a, off_a, actions, coef, frac_bits, action_lo):
  """Adds into acc_w int64 [P, A, C, G, NA] and acc_b int64 [P, A, NA] (or None) in place; O [>= T, n, row] (O[T] is not read).
  -> the boolean [T, n, A] of the transitions that were not skipped."""
  T, n, A = actions.shape
  P, NA = acc_w.shape[0], acc_w.shape[-1]
  p = np.zeros(n, np.int64) if policy_of_env is None else np.asarray(policy_of_env, dtype=np.int64)
  q = quantise(coef, frac_bits)
  j = actions.astype(np.int64) - action_lo
  live = ((p >= 0) & (p < P))[None, :, None] & (j >= 0) & (j < NA) & (q != 0)
  for t in range(T):
    for a in range(A):
      m = live[t, :, a]
      pm, jm, qm = p[m], j[t, m, a], q[t, m, a]
      if acc_b is not None:
        np.add.at(acc_b, (pm, a, jm), qm)
      o = O[t][m][:, off_a[a]:off_a[a] + c_a[a]]
      for c in range(c_a[a]):
        np.add.at(acc_w, (pm, a, c, code_of[o[:, c]].astype(np.int64), jm), qm)
  return live


def apply(w, acc, lr, frac_bits):
  """float32 weights after the update (acc == 0: the element's bits stay)."""
  w = np.asarray(w, np.float32)
  with np.errstate(all="ignore"):
    g = acc.astype(np.float64) * np.float64(2.0 ** -frac_bits)
    new = (w.astype(np.float64) + np.float64(lr) * g).astype(np.float32)
  return np.where(acc != 0, new, w).astype(np.float32)       # np.where copies bits: a -0.0 stays -0.0


def same_f32(a, b):
  """Equal bit for bit, except that any NaN equals any NaN."""
  a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
  return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def same_f64(a, b):
  a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
  return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def special_coefs(frac_bits):
  """The coefficients the quantisation rule distinguishes: NaN, infinities, zeros, the saturation bound and beyond, exact halves of
  both parities, values that round to 0."""
  u = 2.0 ** -frac_bits
  return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, Q_MAX * u, -Q_MAX * u, (Q_MAX + 1) * u, -(Q_MAX + 1) * u, (Q_MAX - 0.5) * u,
                   -(Q_MAX - 0.5) * u, 1e300, -1e300, 0.5 * u, 1.5 * u, 2.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, 0.25 * u, -0.49 * u,
                   0.51 * u, 5e-324, 1.0, -1.0, 3.0 * u], np.float64)
