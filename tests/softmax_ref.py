"""The numpy statement of the softmax table policy of include/sgw.h (sgw_policy_sample, sgw_policy_probs,
sgw_policy_accumulate_softmax): what the device must write, bit for bit.  The scores are tests/policy_ref.py's (one float32 addition
per cell, in cell order); E is float32 arithmetic with every operation rounded on its own (numpy never fuses); the sums, the
threshold and the division are float64; the quantisation and the integer sums are tests/learn_ref.py's."""
import numpy as np

from ai_safety_gridworlds_amd import philox
from tests import learn_ref
from tests import policy_ref

F = np.float32
C1, C2, C3, C4, C5, C6 = (F(float.fromhex(h)) for h in ("0x1.62e430p-1", "0x1.ebfbe0p-3", "0x1.c6b08ep-5", "0x1.3b2ab6p-7",
                                                          "0x1.5d87fep-10", "0x1.430912p-13"))
TAG_SAMPLE = 3


def exp2_rule(z):
  """E(z) for float32 z: +0.0 unless z >= -125 (NaN included); else ldexp(Horner(z - rint(z)), rint(z))."""
  z = np.asarray(z, F)
  with np.errstate(all="ignore"):
    keep = z >= F(-125.0)
    zz = np.where(keep, z, F(0.0)).astype(F)
    k = np.rint(zz).astype(F)
    g = (zz - k).astype(F)
    p = (g * C6).astype(F)
    for c in (C5, C4, C3, C2, C1):
      p = (c + p).astype(F)
      p = (g * p).astype(F)
    p = (F(1.0) + p).astype(F)
    e = np.ldexp(p, k.astype(np.int32)).astype(F)
  return np.where(keep, e, F(0.0)).astype(F)


def weights(s, beta2):
  """s float32 [n, NA] -> (best int [n], w float32 [n, NA], total float64 [n])."""
  s = np.asarray(s, F)
  best = policy_ref.greedy(s)
  top = s[np.arange(s.shape[0]), best]
  with np.errstate(all="ignore"):
    d = (s - top[:, None]).astype(F)
    z = (d * F(beta2)).astype(F)
  w = exp2_rule(z)
  total = np.zeros(s.shape[0], np.float64)
  for j in range(s.shape[1]):
    total = total + w[:, j].astype(np.float64)
  return best, w, total


def pick(w, total, x0):
  """The sampled index of rows whose total is > 0 (rows with total == 0 return NA - 1: the caller replaces them)."""
  u = (np.asarray(x0).astype(np.float64) + 0.5) * 2.0 ** -32
  thr = u * total
  n, NA = w.shape
  cum = np.zeros(n, np.float64)
  index = np.full(n, NA - 1, np.int64)
  found = np.zeros(n, bool)
  for j in range(NA):
    cum = cum + w[:, j].astype(np.float64)
    hit = ~found & (thr < cum)
    index[hit] = j
    found |= hit
  return index, found


def sample(s, beta2, explore_below, seed, env_ids, step, agent):
  """The action INDEX of every row of s [n, NA]: explore first (policy_ref.explore), then best on a degenerate row, else the draw."""
  env_ids = np.asarray(env_ids, dtype=np.uint64)
  NA = s.shape[1]
  best, w, total = weights(s, beta2)
  x0 = philox.philox4x32_10(np.uint64(step & 0xFFFFFFFF), TAG_SAMPLE, agent, env_ids >> np.uint64(32), seed, env_ids)[0]
  idx, found = pick(w, total, x0)
  live = total > 0.0
  assert found[live].all(), "the scan always finds an index on a row that is not degenerate"
  idx = np.where(live, idx, best)
  if explore_below:
    marker = np.full(len(env_ids), -1, np.int64)
    ex = policy_ref.explore(marker, NA, explore_below, seed, env_ids, step, agent)
    idx = np.where(ex >= 0, ex, idx)
  return idx


def act(obs, code_of, weights_, bias, policy_of_env, c_a, off_a, n_actions, action_lo, beta2, explore_below, seed, env_ids, step):
  """policy_ref.act under the softmax rule -> int8 [N, A]."""
  obs = np.asarray(obs)
  n, (P, A) = obs.shape[0], weights_.shape[:2]
  p = np.zeros(n, np.int64) if policy_of_env is None else np.asarray(policy_of_env, dtype=np.int64)
  valid = (p >= 0) & (p < P)
  pc = np.where(valid, p, 0)
  out = np.zeros((n, A), np.int8)
  for a in range(A):
    o = obs[:, off_a[a]:off_a[a] + c_a[a]]
    s = policy_ref.scores(o, code_of, weights_[pc, a], None if bias is None else bias[pc, a])
    idx = sample(s, beta2, explore_below, seed, env_ids, step, a)
    out[:, a] = np.where(valid, action_lo + idx, 0).astype(np.int8)
  return out


def pi_of(s, beta2):
  """pi float64 [n, NA] and the boolean of rows that are not degenerate (those are 1.0 at best, +0.0 elsewhere)."""
  best, w, total = weights(s, beta2)
  live = total > 0.0
  with np.errstate(all="ignore"):
    pi = w.astype(np.float64) / np.where(live, total, 1.0)[:, None]
  onehot = (np.arange(s.shape[1])[None, :] == best[:, None]).astype(np.float64)
  return np.where(live[:, None], pi, onehot), live


def probs(O, code_of, weights_, bias, policy_of_env, c_a, off_a, beta2, actions=None, action_lo=0):
  """O uint8 [T+1, n, row] -> probs float32 [T+1, n, A, NA], p_chosen float64 [T, n, A] (None without actions), pi float64
  [T+1, n, A, NA], live bool [T+1, n, A] (known table and not degenerate)."""
  S, n = O.shape[:2]
  P, A, NA = weights_.shape[0], weights_.shape[1], weights_.shape[-1]
  p = np.zeros(n, np.int64) if policy_of_env is None else np.asarray(policy_of_env, dtype=np.int64)
  ok = (p >= 0) & (p < P)
  pc = np.where(ok, p, 0)
  pi = np.zeros((S, n, A, NA), np.float64)
  live = np.zeros((S, n, A), bool)
  chosen = None if actions is None else np.zeros((S - 1, n, A), np.float64)
  rows = np.arange(n)
  for s in range(S):
    for a in range(A):
      o = O[s][:, off_a[a]:off_a[a] + c_a[a]]
      v = policy_ref.scores(o, code_of, weights_[pc, a], None if bias is None else bias[pc, a])
      q, lv = pi_of(v, beta2)
      q[~ok] = 0.0
      pi[s, :, a], live[s, :, a] = q, lv & ok
      if chosen is not None and s < S - 1:
        j = actions[s, :, a].astype(np.int64) - action_lo
        inside = (j >= 0) & (j < NA)
        chosen[s, :, a] = np.where(inside, q[rows, np.clip(j, 0, NA - 1)], 0.0)
  return pi.astype(F), chosen, pi, live


def grad_terms(pi, j, coef, frac_bits):
  """q int64 [..., NA] of transitions with probabilities pi [..., NA], action index j [...] (inside 0 .. NA-1) and coef [...]."""
  NA = pi.shape[-1]
  with np.errstate(all="ignore"):
    d = (np.arange(NA) == np.asarray(j)[..., None]).astype(np.float64) - pi
    x = np.asarray(coef, np.float64)[..., None] * d
  return learn_ref.quantise(x, frac_bits)


def accumulate(acc_w, acc_b, O, code_of, weights_, bias, policy_of_env, c_a, off_a, beta2, actions, coef, frac_bits, action_lo):
  """Adds the score-function sums into acc_w int64 [P, A, C, G, NA] and acc_b int64 [P, A, NA] (or None) in place; O [>= T, n, row].
  -> the boolean [T, n, A] of the transitions that were not skipped (known table, action in range, not degenerate)."""
  T, n, A = actions.shape
  P, NA = acc_w.shape[0], acc_w.shape[-1]
  p = np.zeros(n, np.int64) if policy_of_env is None else np.asarray(policy_of_env, dtype=np.int64)
  _, _, pi, live = probs(O[:T], code_of, weights_, bias, policy_of_env, c_a, off_a, beta2)
  j = actions.astype(np.int64) - action_lo
  used = live & (j >= 0) & (j < NA)
  q = grad_terms(pi, np.clip(j, 0, NA - 1), coef, frac_bits)
  ks = np.arange(NA)
  for t in range(T):
    for a in range(A):
      m = used[t, :, a]
      pm, qm = p[m], q[t, m, a]                                         # [k], [k, NA]
      if acc_b is not None:
        np.add.at(acc_b, (pm[:, None], a, ks[None, :]), qm)
      o = O[t][m][:, off_a[a]:off_a[a] + c_a[a]]
      for c in range(c_a[a]):
        np.add.at(acc_w, (pm[:, None], a, c, code_of[o[:, c]].astype(np.int64)[:, None], ks[None, :]), qm)
  return used
