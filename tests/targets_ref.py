"""The contract of sgw_td_targets (include/sgw.h) as a plain numpy loop: the backward recursion over the T rows of a rollout
buffer, every element (env, agent, column) on its own, ONE IEEE double operation per line (numpy's elementwise float64 `*`, `+`,
`-` round once each; nothing here can be fused).  The tests compare the kernel and the host build of its rule with this, bit
for bit."""
import numpy as np

FIRST, MID, LAST, DEAD = 0, 1, 2, 3
TERMINATED, MAX_STEPS, TERM_NONE = 0, 1, 255
BOOTSTRAP_TRUNCATED = 1


def td_targets(reward, step_type, term_reason, value, value0, gamma, lam, flags=0, want_adv=None):
  """reward [T, N, A, C], step_type [T, N, A], term_reason [T, N, R] or None, value [T, N, A, C] or None, value0 [N, A, C] or
  None, gamma [C] -> (ret [T, N, A, C], adv [T, N, A, C] or None, valid uint8 [T, N, A])."""
  reward = np.asarray(reward, np.float64)
  T, n, A, C = reward.shape
  want_adv = (value is not None and value0 is not None) if want_adv is None else want_adv
  g = np.broadcast_to(np.asarray(gamma, np.float64).reshape(1, 1, C), (n, A, C))
  gl = g * np.float64(lam)
  ret = np.zeros((T, n, A, C))
  adv = np.zeros((T, n, A, C)) if want_adv else None
  valid = np.zeros((T, n, A), np.uint8)
  zero = np.zeros((n, A, C))
  carry_ret = value[T - 1].copy() if value is not None else zero.copy()
  carry_adv = zero.copy()
  if term_reason is not None:
    R = term_reason.shape[2]
    reason_col = np.minimum(np.arange(A), R - 1)
  with np.errstate(all="ignore"):
    for t in range(T - 1, -1, -1):
      st = step_type[t]                                            # [N, A]
      r = reward[t]
      mid = st == MID
      last = st == LAST
      truncated = np.zeros((n, A), bool)
      if flags & BOOTSTRAP_TRUNCATED:
        truncated = last & (term_reason[t][:, reason_col] == MAX_STEPS)
      terminated = last & ~truncated
      valid[t] = (mid | last).astype(np.uint8)
      v = value[t] if value is not None else zero
      gv = g * v
      boot = r + gv                                                # r + g * v
      gc = g * carry_ret
      ret_mid = r + gc                                             # r + g * carry_ret
      ret_t = np.where(mid[..., None], ret_mid, np.where(truncated[..., None], boot, np.where(terminated[..., None], r, 0.0)))
      ret[t] = ret_t
      carry_ret = ret_t
      if want_adv:
        vprev = value[t - 1] if t > 0 else value0
        delta = boot - vprev                                       # (r + g * v) - vprev
        glc = gl * carry_adv
        adv_mid = delta + glc                                      # ((r + g * v) - vprev) + gl * carry_adv
        adv_term = r - vprev
        adv_t = np.where(mid[..., None], adv_mid, np.where(truncated[..., None], delta, np.where(terminated[..., None], adv_term, 0.0)))
        adv[t] = adv_t
        carry_adv = adv_t
  return ret, adv, valid


def td_targets_scalar_loop(reward, step_type, term_reason, value, value0, gamma, lam, flags=0):
  """The same rule written element by element with Python floats (CPython's float arithmetic is the C double's): the check of
  the vectorised form above, used on small shapes only."""
  T, n, A, C = reward.shape
  want_adv = value is not None and value0 is not None
  ret = np.zeros((T, n, A, C)); adv = np.zeros((T, n, A, C)) if want_adv else None
  valid = np.zeros((T, n, A), np.uint8)
  for i in range(n):
    for a in range(A):
      for c in range(C):
        g = float(gamma[c])
        gl = g * float(lam)
        carry_ret = float(value[T - 1, i, a, c]) if value is not None else 0.0
        carry_adv = 0.0
        for t in range(T - 1, -1, -1):
          st = int(step_type[t, i, a]); r = float(reward[t, i, a, c])
          if st == MID:
            cont = 1
          elif st == LAST:
            R = term_reason.shape[2] if term_reason is not None else 1
            cont = 2 if (flags & BOOTSTRAP_TRUNCATED) and int(term_reason[t, i, min(a, R - 1)]) == MAX_STEPS else 0
          else:
            ret[t, i, a, c] = 0.0
            if want_adv:
              adv[t, i, a, c] = 0.0
            valid[t, i, a] = 0
            carry_ret = 0.0; carry_adv = 0.0
            continue
          valid[t, i, a] = 1
          v = float(value[t, i, a, c]) if value is not None else 0.0
          x = 0.0
          if want_adv:
            vprev = float(value[t - 1, i, a, c]) if t > 0 else float(value0[i, a, c])
          if cont == 1:
            gc = g * carry_ret
            y = r + gc
            if want_adv:
              gv = g * v; b = r + gv; d = b - vprev; glc = gl * carry_adv
              x = d + glc
          elif cont == 2:
            gv = g * v
            y = r + gv
            if want_adv:
              x = y - vprev
          else:
            y = r
            if want_adv:
              x = r - vprev
          ret[t, i, a, c] = y
          if want_adv:
            adv[t, i, a, c] = x
          carry_ret = y; carry_adv = x
  return ret, adv, valid


def bits(a):
  return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_bits(got, want):
  """Equal bit for bit, except that any NaN equals any NaN (the payload of a NaN an operation produces is not pinned)."""
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  if got.shape != want.shape:
    return False
  nan = np.isnan(want)
  return bool((np.isnan(got) == nan).all()) and bool((bits(np.where(nan, 0.0, got)) == bits(np.where(nan, 0.0, want))).all())


# ---- inputs that exercise the rule -------------------------------------------------------------------------------------------
PATTERNS = ("all_mid", "first_at_0", "last_at_end", "last_then_first", "last_then_dead", "byte_77", "random")


def step_types(rng, T, n, A, R):
  """step_type [T, n, A] drawn per (env, agent) from every pattern the rule distinguishes, and term_reason [T, n, R] with both
  SGW_TERMINATED and SGW_MAX_STEPS at LAST rows (TERM_NONE elsewhere).  -> step_type, term_reason, the pattern index [n, A]."""
  st = np.full((T, n, A), MID, np.uint8)
  which = rng.integers(0, len(PATTERNS), size=(n, A))
  which.reshape(-1)[:len(PATTERNS)] = np.arange(len(PATTERNS))[:which.size]           # every pattern occurs where there is room
  for i in range(n):
    for a in range(A):
      p = PATTERNS[which[i, a]]
      k = int(rng.integers(0, T))
      if p == "first_at_0":
        st[0, i, a] = FIRST
      elif p == "last_at_end":
        st[T - 1, i, a] = LAST
      elif p == "last_then_first":
        st[k, i, a] = LAST
        if k + 1 < T:
          st[k + 1, i, a] = FIRST
      elif p == "last_then_dead":
        st[k, i, a] = LAST
        st[k + 1:k + 1 + int(rng.integers(1, 4)), i, a] = DEAD
      elif p == "byte_77":
        st[k, i, a] = 77
      elif p == "random":
        st[:, i, a] = rng.choice(np.array([FIRST, MID, MID, MID, LAST, DEAD], np.uint8), size=T)
  tr = np.full((T, n, R), TERM_NONE, np.uint8)
  reason = rng.choice(np.array([TERMINATED, MAX_STEPS], np.uint8), size=(T, n, R))
  col = np.minimum(np.arange(A), R - 1)
  for a in range(A):
    at = st[:, :, a] == LAST
    tr[:, :, col[a]][at] = reason[:, :, col[a]][at]
  return st, tr, which


def scales(rng, shape):
  return rng.choice([1.0, 1.0, 1e3, 1e12], size=shape)


def numbers(rng, shape, scale=None):
  """Integers, fractions (0.1, 1/3, 1e-3) and magnitudes up to 1e12 mixed (the generator of test_scalarise_gpu._synthetic), so
  that every rounding of the rule shows in the last bits.  scale: the magnitudes, where two arrays are to share them (a value on
  the scale of its reward: the rounding of g * v then reaches the last bit of r + g * v far more often than with a reward 1e9
  times larger, where it never does)."""
  v = rng.integers(-60, 60, size=shape).astype(np.float64)
  v += rng.choice([0.0, 0.1, 1.0 / 3.0, 1e-3], size=shape)
  v *= scales(rng, shape) if scale is None else scale
  return v


GAMMAS = (0.99, 1.0, 0.0, 0.5)
SENTINEL, SENTINEL_BYTE = -777.25, 0xEE


def make_case(rng, T, n, A, C, R, src_rows, dst_rows, lam):
  """One synthetic call: padded inputs as the C ABI takes them (rows n.. of reward hold NaN, of step_type 77, of value NaN), gamma
  per column from GAMMAS, and three special elements where there is room: a terminated LAST with reward -0.0, a NaN reward, an
  infinite value."""
  st, tr, which = step_types(rng, T, n, A, R)
  reward = np.full((T, src_rows, A, C), np.nan)
  scale = scales(rng, (T, n, A, C))
  reward[:, :n] = numbers(rng, (T, n, A, C), scale)
  step_type = np.full((T, src_rows, A), 77, np.uint8)
  step_type[:, :n] = st
  term_reason = np.full((T, src_rows, R), TERM_NONE, np.uint8)
  term_reason[:, :n] = tr
  value = np.full((T, dst_rows, A, C), np.nan)
  value[:, :n] = numbers(rng, (T, n, A, C), scale)
  value0 =np.full((dst_rows, A, C), np.nan)
  value0[:n] = numbers(rng, (n, A, C))
  special = {}
  if n >= 3:
    t = T - 1
    step_type[t, 0, 0] = LAST; term_reason[t, 0, 0] = TERMINATED; reward[t, 0, 0, :] = -0.0
    special["negzero"] = (t, 0, 0)
    step_type[T // 2, 1, 0] = MID; reward[T // 2, 1, 0, 0] = np.nan
    special["nan"] = (T // 2, 1, 0)
    value[T // 2, 2, A - 1, C - 1] = np.inf
    special["inf"] = (T // 2, 2, A - 1)
  gamma = np.array([GAMMAS[c % len(GAMMAS)] for c in range(C)])
  return dict(T=T, n=n, A=A, C=C, R=R, src_rows=src_rows, dst_rows=dst_rows, lam=lam, gamma=gamma, reward=reward, step_type=step_type,
              term_reason=term_reason, value=value, value0=value0, special=special, which=which)


def expected(case, flags, with_value=True, want_adv=True):
  """(ret, adv, valid) of the rows n < N of a make_case() call."""
  n = case["n"]
  return td_targets(case["reward"][:, :n], case["step_type"][:, :n], case["term_reason"][:, :n], case["value"][:, :n] if with_value else None,
                    case["value0"][:n] if with_value else None, case["gamma"], case["lam"], flags, want_adv=want_adv and with_value)


def check_outputs(case, got, want, asked, what=""):
  """got = (ret, adv [T, dst_rows, A, C], valid [T, dst_rows, A]) as the call left them over the SENTINEL fill; asked = (ret, adv,
  valid) booleans.  Rows n >= N and outputs not asked for keep the fill; the rest equals `want` bit for bit."""
  n = case["n"]
  for name, g, w, on, fill in zip(("ret", "adv", "valid"), got, want, asked, (SENTINEL, SENTINEL, SENTINEL_BYTE)):
    g = np.asarray(g)
    if not on:
      assert (g == fill).all(), "%s %s: an output that was not asked for was written" % (what, name)
      continue
    assert (g[:, n:] == fill).all(), "%s %s: a padding row was written" % (what, name)
    if name == "valid":
      assert np.array_equal(g[:, :n], w), "%s valid differs at %s" % (what, np.argwhere(g[:, :n] != w)[:3].tolist())
    else:
      ok = same_bits(g[:, :n], w)
      if not ok:
        bad = np.argwhere(~((bits(g[:, :n]) == bits(w)) | (np.isnan(g[:, :n]) & np.isnan(w))))
        i = tuple(bad[0])
        raise AssertionError("%s %s: %d of %d values differ, first at %s want %r got %r" % (what, name, len(bad), w.size, i, w[i], g[:, :n][i]))


def fused_differs(r, g, v):
  """Fraction of elements where the correctly rounded r + g * v (what a fused multiply-add gives) differs from the two-rounding
  value, computed exactly with fractions.Fraction."""
  from fractions import Fraction
  r, v = np.asarray(r, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
  g = np.broadcast_to(np.asarray(g, np.float64), r.shape) if np.ndim(g) else np.full(r.shape, float(g))
  differ = 0
  for x, gg, y in zip(r.tolist(), g.tolist(), v.tolist()):
    exact = Fraction(x) + Fraction(gg) * Fraction(y)
    fused = exact.numerator / exact.denominator                     # int / int is correctly rounded in CPython
    differ += fused != x + gg * y
  return differ / max(1, r.size)
