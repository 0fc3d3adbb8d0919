"""GPU tier of sgw_td_targets: the kernel on synthetic buffers through the C ABI (ragged env counts, every output subset, every
argument error), BatchedEngine.td_targets over real rollouts of island_navigation_ex level 9 (terminated and max-steps episode
ends, auto-reset rows, a LAST in the last row) and of island_navigation_ex_ma (agents that finish one by one), and one call
captured in a graph and replayed over refilled inputs.  Expected values always come from tests/targets_ref.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import scalarise_ref as SR
from tests import targets_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ERR_ARG = -1
IMA = next(r for r in LP.ROWS if r["id"] == "island_ex_ma")
SPECS = {"island": ("island_navigation_ex", dict(level=9)), "savanna": ("aintelope_savanna", dict(amount_agents=2)),
         "island_ma": (IMA["name"], IMA["kw"]), "firemaker": ("firemaker_ex_ma", dict(amount_agents=3))}
# (engine, C) -> the (A, C) pairs (1, 10), (2, 4), (1, 1), (3, 3); one term_reason column (R = 1) with A = 1 and A = 3, one per agent (R = A)
# in the two families whose agents finish one by one
SHAPES = [("island", 10), ("savanna", 4), ("island_ma", 4), ("island", 1), ("firemaker", 3)]
AR = {"island": (1, 1), "savanna": (2, 2), "island_ma": (2, 2), "firemaker": (3, 1)}
LAMBDAS = (0.95, 0.0, 1.0)


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def engines():
  made = {}

  def get(kind, n):
    if (kind, n) not in made:
      name, kw = SPECS[kind]
      made[(kind, n)] = BatchedEngine(make_spec(name, **kw), n, device=DEV, outputs=("step_type",))
    return made[(kind, n)]

  yield get
  for e in made.values():
    e.close()


def _td(case, d, outs, flags=0, with_value=True, **over):
  """struct sgw_td over the device tensors d of a make_case() call; outs = (ret, adv, valid) tensors or None."""
  ptr = lambda t: None if t is None else t.data_ptr()
  garr = (C.c_double * case["C"])(*case["gamma"].tolist())
  kw = dict(reward=ptr(d["reward"]), step_type=ptr(d["step_type"]), term_reason=ptr(d["term_reason"]),
            value=ptr(d["value"]) if with_value else None, value0=ptr(d["value0"]) if with_value else None,
            ret=ptr(outs[0]), adv=ptr(outs[1]), valid=ptr(outs[2]), src_rows=case["src_rows"], dst_rows=case["dst_rows"],
            T=case["T"], C=case["C"], flags=flags, reserved_=0, lambda_=case["lam"], gamma=garr)
  kw.update(over)
  td = N.Td(**kw)
  td._keep = garr
  return td


def _outs(case, asked=(True, True, True)):
  shape = (case["T"], case["dst_rows"], case["A"], case["C"])
  return [torch.full(shape, R.SENTINEL, dtype=torch.float64, device=DEV), torch.full(shape, R.SENTINEL, dtype=torch.float64, device=DEV),
          torch.full(shape[:3], R.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)], asked


def _run(e, case, d, flags, with_value, asked, what):
  outs, _ = _outs(case)
  td = _td(case, d, [o if on else None for o, on in zip(outs, asked)], flags, with_value)
  rc = e._lib.sgw_td_targets(e._h, C.byref(td), _stream())
  assert rc == 0, (what, e._lib.sgw_last_error())
  torch.cuda.synchronize()
  got = [o.cpu().numpy() for o in outs]
  want = R.expected(case, flags, with_value, want_adv=asked[1])
  R.check_outputs(case, got, want, asked, what)
  return got


# ---- 1. the kernel on synthetic buffers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind,Cn", SHAPES)
def test_kernel_on_synthetic_buffers(engines, kind, Cn, n):
  e = engines(kind, n)
  A, Rr = AR[kind]
  assert e.spec.A == A and e._lib.sgw_out_row_bytes(e._h, 5) == Rr
  rng = np.random.default_rng(1000 * n + 10 * A + Cn)
  k = 0
  for T in (1, 2, 9):
    for dst_rows in sorted({n, e.n_pad}):
      lam = LAMBDAS[k % 3]; k += 1
      case = R.make_case(rng, T, n, A, Cn, Rr, e.n_pad, dst_rows, lam)
      d = {key: _dev(case[key]) for key in ("reward", "step_type", "term_reason", "value", "value0")}
      what = "%s C=%d n=%d T=%d dst_rows=%d lambda=%g" % (kind, Cn, n, T, dst_rows, lam)
      for flags in (0, R.BOOTSTRAP_TRUNCATED):
        ret, adv, valid = _run(e, case, d, flags, True, (True, True, True), what + " flags=%d" % flags)
      _run(e, case, d, R.BOOTSTRAP_TRUNCATED, False, (True, False, True), what + " no values")
      if case["special"]:
        t, i, a = case["special"]["negzero"]
        assert (ret[t, i, a] == 0).all() and np.signbit(ret[t, i, a]).all(), "a terminated LAST returns its reward itself: -0.0 stays -0.0"
        t, i, a = case["special"]["nan"]
        assert np.isnan(ret[t, i, a, 0]) and np.isnan(adv[t, i, a, 0]) and valid[t, i, a] == 1
        t, i, a = case["special"]["inf"]
        if case["step_type"][t, i, a] == R.MID:              # (a terminated LAST does not read its own value)
          assert not np.isfinite(adv[t, i, a, -1])


@pytest.mark.parametrize("kind,Cn", SHAPES)
def test_the_inputs_tell_a_contracted_build_and_cover_every_row_kind(kind, Cn):
  """What the synthetic cases are for, checked on the host arrays of the largest one: the correctly rounded fused r + g * v
  (fractions.Fraction) differs from the two-rounding value on at least 5 % of the elements, every step-type pattern is drawn, and
  both termination reasons stand at LAST rows."""
  A, Rr = AR[kind]
  n, T = 130, 9
  case = R.make_case(np.random.default_rng(1000 * n + 10 * A + Cn), T, n, A, Cn, Rr, 192, n, 0.95)
  r, v = case["reward"][:, :n], case["value"][:, :n]
  ok = np.isfinite(r) & np.isfinite(v)
  g = np.broadcast_to(case["gamma"], r.shape)
  frac = R.fused_differs(r[ok], g[ok], v[ok])
  print("%s C=%d: fused != two roundings on %.1f %% of %d elements" % (kind, Cn, 100 * frac, int(ok.sum())))
  assert frac >= 0.05
  st = case["step_type"][:, :n]
  assert set(np.unique(case["which"])) == set(range(len(R.PATTERNS)))
  assert all((st == b).any() for b in (R.FIRST, R.MID, R.LAST, R.DEAD, 77))
  assert (st[0] == R.FIRST).any() and (st[T - 1] == R.LAST).any()
  assert ((st[:-1] == R.LAST) & (st[1:] == R.FIRST)).any() and ((st[:-1] == R.LAST) & (st[1:] == R.DEAD)).any()
  col = np.minimum(np.arange(A), Rr - 1)
  reasons = case["term_reason"][:, :n][:, :, col][st == R.LAST]
  assert set(reasons.tolist()) == {R.TERMINATED, R.MAX_STEPS}
  boot, plain = R.expected(case, R.BOOTSTRAP_TRUNCATED), R.expected(case, 0)
  assert not R.same_bits(boot[0], plain[0]) and not R.same_bits(boot[1], plain[1])


def test_every_output_subset(engines):
  e = engines("island_ma", 65)
  case = R.make_case(np.random.default_rng(5), 9, 65, 2, 4, 2, e.n_pad, 65, 0.95)
  d = {key: _dev(case[key]) for key in ("reward", "step_type", "term_reason", "value", "value0")}
  for asked in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (True, True, False)):
    _run(e, case, d, R.BOOTSTRAP_TRUNCATED, True, asked, "subset %s" % (asked,))
  _run(e, case, d, 0, False, (True, False, False), "ret alone, no values, no term_reason")


def test_bad_arguments(engines):
  e = engines("savanna", 65)
  L = e._lib
  case = R.make_case(np.random.default_rng(6), 2, 65, 2, 4, 2, e.n_pad, 65, 0.95)
  d = {key: _dev(case[key]) for key in ("reward", "step_type", "term_reason", "value", "value0")}
  outs, _ = _outs(case)
  s = _stream()
  call = lambda td: L.sgw_td_targets(e._h, None if td is None else C.byref(td), s)
  good = _td(case, d, outs, R.BOOTSTRAP_TRUNCATED)
  assert L.sgw_td_targets(None, C.byref(good), s) == ERR_ARG and b"null engine" in L.sgw_last_error()
  assert call(None) == ERR_ARG
  bad = dict(
      null_reward=dict(reward=None), null_step_type=dict(step_type=None), null_gamma=dict(gamma=None),
      no_output=dict(ret=None, adv=None, valid=None), adv_without_value=dict(value=None), adv_without_value0=dict(value0=None),
      bootstrap_without_term_reason=dict(term_reason=None), unknown_flag=dict(flags=2), unknown_flags=dict(flags=-1),
      T_zero=dict(T=0), T_negative=dict(T=-3), C_zero=dict(C=0), C_too_large=dict(C=N.MAX_K + 1),
      src_rows_short=dict(src_rows=64), dst_rows_short=dict(dst_rows=64),
      reward_misaligned=dict(reward=d["reward"].data_ptr() + 4), value_misaligned=dict(value=d["value"].data_ptr() + 4),
      value0_misaligned=dict(value0=d["value0"].data_ptr() + 2), ret_misaligned=dict(ret=outs[0].data_ptr() + 4),
      adv_misaligned=dict(adv=outs[1].data_ptr() + 1),
      ret_is_reward=dict(ret=d["reward"].data_ptr()), adv_is_value=dict(adv=d["value"].data_ptr()), ret_is_value0=dict(ret=d["value0"].data_ptr()),
      valid_is_step_type=dict(valid=d["step_type"].data_ptr()), valid_is_term_reason=dict(valid=d["term_reason"].data_ptr()))
  for name, over in bad.items():
    assert call(_td(case, d, outs, **dict(dict(flags=R.BOOTSTRAP_TRUNCATED), **over))) == ERR_ARG, name
    assert b"sgw_td_targets" in L.sgw_last_error(), name
  torch.cuda.synchronize()
  assert (outs[0] == R.SENTINEL).all() and (outs[1] == R.SENTINEL).all() and (outs[2] == R.SENTINEL_BYTE).all(), "a refused call writes nothing"
  for k in ("reward", "value"):
    assert R.same_bits(d[k].cpu().numpy(), case[k])
  assert call(good) == 0, L.sgw_last_error()                                  # and the engine still works
  assert call(_td(case, d, [outs[0], None, None], 0, False, term_reason=None)) == 0, "ret needs neither values nor term_reason"
  torch.cuda.synchronize()


# ---- 2. real rollouts through BatchedEngine.td_targets ---------------------------------------------------------------------
def _readback(e, o, T):
  n, A, K = e.n_envs, e.spec.A, e.spec.K
  reward = o["reward"].cpu().numpy().reshape(T, n, A, K)
  st = o["step_type"].cpu().numpy().reshape(T, n, A)
  tr = o["term_reason"].cpu().numpy().reshape(T, n, -1)
  return reward, st, tr


def _check_engine(e, T, reward, st, tr, gamma, lam, values, value0, bootstrap, scalar, what):
  n, A = e.n_envs, e.spec.A
  Cn = 1 if scalar else e.spec.K
  if scalar:
    reward = SR.loop_sums(reward).reshape(T, n, A, 1)
  v_np = None if values is None else values.cpu().numpy().reshape(T, n, A, Cn)
  v0_np = None if value0 is None else value0.cpu().numpy().reshape(n, A, Cn)
  res = e.td_targets(T, gamma, lam, values=values, value0=value0, bootstrap_truncated=bootstrap, scalar=scalar)
  torch.cuda.synchronize()
  g = np.full(Cn, gamma) if np.ndim(gamma) == 0 else np.asarray(gamma)
  want = R.td_targets(reward, st, tr, v_np, v0_np, g, 1.0 if lam is None else lam, R.BOOTSTRAP_TRUNCATED if bootstrap else 0)
  lead = (T, n) if A == 1 else (T, n, A)
  assert res["returns"].shape == lead + (Cn,) and res["returns"].dtype == torch.float64
  assert res["valid"].shape == lead and res["valid"].dtype == torch.bool
  assert ("advantages" in res) == (value0 is not None)
  assert R.same_bits(res["returns"].cpu().numpy().reshape(T, n, A, Cn), want[0]), what + ": returns"
  assert np.array_equal(res["valid"].cpu().numpy().reshape(T, n, A), want[2].astype(bool)), what + ": valid"
  if value0 is not None:
    assert res["advantages"].shape == lead + (Cn,)
    assert R.same_bits(res["advantages"].cpu().numpy().reshape(T, n, A, Cn), want[1]), what + ": advantages"
  return res, want


def test_engine_rollout_island_level9():
  T, n = 24, 130
  e = BatchedEngine(make_spec("island_navigation_ex", level=9, max_iterations=7), n, device=DEV, env_id_base=1000,
                    outputs=("reward", "step_type", "term_reason"))
  try:
    e.reset()
    o = e.rollout(T, 0x5AFE, write_every=True)
    reward, st, tr = _readback(e, o, T)
    K = e.spec.K
    last = st[:, :, 0] == R.LAST
    counts = (int((last & (tr[:, :, 0] == R.TERMINATED)).sum()), int((last & (tr[:, :, 0] == R.MAX_STEPS)).sum()),
              int((st == R.FIRST).sum()), int(last[T - 1].sum()))
    print("terminated LAST %d, max-steps LAST %d, FIRST %d, LAST in the last row %d" % counts)
    assert counts == (369, 156, 501, 24), "what the oracle gives for this configuration"
    rng = np.random.default_rng(3)
    values, value0 = _dev(R.numbers(rng, (T, n, K))), _dev(R.numbers(rng, (n, K)))
    gamma = [R.GAMMAS[c % 4] for c in range(K)]
    first = None
    for bootstrap in (False, True):
      res, want = _check_engine(e, T, reward, st, tr, gamma, 0.95, values, value0, bootstrap, False, "bootstrap=%r" % bootstrap)
      ptrs = {k: v.data_ptr() for k, v in res.items()}
      assert first is None or ptrs == first, "result tensors are allocated once per (T, C) and reused"
      first = ptrs
      _check_engine(e, T, reward, st, tr, 0.99, None, None, None, bootstrap, False, "returns only, bootstrap=%r" % bootstrap)
    _, boot = _check_engine(e, T, reward, st, tr, gamma, 0.95, values, value0, True, False, "again")
    _, plain = _check_engine(e, T, reward, st, tr, gamma, 0.95, values, value0, False, False, "again")
    assert not R.same_bits(boot[0], plain[0]), "the max-steps episodes bootstrap from their own row"
    sv, sv0 = _dev(R.numbers(rng, (T, n))), _dev(R.numbers(rng, (n,)))
    for bootstrap in (False, True):
      _check_engine(e, T, reward, st, tr, 0.99, 0.95, sv, sv0, bootstrap, True, "scalar, bootstrap=%r" % bootstrap)
    res = e.td_targets(T, 0.99, buffers={k: o[k] for k in ("reward", "step_type", "term_reason")}, bootstrap_truncated=True)   # the views rollout returned
    want = R.td_targets(reward, st, tr, None, None, np.full(K, 0.99), 1.0, R.BOOTSTRAP_TRUNCATED)
    assert R.same_bits(res["returns"].cpu().numpy().reshape(T, n, 1, K), want[0])
    with pytest.raises(N.SgwError, match="needs the 'reward', 'step_type'"):
      e.td_targets(T + 1, 0.99)                    # the engine holds [T, N_pad] buffers
    with pytest.raises(N.SgwError, match="no CPU path"):
      e.td_targets(T, 0.99, values=values.cpu(), value0=value0)
    with pytest.raises(N.SgwError, match="no CPU path"):
      e.td_targets(T, 0.99, buffers={"reward": o["reward"].cpu(), "step_type": o["step_type"]})
    with pytest.raises(ValueError):
      e.td_targets(T, [0.9, 0.8])
  finally:
    e.close()
  with pytest.raises(N.SgwError, match="no CPU path"):
    e.td_targets(T, 0.99)


def test_engine_rollout_per_agent_family():
  T, n = 40, 70
  e = BatchedEngine(make_spec(IMA["name"], **IMA["kw"]), n, device=DEV, outputs=("reward", "step_type", "term_reason"))
  try:
    e.seed_rng(base=11)
    e.reset()
    o = e.rollout(T, 0xD1CE, write_every=True)
    reward, st, tr = _readback(e, o, T)
    A, K = e.spec.A, e.spec.K
    assert A == 2 and tr.shape[2] == A, "one term_reason column per agent: R = A"
    assert (st == R.DEAD).any(), "an agent that finished waits as DEAD while the other plays on"
    assert ((st[:, :, 0] == R.LAST) & (st[:, :, 1] == R.MID)).any() or ((st[:, :, 1] == R.LAST) & (st[:, :, 0] == R.MID)).any(), \
        "one agent's LAST precedes the other's"
    rng = np.random.default_rng(4)
    values, value0 = _dev(R.numbers(rng, (T, n, A, K))), _dev(R.numbers(rng, (n, A, K)))
    gamma = [R.GAMMAS[c % 4] for c in range(K)]
    for bootstrap in (False, True):
      res, _ = _check_engine(e, T, reward, st, tr, gamma, 0.95, values, value0, bootstrap, False, "bootstrap=%r" % bootstrap)
      dead = torch.from_numpy(st == R.DEAD).to(DEV)
      assert not bool(res["valid"][dead].any()) and bool((res["returns"][dead] == 0).all())
  finally:
    e.close()


# ---- 3. under capture ----------------------------------------------------------------------------------------------------------
def test_td_targets_under_graph_capture():
  """A plain launch on the caller's stream: one td_targets call (without scalar=True: a single kernel) captured by
  torch.cuda.graph on a side stream after a warm-up outside the capture, replayed twice over inputs refilled in place."""
  T, n = 9, 130
  e = BatchedEngine(make_spec("island_navigation_ex", level=9), n, device=DEV, outputs=("reward", "step_type", "term_reason"))
  try:
    K, n_pad = e.spec.K, e.n_pad
    rng = np.random.default_rng(8)
    cases = [R.make_case(rng, T, n, 1, K, 1, n_pad, n, 0.95) for _ in range(3)]
    for c in cases:
      c["gamma"] = np.array([R.GAMMAS[k % 4] for k in range(K)])
    bufs = {"reward": torch.zeros((T, n_pad, K), dtype=torch.float64, device=DEV),
            "step_type": torch.zeros((T, n_pad, 1), dtype=torch.uint8, device=DEV),
            "term_reason": torch.zeros((T, n_pad), dtype=torch.uint8, device=DEV)}
    values, value0 = torch.zeros((T, n, K), dtype=torch.float64, device=DEV), torch.zeros((n, K), dtype=torch.float64, device=DEV)

    def fill(c):
      bufs["reward"].copy_(_dev(c["reward"]).reshape(T, n_pad, K))
      bufs["step_type"].copy_(_dev(c["step_type"]))
      bufs["term_reason"].copy_(_dev(c["term_reason"]).reshape(T, n_pad))
      values.copy_(_dev(c["value"]).reshape(T, n, K)); value0.copy_(_dev(c["value0"]).reshape(n, K))

    kw = dict(values=values, value0=value0, buffers=bufs, bootstrap_truncated=True)
    gamma = cases[0]["gamma"].tolist()
    fill(cases[0])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      res = e.td_targets(T, gamma, 0.95, **kw)               # warm-up outside the capture: the result tensors exist
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      res2 = e.td_targets(T, gamma, 0.95, **kw)
    assert all(res2[k].data_ptr() == res[k].data_ptr() for k in res)
    for c in cases[1:]:
      fill(c)
      for k in ("returns", "advantages"):
        res[k].fill_(R.SENTINEL)
      graph.replay()
      torch.cuda.synchronize()
      want = R.expected(c, R.BOOTSTRAP_TRUNCATED)
      assert R.same_bits(res["returns"].cpu().numpy().reshape(T, n, 1, K), want[0])
      assert R.same_bits(res["advantages"].cpu().numpy().reshape(T, n, 1, K), want[1])
      assert np.array_equal(res["valid"].cpu().numpy().reshape(T, n, 1), want[2].astype(bool))
  finally:
    e.close()
