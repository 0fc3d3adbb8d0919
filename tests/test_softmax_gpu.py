"""The softmax table policy on the device against tests/softmax_ref.py: integers equal, float bits equal, no tolerance anywhere.
act against the reference's tape; policy_step_n under sampling against a host loop of act + step on a fork over the direct, captured
and replayed paths, with a greedy call in between (no shared graph); policy_probs and the policy-gradient sums through the C ABI on
synthetic observations; the refusals; and pg_learn redone in numpy from what the device left."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine, fused_views
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import learn_ref
from tests import policy_gpu_util as U
from tests import policy_ref
from tests import scalarise_ref
from tests import softmax_ref as S
from tests import targets_ref

pytestmark = pytest.mark.gpu

BASE = (1 << 32) + 11
BETAS = (0.0, 1.4427, 64.0)
SENT32, SENT64 = np.float32(-777.25), np.float64(-777.25)
# id -> (env name, kwargs, source, the N of the closed-loop tests)
GEOS = {
    "island_l9_board": ("island_navigation_ex", dict(level=9), "board", 65),              # 6 x 8, A = 1
    "island_ma_views": ("island_navigation_ex_ma", dict(), "views", 65),                  # 5 x 5 windows from the step launch, A = 2
    "firemaker_views": ("firemaker_ex_ma", dict(amount_agents=2), "views", 17),           # windows 5 x 5, none, 33 x 33 (cut into cell ranges)
}


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(U.DEV)


def _setup(geo, n, P, seed, beta2, mixed=False, epsilon=0.0):
  name, kw, source = GEOS[geo][:3] if geo in GEOS else U.GEOMETRIES[geo]
  spec = make_spec(name, **kw)
  if source == "views":
    assert fused_views(spec), "the windows come from the step launch"
  eng = BatchedEngine(spec, n, device=U.DEV, env_id_base=BASE, outputs=U.outputs_for(spec, source))
  if name in U.GENERATOR_ENVS:
    eng.seed_rng(base=7)
  eng.reset()
  rng = np.random.default_rng(seed)
  pol = TablePolicy(eng, source=source, chars=list(spec.layer_chars) + [U.WIN], n_policies=P, seed=17, epsilon=epsilon)
  pol.beta2 = np.float32(beta2)
  w, b, idx = U.fill_policy(pol, rng, mixed, with_index=P > 1)
  return spec, eng, rng, pol, (w, b, idx)


def _ref_act(pol, obs, tables, step, beta2=None):
  w, b, idx = tables
  c_a, off_a, _ = policy_ref.geometry(pol.spec, pol.source)
  ids = BASE + np.arange(obs.shape[0])
  return S.act(obs, pol.code_of.cpu().numpy(), w, b, idx, c_a, off_a, pol.n_actions, pol.action_lo, pol.beta2 if beta2 is None else beta2,
               pol.explore_below, pol.seed, ids, step)


def _twin(eng, src):
  p = TablePolicy(eng, source=src.source, chars=src.chars, n_policies=src.n_policies, seed=src.seed)
  p.explore_below, p.beta2 = src.explore_below, src.beta2
  p.weights.copy_(src.weights); p.bias.copy_(src.bias)
  if src.policy_of_env is not None:
    p.set_policy_of_env(src.policy_of_env.clone())
  return p


def _snapshot(res):
  return {k: v.cpu().numpy().copy() for k, v in res.items()}


def _host_loop(eng, pol, T):
  outs, tape, seen = [], [], []
  for t in range(T):
    seen.append(eng._bufs[pol.source].cpu().numpy()[:eng.n_envs].copy())
    a = eng.act(pol, t=t)
    tape.append(a.cpu().numpy().copy())
    outs.append(_snapshot(eng.step_n(a.reshape((1,) + tuple(a.shape)))))
  pol.step += T
  return outs, np.stack(tape), seen


# ---- act ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta2", BETAS)
@pytest.mark.parametrize("geo", sorted(GEOS))
def test_act_equals_the_reference(geo, beta2):
  spec, eng, rng, pol, tables = _setup(geo, GEOS[geo][3], 3, 11, beta2, epsilon=0.25)
  pol.step.fill_(5)
  obs = eng._bufs[pol.source].cpu().numpy()[:eng.n_envs]
  got = eng.act(pol, t=3).cpu().numpy()
  want = _ref_act(pol, obs, tables, 8)
  assert got.shape == want.shape and (got == want).all()
  assert (got[0] == 0).all() and (got[2] == 0).all(), "a policy index out of range writes 0"
  plain = _ref_act(pol, obs, tables, 8, beta2=np.float32(1e30))             # (all but greedy)
  if beta2 != 64.0:
    assert (want != plain).any(), "the draw chooses something else than the first maximum somewhere"
  # synthetic rows over every code, the rows n >= N full of the winning byte (never read)
  row = obs.shape[1]
  alpha = np.array([ord(c) for c in spec.layer_chars] + [ord(U.WIN), 0, 200], np.uint8)
  syn = np.full((eng.n_pad, row), ord(U.WIN), np.uint8)
  syn[:eng.n_envs] = alpha[rng.integers(0, len(alpha), size=(eng.n_envs, row))]
  out = torch.full((eng.n_envs + 3, spec.A), 99, dtype=torch.int8, device=U.DEV)
  got = eng.act(pol, obs=_dev(syn), out=out[:eng.n_envs], t=0).cpu().numpy()
  assert (got == _ref_act(pol, syn[:eng.n_envs], tables, 5)).all()
  assert (out[eng.n_envs:].cpu().numpy() == 99).all(), "rows n >= N are not written"
  eng.close()


# ---- the closed loop ------------------------------------------------------------------------------------------------------------
def _closed_loop(geo, write_every, beta2, modes, record=None):
  """One call per entry of `modes` ("s": sampled, "g": greedy over the same buffers) on engine A, the same calls as a host loop of
  act + step on fork B, A's tape through step_n on fork R; the tables are rewritten in place before the fourth call.  record: a
  dict that receives every call's outputs ("A") and action tape ("tapeA") of engine A."""
  T = 8
  spec, eng, rng, polA, tables = _setup(geo, GEOS[geo][3], 3, 2 * len(modes) + int(write_every), beta2, epsilon=0.25)
  A, B, R = eng.fork(), eng.fork(), eng.fork()
  polB = _twin(B, polA)
  differ = 0
  for call, mode in enumerate(modes):
    if call == 3:
      w, b, _ = U.fill_policy(polA, rng, mixed=False, with_index=False)
      polB.weights.copy_(polA.weights); polB.bias.copy_(polA.bias)
      tables = (w, b, tables[2])
    polA.beta2 = polB.beta2 = np.float32(beta2) if mode == "s" else None
    resA = _snapshot(A.policy_step_n(polA, T, write_every=write_every))
    outsB, tapeB, seen = _host_loop(B, polB, T)
    tapeA = resA.pop("actions")
    assert (tapeA == tapeB).all(), "call %d (%s): action tapes differ" % (call, mode)
    if record is not None:
      record.setdefault("A", []).append(resA); record.setdefault("tapeA", []).append(tapeA)
    for k in resA:
      wantB = np.stack([o[k] for o in outsB]) if write_every else outsB[-1][k]
      assert LP._same(resA[k].reshape(wantB.shape), wantB), "call %d (%s): output %r differs from the host loop" % (call, mode, k)
    resR = _snapshot(R.step_n(torch.from_numpy(tapeA).to(U.DEV), write_every=True))
    for k, v in resA.items():
      want = resR[k] if write_every else resR[k][-1]
      assert LP._same(v.reshape(want.shape), want), "call %d (%s): output %r differs from step_n over the tape" % (call, mode, k)
    for t in range(T):
      if mode == "s":
        want = _ref_act(polA, seen[t], tables, call * T + t, beta2=np.float32(beta2))
      else:
        want = U.ref_actions(polA, seen[t], tables[0], tables[1], tables[2], BASE, call * T + t)
        differ += int((want != _ref_act(polA, seen[t], tables, call * T + t, beta2=np.float32(beta2))).sum())
      assert (tapeA[t] == want).all(), "call %d (%s) step %d: the tape is not the reference's" % (call, mode, t)
  assert int(polA.step.item()) == len(modes) * T == int(polB.step.item())
  assert torch.equal(A.get_state(), B.get_state()) and torch.equal(A.get_state(), R.get_state())
  for e in (eng, A, B, R):
    e.close()
  return differ


@pytest.mark.parametrize("write_every", [False, True])
@pytest.mark.parametrize("geo", sorted(GEOS))
def test_sampled_closed_loop_equals_the_host_loop(geo, write_every):
  beta2 = BETAS[(sorted(GEOS).index(geo) + int(write_every)) % 3]
  _closed_loop(geo, write_every, beta2, "ssss")                 # direct, captured, replayed, replayed over rewritten tables


def test_a_greedy_call_between_sampled_calls_has_its_own_graph():
  """Same policy struct, same buffers, T = 8: only the kind of call tells the captures apart."""
  differ = _closed_loop("island_l9_board", True, 1.4427, "ssgsgg")
  assert differ > 0, "the greedy tapes are not the sampled ones"


# ---- probs and the gradient sums through the C ABI --------------------------------------------------------------------------------
def _observations(rng, spec, S_, rows, n, row):
  obs = np.full((S_, rows, row), ord(U.WIN), np.uint8)
  alpha = np.array([ord(c) for c in spec.layer_chars] + [ord(U.WIN), 0, 7, 200, 255], np.uint8)
  obs[:, :n] = alpha[rng.integers(0, len(alpha), size=(S_, n, row))]
  return obs


def _special_tables(pol, w, b):
  """Rows of every kind of the rule, decided by the first observation byte of an agent."""
  w = w.copy()
  assert w.shape[3] > 2 and w.shape[4] > 1
  w[:, :, 0, 0, 0] = np.inf               # code 0 in cell 0: top = +inf -> degenerate
  w[:, :, 0, 1, 1] = -np.inf              # code 1 in cell 0: a -inf score, never sampled
  w[:, :, 0, 2, 0] = np.nan               # code 2 in cell 0: score[0] is NaN and is never displaced -> top NaN -> degenerate
  pol.weights.copy_(_dev(w))
  return w


CASES = [("island_l9_board", 1), ("island_l9_board", 65), ("island_l9_board", 257), ("island_ma_views", 65), ("island_ma_views", 257),
         ("firemaker_views", 17)]


@pytest.mark.parametrize("geo,n", CASES)
def test_probs_match_the_numpy_statement(geo, n):
  L = N.lib()
  T = 3
  for P, beta2 in ((1, BETAS[n % 3]), (3, BETAS[(n + 1) % 3])):
    spec, eng, rng, pol, (w, b, idx) = _setup(geo, n, P, 7 * n + P, beta2, mixed=P == 1)
    w = _special_tables(pol, w, b)
    A, NA, n_pad = spec.A, pol.n_actions, eng.n_pad
    c_a, off_a, row = policy_ref.geometry(spec, pol.source)
    O = _observations(rng, spec, T + 1, n_pad, n, row)
    actions = rng.integers(pol.action_lo - 1, pol.action_lo + NA + 1, size=(T, n, A)).astype(np.int8)
    code_of = pol.code_of.cpu().numpy()
    want_p, want_c, pi, live = S.probs(O[:, :n], code_of, w, b, idx, c_a, off_a, np.float32(beta2), actions, pol.action_lo)
    obs0, obs, acts = _dev(O[0]), _dev(O[1:]), _dev(actions)
    tail = 5
    for asked in ((True, True), (True, False), (False, True)):
      probs = torch.full(((T + 1) * n * A * NA + tail,), float(SENT32), dtype=torch.float32, device=U.DEV)
      chosen = torch.full((T * n * A + tail,), float(SENT64), dtype=torch.float64, device=U.DEV)
      rc = L.sgw_policy_probs(eng._h, C.byref(pol.native()), float(beta2), obs0.data_ptr(), obs.data_ptr(), n_pad, T, acts.data_ptr(),
                              probs.data_ptr() if asked[0] else None, chosen.data_ptr() if asked[1] else None, None)
      assert rc == 0, L.sgw_last_error()
      gp, gc = probs.cpu().numpy(), chosen.cpu().numpy()
      what = "%s n=%d P=%d beta2=%r asked=%r" % (geo, n, P, beta2, asked)
      assert (gp[-tail:] == SENT32).all() and (gc[-tail:] == SENT64).all(), what + ": written past the last row"
      if asked[0]:
        assert learn_ref.same_f32(gp[:-tail].reshape(want_p.shape), want_p), what
      else:
        assert (gp == SENT32).all(), what
      if asked[1]:
        assert learn_ref.same_f64(gc[:-tail].reshape(want_c.shape), want_c), what
      else:
        assert (gc == SENT64).all(), what
    # the engine's surface: the same numbers, persistent result tensors
    res = eng.policy_probs(pol, T, obs0, obs, acts)
    assert learn_ref.same_f32(res["probs"].cpu().numpy(), want_p) and learn_ref.same_f64(res["p_chosen"].cpu().numpy(), want_c)
    assert eng.policy_probs(pol, T, obs0, obs, acts)["probs"].data_ptr() == res["probs"].data_ptr()
    # the inputs do their work
    known = np.ones(n, bool) if idx is None else (idx >= 0) & (idx < P)
    assert (want_p[:, ~known] == 0).all() and (want_c[:, ~known] == 0).all()
    if n > 1:
      assert (~live[:, known]).any() and live.any(), "degenerate and ordinary rows both occur"
      dead = ~live & known[None, :, None]
      assert set(np.unique(want_p[dead])) == ({0.0, 1.0} if NA > 1 else {1.0}) and (want_p[dead].sum(axis=-1) == 1).all()
      assert set(np.unique(want_c[dead[:T]])) <= {0.0, 1.0}
      sums = pi[live].sum(axis=-1)
      assert np.abs(sums - 1.0).max() < 1e-12
    eng.close()


def _coefs(rng, shape):
  coef = rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)
  flat = coef.reshape(-1)
  sp = learn_ref.special_coefs(24)
  at = np.arange(0, flat.size, 7)
  flat[at] = sp[np.arange(at.size) % len(sp)]
  return coef


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("geo,n", CASES)
def test_gradient_sums_match_the_numpy_statement(geo, n, P):
  L = N.lib()
  T = 2
  beta2 = BETAS[(n + P) % 3]
  spec, eng, rng, pol, (w, b, idx) = _setup(geo, n, P, 31 * n + P, beta2, mixed=False)
  w = _special_tables(pol, w, b)
  A, NA, n_pad, lo = spec.A, pol.n_actions, eng.n_pad, pol.action_lo
  c_a, off_a, row = policy_ref.geometry(spec, pol.source)
  code_of = pol.code_of.cpu().numpy()
  inputs = []
  for k in range(2):
    O = _observations(rng, spec, T + 1, n_pad, n, row)
    actions = rng.integers(lo - 1, lo + NA + 1, size=(T, n, A)).astype(np.int8)
    inputs.append((O, actions, _coefs(rng, (T, n, A))))
  used_any = skipped_any = False
  for frac in (0, 24, 52):
    start_w = rng.integers(-2 ** 40, 2 ** 40, size=w.shape).astype(np.int64)            # the accumulators start non-zero
    start_b = rng.integers(-2 ** 40, 2 ** 40, size=b.shape).astype(np.int64)
    runs = []
    for run in range(2):
      want_w, want_b = start_w.copy(), start_b.copy()
      acc_w, acc_b = _dev(start_w), _dev(start_b)
      for k, (O, actions, coef) in enumerate(inputs):
        with_bias = k == 0
        obs0, obs, acts, cf = _dev(O[0]), _dev(O[1:]), _dev(actions), _dev(coef)
        rc = L.sgw_policy_accumulate_softmax(eng._h, C.byref(pol.native()), float(beta2), obs0.data_ptr(), obs.data_ptr(), n_pad, T,
                                             acts.data_ptr(), cf.data_ptr(), frac, acc_w.data_ptr(), acc_b.data_ptr() if with_bias else None, None)
        assert rc == 0, L.sgw_last_error()
        if run == 0:
          used = S.accumulate(want_w, want_b if with_bias else None, O[:, :n], code_of, w, b, idx, c_a, off_a, np.float32(beta2), actions, coef,
                              frac, lo)
          used_any |= bool(used.any()); skipped_any |= bool((~used).any())
          what = "%s n=%d P=%d beta2=%r frac_bits=%d call %d" % (geo, n, P, beta2, frac, k)
          assert np.array_equal(acc_w.cpu().numpy(), want_w), what
          assert np.array_equal(acc_b.cpu().numpy(), want_b), what
      runs.append((acc_w.cpu().numpy(), acc_b.cpu().numpy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "two runs give the same bits"
    if n > 1:                                    # (a single env's four transitions may all be skipped)
      assert not np.array_equal(runs[0][0], start_w) and not np.array_equal(runs[0][1], start_b)
  assert (used_any and skipped_any) or n == 1
  eng.close()


@pytest.mark.parametrize("geo,P,n,T", [("island_l9_board", 1, 650, 100), ("firemaker_views", 1, 70, 30), ("island_ma_board", 3, 650, 100)])
def test_gradient_sums_past_the_first_trip_of_the_grid(geo, P, n, T):
  """The shapes of tests/grid_caps.py at which the workgroups of a slice stride over more tiles than there are workgroups (LDS bins,
  LDS bins of a window cut into cell ranges, global atomics), with a ragged last env group."""
  from tests import grid_caps as GC
  L = N.lib()
  trips = GC.policy_accumulate(n=n, T=T, **GC.learn_geometry(geo, P))
  assert trips.extra["tiles"] > trips.extra["per_slice"] and trips.max_trips >= 2 and trips.partial
  beta2 = 1.4427
  spec, eng, rng, pol, (w, b, idx) = _setup(geo, n, P, n + T + P, beta2, mixed=False)
  w = _special_tables(pol, w, b)
  A, NA, n_pad, lo = spec.A, pol.n_actions, eng.n_pad, pol.action_lo
  c_a, off_a, row = policy_ref.geometry(spec, pol.source)
  O = _observations(rng, spec, T + 1, n_pad, n, row)
  actions = rng.integers(lo - 1, lo + NA + 1, size=(T, n, A)).astype(np.int8)
  coef = _coefs(rng, (T, n, A))
  want_w, want_b = np.zeros(w.shape, np.int64), np.zeros(b.shape, np.int64)
  acc_w, acc_b = _dev(want_w), _dev(want_b)
  obs0, obs, acts, cf = _dev(O[0]), _dev(O[1:]), _dev(actions), _dev(coef)
  rc = L.sgw_policy_accumulate_softmax(eng._h, C.byref(pol.native()), beta2, obs0.data_ptr(), obs.data_ptr(), n_pad, T, acts.data_ptr(),
                                       cf.data_ptr(), 24, acc_w.data_ptr(), acc_b.data_ptr(), None)
  assert rc == 0, L.sgw_last_error()
  used = S.accumulate(want_w, want_b, O[:, :n], pol.code_of.cpu().numpy(), w, b, idx, c_a, off_a, np.float32(beta2), actions, coef, 24, lo)
  assert used.any() and (~used).any()
  assert np.array_equal(acc_w.cpu().numpy(), want_w) and np.array_equal(acc_b.cpu().numpy(), want_b)
  eng.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments():
  L = N.lib()
  spec, eng, rng, pol, (w, b, idx) = _setup("island_l9_board", 70, 1, 2, 1.0)
  n, n_pad, A, NA, T = 70, eng.n_pad, spec.A, pol.n_actions, 8
  row = spec.H * spec.W
  O = _dev(_observations(rng, spec, T + 1, n_pad, n, row))
  obs0, obs = O[0], O[1:]
  acts = torch.zeros((T, n, A), dtype=torch.int8, device=U.DEV)
  coef = torch.zeros((T, n, A), dtype=torch.float64, device=U.DEV)
  spare = torch.zeros((T + 1) * n * A * NA + 8, dtype=torch.float64, device=U.DEV)
  aw, ab = pol.acc_weights, pol.acc_bias
  p = pol.native()

  def variant(**kw):
    q = N.Policy.from_buffer_copy(p)
    for k, v in kw.items():
      setattr(q, k, v)
    return q

  def sample(pp=None, beta2=1.0, o=obs0.data_ptr(), a=acts.data_ptr()):
    return L.sgw_policy_sample(eng._h, C.byref(pp or p), beta2, o, 0, a, None)

  def step_n(pp=None, beta2=1.0, o=obs0.data_ptr(), T_=T, out=None, a=acts.data_ptr()):
    return L.sgw_policy_sample_step_n(eng._h, C.byref(pp or p), beta2, o, T_, 0, C.byref(out or eng._out), a, 0, None)

  def probs(pp=None, beta2=1.0, o0=obs0.data_ptr(), o=obs.data_ptr(), rows=n_pad, T_=T, a=acts.data_ptr(), pr=spare.data_ptr(), c=None):
    return L.sgw_policy_probs(eng._h, C.byref(pp or p), beta2, o0, o, rows, T_, a, pr, c, None)

  def accumulate(pp=None, beta2=1.0, o0=obs0.data_ptr(), o=obs.data_ptr(), rows=n_pad, T_=T, a=acts.data_ptr(), cf=coef.data_ptr(), f=24,
                 w_=aw.data_ptr(), b_=ab.data_ptr()):
    return L.sgw_policy_accumulate_softmax(eng._h, C.byref(pp or p), beta2, o0, o, rows, T_, a, cf, f, w_, b_, None)

  assert sample() == 0 and probs() == 0 and accumulate() == 0, L.sgw_last_error()
  assert probs(T_=0, o=None, a=None) == 0, "T = 0 needs no obs"
  assert probs(pr=None, c=spare.data_ptr()) == 0 and accumulate(T_=1, o=None) == 0 and accumulate(b_=None) == 0
  ARG, UNSUPPORTED = -1, -3
  bad_beta = (-1.0, -2.0 ** -140, float("nan"), float("inf"), -float("inf"))
  for call in (sample, step_n, probs, accumulate):
    for beta2 in bad_beta:
      assert call(beta2=beta2) == ARG and b"beta2" in L.sgw_last_error(), (call.__name__, beta2)
    assert call(beta2=0.0) == 0, L.sgw_last_error()
  no_board = N.Out.from_buffer_copy(eng._out)
  no_board.board = None
  for rc in (sample(o=None), sample(a=None), sample(o=obs0.data_ptr() + 8), sample(pp=variant(n_codes=65)), sample(pp=variant(cells=47)),
             sample(pp=variant(weights=None)), sample(pp=variant(explore_below=(1 << 32) + 1)), sample(pp=variant(source=1)),
             step_n(T_=0), step_n(o=None), step_n(a=None), step_n(out=no_board), step_n(pp=variant(step_dev=None)), step_n(o=obs0.data_ptr() + 8),
             probs(T_=-1), probs(o0=None), probs(o=None), probs(pr=None), probs(rows=n - 1), probs(o0=obs0.data_ptr() + 8),
             probs(o=obs.data_ptr() + 4), probs(pr=None, c=spare.data_ptr(), a=None), probs(pr=spare.data_ptr() + 2),
             probs(c=spare.data_ptr() + 4), probs(pp=variant(n_policies=0)),
             accumulate(T_=0), accumulate(a=None), accumulate(cf=None), accumulate(w_=None), accumulate(o0=None), accumulate(o=None),
             accumulate(f=-1), accumulate(f=53), accumulate(cf=coef.data_ptr() + 4), accumulate(w_=aw.data_ptr() + 4),
             accumulate(b_=ab.data_ptr() + 4), accumulate(o0=obs0.data_ptr() + 8), accumulate(o=obs.data_ptr() + 8),
             accumulate(w_=coef.data_ptr()), accumulate(b_=coef.data_ptr()), accumulate(w_=ab.data_ptr()), accumulate(rows=n - 1),
             accumulate(w_=pol.weights.data_ptr()), accumulate(pp=variant(source=7))):
    assert rc == ARG, L.sgw_last_error()
  big = make_spec("island_navigation_ex", level=9)
  big.native.n_actions = 17
  e17 = BatchedEngine(big, 4, device=U.DEV, outputs=("board", "step_type"))
  for rc in (L.sgw_policy_sample(e17._h, C.byref(p), 1.0, obs0.data_ptr(), 0, acts.data_ptr(), None),
             L.sgw_policy_sample_step_n(e17._h, C.byref(p), 1.0, obs0.data_ptr(), T, 0, C.byref(e17._out), acts.data_ptr(), 0, None),
             L.sgw_policy_probs(e17._h, C.byref(p), 1.0, obs0.data_ptr(), None, 4, 0, None, spare.data_ptr(), None, None),
             L.sgw_policy_accumulate_softmax(e17._h, C.byref(p), 1.0, obs0.data_ptr(), None, 4, 1, acts.data_ptr(), coef.data_ptr(), 24,
                                             aw.data_ptr(), None, None)):
    assert rc == UNSUPPORTED, L.sgw_last_error()
  # a row of more than 2048 bytes (two 33 x 33 windows: 2178): acting and the probabilities stage 16 of them, the gradient sums
  # (32 KiB of rows beside their bins) refuse, the plain ones through the same plan too
  wide = make_spec("firemaker_ex_ma", amount_agents=2, agent_observation_radius=None)
  wrow = sum(h * w_ for (h, w_) in wide.view_shapes)
  assert wrow == 2178 and 16 * wrow <= 48 * 1024 and 16 * wrow > 32 * 1024
  ew = BatchedEngine(wide, 4, device=U.DEV, env_id_base=BASE, outputs=U.outputs_for(wide, "views"))
  pw = TablePolicy(ew, source="views", chars=list(wide.layer_chars) + [U.WIN], seed=17)
  wobs = _dev(_observations(rng, wide, 1, ew.n_pad, 4, wrow)[0])
  wacts = torch.zeros((1, 4, wide.A), dtype=torch.int8, device=U.DEV)
  wcoef = torch.ones((1, 4, wide.A), dtype=torch.float64, device=U.DEV)
  wprobs = torch.zeros((4, wide.A, pw.n_actions), dtype=torch.float32, device=U.DEV)
  waw, wab = pw.acc_weights, pw.acc_bias
  assert L.sgw_policy_sample(ew._h, C.byref(pw.native()), 1.0, wobs.data_ptr(), 0, wacts.data_ptr(), None) == 0, L.sgw_last_error()
  assert L.sgw_policy_probs(ew._h, C.byref(pw.native()), 1.0, wobs.data_ptr(), None, 4, 0, None, wprobs.data_ptr(), None, None) == 0
  wacts.zero_()
  rc = L.sgw_policy_accumulate_softmax(ew._h, C.byref(pw.native()), 1.0, wobs.data_ptr(), None, ew.n_pad, 1, wacts.data_ptr(), wcoef.data_ptr(), 24,
                                       waw.data_ptr(), wab.data_ptr(), None)
  assert rc == UNSUPPORTED and b"sgw_policy_accumulate_softmax" in L.sgw_last_error() and b"too long" in L.sgw_last_error()
  rc = L.sgw_policy_accumulate(ew._h, C.byref(pw.native()), wobs.data_ptr(), None, ew.n_pad, 1, wacts.data_ptr(), wcoef.data_ptr(), 24,
                               waw.data_ptr(), wab.data_ptr(), None)
  assert rc == UNSUPPORTED and b"sgw_policy_accumulate:" in L.sgw_last_error() and b"too long" in L.sgw_last_error()
  torch.cuda.synchronize()
  assert not waw.any() and not wab.any(), "a refused call leaves the accumulators alone"
  ew.close()
  assert not aw.any() and not ab.any(), "zero coefficients and refused calls leave the accumulators alone"
  # the Python surface
  greedy = TablePolicy(eng, chars=pol.chars)
  for call in (lambda: eng.policy_probs(greedy), lambda: eng.policy_accumulate_softmax(greedy, coef, T, obs0, obs, acts),
               lambda: eng.pg_learn(greedy, T, 0.9, 0.1), lambda: eng.pg_learn(pol, T, 0.9, 0.1, critic=pol)):
    with pytest.raises(N.SgwError):
      call()
  with pytest.raises(ValueError):
    eng.pg_learn(pol, T, 0.9, 0.1, critic_lr=0.1)
  assert pol.set_temperature(math.inf).beta2 == 0.0 and pol.temperature == math.inf
  assert pol.set_temperature(2.0).beta2 == np.float32(1.4426950408889634 / 2.0) and abs(pol.temperature - 2.0) < 1e-6
  assert pol.set_temperature(None).beta2 is None and pol.temperature is None
  eng.close(); e17.close()


# ---- the engine's composition -----------------------------------------------------------------------------------------------------
def _numpy_pg_learn(eng, pol, critic, traj, tabs, ctabs, T, gamma, lam, lr, critic_lr, frac):
  """One pg_learn iteration redone from what the device left: the new (policy tables, critic tables, coef, valid, step_type)."""
  spec, n, A = eng.spec, eng.n_envs, eng.spec.A
  c_a, off_a, row = policy_ref.geometry(spec, pol.source)
  obs0 = traj["obs0"].cpu().numpy()
  boards = traj[pol.source].cpu().numpy().reshape(T, n, row)
  actions = traj["actions"].cpu().numpy()
  reward = traj["reward"].cpu().numpy().reshape(T, n, A, spec.K)
  step_type = traj["step_type"].cpu().numpy().reshape(T, n, A)
  code_of = pol.code_of.cpu().numpy()
  O = learn_ref.observations(obs0, boards, n)
  ks = eng._agent_ks()
  scalar = np.stack([scalarise_ref.loop_sums(reward[:, :, a], ks[a]) for a in range(A)], axis=2)
  w, b = tabs
  if critic is not None:
    cw, cb = ctabs
    _, vmax, chosen = learn_ref.scores(O, critic.code_of.cpu().numpy(), cw, cb, None, c_a, off_a, actions, pol.action_lo)
    _, adv, valid = targets_ref.td_targets(scalar[..., None], step_type, None, vmax[1:][..., None], vmax[0][..., None], np.array([gamma]), lam)
    coef = adv[..., 0]
  else:
    ret, _, valid = targets_ref.td_targets(scalar[..., None], step_type, None, None, None, np.array([gamma]), lam)
    coef = ret[..., 0]
  valid = valid.astype(bool)
  coef = np.where(valid, coef, 0.0)
  acc_w, acc_b = np.zeros(w.shape, np.int64), np.zeros(b.shape, np.int64)
  S.accumulate(acc_w, acc_b, O, code_of, w, b, None, c_a, off_a, pol.beta2, actions, coef, frac, pol.action_lo)
  new = (learn_ref.apply(w, acc_w, lr, frac), learn_ref.apply(b, acc_b, lr, frac))
  cnew = ctabs
  if critic is not None and critic_lr is not None:
    delta = np.where(valid, (coef + vmax[:-1]) - chosen, 0.0)
    acc_w, acc_b = np.zeros(cw.shape, np.int64), np.zeros(cb.shape, np.int64)
    learn_ref.accumulate(acc_w, acc_b, O, critic.code_of.cpu().numpy(), None, c_a, off_a, actions, delta, frac, pol.action_lo)
    cnew = (learn_ref.apply(cw, acc_w, critic_lr, frac), learn_ref.apply(cb, acc_b, critic_lr, frac))
  return new, cnew, coef, valid, step_type


@pytest.mark.parametrize("with_critic", [False, True])
@pytest.mark.parametrize("name", ["island_navigation_ex", "island_navigation_ex_ma"])
def test_pg_learn_equals_the_update_redone_in_numpy(name, with_critic):
  T, n, gamma, lam, lr, critic_lr, frac = 12, 65, 0.9, 0.8, 0.05, 0.02, 24
  spec = make_spec(name, level=9, max_iterations=7) if name == "island_navigation_ex" else make_spec(name, max_iterations=7)
  outs = ("board", "reward", "cumulative", "step_type", "term_reason", "frame", "actual_action")
  eng = BatchedEngine(spec, n, device=U.DEV, env_id_base=BASE, outputs=outs)
  if name in U.GENERATOR_ENVS:
    eng.seed_rng(base=7)
  eng.reset()
  rng = np.random.default_rng(4 + int(with_critic))

  def tables(pol, scale):
    w = rng.normal(size=tuple(pol.weights.shape)).astype(np.float32) * np.float32(scale)
    b = rng.normal(size=tuple(pol.bias.shape)).astype(np.float32)
    pol.weights.copy_(_dev(w)); pol.bias.copy_(_dev(b))
    return w, b

  pol = TablePolicy(eng, seed=11, epsilon=0.1).set_temperature(0.7)
  tabs = tables(pol, 0.1)
  critic, ctabs = None, None
  if with_critic:
    critic = TablePolicy(eng, seed=12)
    ctabs = tables(critic, 0.1)
  first_board = eng._bufs["board"][:n].cpu().numpy().copy()
  kinds = set()
  for it in range(2):
    traj = eng.pg_learn(pol, T, gamma, lr, lam=lam, critic=critic, critic_lr=critic_lr if with_critic else None, frac_bits=frac)
    if it == 0:
      assert np.array_equal(traj["obs0"].cpu().numpy(), first_board), "obs0: the rows the first action was chosen on"
      assert (traj["actions"][0].cpu().numpy() == _ref_act(pol, first_board, (tabs[0], tabs[1], None), 0)).all()
    tabs, ctabs, coef, valid, step_type = _numpy_pg_learn(eng, pol, critic, traj, tabs, ctabs, T, gamma, lam, lr,
                                                          critic_lr if with_critic else None, frac)
    assert learn_ref.same_f64(traj["coef"].cpu().numpy(), coef) and np.array_equal(traj["valid"].cpu().numpy(), valid)
    assert learn_ref.same_f32(pol.weights.cpu().numpy(), tabs[0]), "weights after pg_learn call %d" % it
    assert learn_ref.same_f32(pol.bias.cpu().numpy(), tabs[1]), "bias after pg_learn call %d" % it
    if with_critic:
      assert learn_ref.same_f32(critic.weights.cpu().numpy(), ctabs[0]) and learn_ref.same_f32(critic.bias.cpu().numpy(), ctabs[1])
      assert not critic.acc_weights.any()
    assert not pol.acc_weights.any() and not pol.acc_bias.any(), "the accumulators are cleared behind the update"
    assert int(pol.step.item()) == T * (it + 1)
    kinds |= set(np.unique(step_type).tolist())
    assert valid.any() and (~valid).any() and (coef[valid] != 0).any()
  assert {N.FIRST, N.MID, N.LAST} <= kinds, "episodes end and auto-reset inside the buffer"
  assert np.isfinite(tabs[0]).all()
  eng.close()
