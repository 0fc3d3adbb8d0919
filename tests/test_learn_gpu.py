"""sgw_policy_scores / sgw_policy_accumulate / sgw_policy_apply on the device against tests/learn_ref.py: integers equal, float bits
equal, no tolerance anywhere.  Synthetic observations through the C ABI (both row layouts, every output subset, several tables with
indices out of range, actions and coefficients at every edge of the rules), then the engine's composition (policy_rollout,
policy_scores, td_targets, policy_accumulate, policy_apply = q_learn) redone in numpy from what the device left, and the chain
under graph capture."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec
from tests import learn_ref as R
from tests import policy_gpu_util as U
from tests import policy_ref
from tests import scalarise_ref
from tests import targets_ref

pytestmark = pytest.mark.gpu

FRAC = 24
SENT32, SENT64 = np.float32(-777.25), np.float64(-777.25)


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(U.DEV)


def _setup(geo, n, P, seed, mixed=True):
  name, kw, source = U.GEOMETRIES[geo]
  spec = make_spec(name, **kw)
  eng = BatchedEngine(spec, n, device=U.DEV, outputs=U.outputs_for(spec, source))
  rng = np.random.default_rng(seed)
  pol = TablePolicy(eng, source=source, chars=list(spec.layer_chars) + [U.WIN], n_policies=P, seed=5)
  w, b, idx = U.fill_policy(pol, rng, mixed, with_index=P > 1)
  c_a, off_a, row = policy_ref.geometry(spec, source)
  return spec, eng, rng, pol, w, b, idx, c_a, off_a, row


def _alphabet(spec):
  """Every code of the test policies: the spec's characters, the winning byte, and bytes outside them (code 0)."""
  return np.array([ord(c) for c in spec.layer_chars] + [ord(U.WIN), 0, 7, 200, 255], np.uint8)


def _observations(rng, spec, S, rows, n, row):
  """uint8 [S, rows, row]: rows n < N random over every code, rows n >= N full of the winning byte (never read)."""
  obs = np.full((S, rows, row), ord(U.WIN), np.uint8)
  alpha = _alphabet(spec)
  obs[:, :n] = alpha[rng.integers(0, len(alpha), size=(S, n, row))]
  return obs


# ---- scores ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [0, 3])
@pytest.mark.parametrize("n", [1, 70])
@pytest.mark.parametrize("geo", ["island_l9_board", "firemaker_views"])
def test_scores_match_the_numpy_statement(geo, n, T):
  L = N.lib()
  for P in (1, 3):
    spec, eng, rng, pol, w, b, idx, c_a, off_a, row = _setup(geo, n, P, 100 * n + T + P)
    A, NA, n_pad = spec.A, pol.n_actions, eng.n_pad
    assert n_pad == (128 if n == 70 else 64)
    O = _observations(rng, spec, T + 1, n_pad, n, row)
    obs0, obs = _dev(O[0]), (_dev(O[1:]) if T else None)
    actions = rng.integers(pol.action_lo - 1, pol.action_lo + NA + 1, size=(T, n, A)).astype(np.int8)    # one below and one above the range too
    if T:
      actions.reshape(-1)[0] = -1
    acts = _dev(actions) if T else None
    code_of = pol.code_of.cpu().numpy()
    want = R.scores(O[:, :n], code_of, w, b, idx, c_a, off_a, actions if T else None, pol.action_lo)
    shapes = ((T + 1, n, A, NA), (T + 1, n, A), (max(T, 1), n, A))
    for asked in itertools.product((False, True), repeat=3):
      if not any(asked):
        continue
      bufs = [torch.full(shapes[0], float(SENT32), dtype=torch.float32, device=U.DEV),
              torch.full(shapes[1], float(SENT64), dtype=torch.float64, device=U.DEV),
              torch.full(shapes[2], float(SENT64), dtype=torch.float64, device=U.DEV)]
      ptrs = [t.data_ptr() if on else None for t, on in zip(bufs, asked)]
      rc = L.sgw_policy_scores(eng._h, C.byref(pol.native()), obs0.data_ptr(), obs.data_ptr() if T else None, n_pad, T,
                               acts.data_ptr() if T else None, ptrs[0], ptrs[1], ptrs[2], None)
      assert rc == 0, L.sgw_last_error()
      got = [t.cpu().numpy() for t in bufs]
      what = "%s n=%d T=%d P=%d asked=%r" % (geo, n, T, P, asked)
      for k, same in ((0, R.same_f32), (1, R.same_f64), (2, R.same_f64)):
        if not asked[k]:
          assert (got[k] == (SENT32 if k == 0 else SENT64)).all(), what + ": an output that was not asked for was written"
        elif k == 2 and T == 0:
          assert (got[k] == SENT64).all(), what + ": there is no chosen without a step"
        else:
          assert same(got[k], want[k]), what + ": output %d" % k
    # epsilon = 0: the first maximum of scores[s] is the action sgw_policy_act takes on O[s]
    sc = want[0]
    for s in range(T + 1):
      out = torch.zeros((n, A), dtype=torch.int8, device=U.DEV)
      rows = obs0 if s == 0 else obs[s - 1]
      assert L.sgw_policy_act(eng._h, C.byref(pol.native()), rows.data_ptr(), 0, out.data_ptr(), None) == 0, L.sgw_last_error()
      best = np.stack([policy_ref.greedy(sc[s, :, a]) for a in range(A)], axis=1) + pol.action_lo
      if idx is not None:
        best[(idx < 0) | (idx >= P)] = 0
      assert (out.cpu().numpy() == best).all()
    # the inputs do their work: out-of-range tables give +0.0, an agent without a window gets its bias, an outside action +0.0
    if idx is not None and n > 1:
      assert (sc[:, 0] == 0).all() and not np.signbit(sc[:, 0]).any() and (want[1][:, 0] == 0).all()
    for a in range(A):
      if c_a[a] == 0 and P == 1:
        assert R.same_f32(sc[:, :, a], np.broadcast_to(b[0, a], sc[:, :, a].shape))
    if T:
      j = actions.astype(np.int64) - pol.action_lo
      assert ((j < 0) | (j >= NA)).any() and (want[2][(j < 0) | (j >= NA)] == 0).all()
    eng.close()


# ---- accumulate -----------------------------------------------------------------------------------------------------------------
def _transition_inputs(rng, start, T, n, A, NA, action_lo):
  """actions int8 [T, n, A] cycling through every index, -1 and action_lo + n_actions; coef float64 [T, n, A]: three in four random,
  one in four from the special values of the quantisation rule.  `start`: transitions drawn so far (the cycles go on across calls)."""
  i = start + np.arange(T * n * A)
  cycle = np.array(list(range(action_lo, action_lo + NA)) + [-1, action_lo + NA], np.int64)
  actions = cycle[i % len(cycle)].astype(np.int8).reshape(T, n, A)
  special = R.special_coefs(FRAC)
  coef = rng.normal(size=i.size) * 10.0 ** rng.uniform(-3, 3, size=i.size)
  sp = (i % 4) == 3
  coef[sp] = special[(i[sp] // 4) % len(special)]
  return actions, coef.reshape(T, n, A)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("n", [1, 64, 70])
@pytest.mark.parametrize("geo", ["island_l9_board", "island_ma_board", "firemaker_views"])
def test_accumulate_matches_the_numpy_statement(geo, n, T, P):
  L = N.lib()
  spec, eng, rng, pol, w, b, idx, c_a, off_a, row = _setup(geo, n, P, 1000 * n + 10 * T + P, mixed=False)
  A, NA, n_pad, lo = spec.A, pol.n_actions, eng.n_pad, pol.action_lo
  code_of = pol.code_of.cpu().numpy()
  want_w = rng.integers(-2 ** 40, 2 ** 40, size=w.shape).astype(np.int64)            # the accumulators start non-zero
  want_b = rng.integers(-2 ** 40, 2 ** 40, size=b.shape).astype(np.int64)
  acc_w, acc_b = _dev(want_w), _dev(want_b)
  calls = max(3, -(-4 * (NA + 3) // (T * n * A)))
  drawn, layouts, live_all, q_all, act_all, seen = 0, set(), [], [], [], np.zeros((max(c_a), 256), bool)
  for k in range(calls):
    plain = k % 2 == 1
    rows = n if plain else n_pad
    O = _observations(rng, spec, T + 1, rows, n, row)
    actions, coef = _transition_inputs(rng, drawn, T, n, A, NA, lo)
    drawn += actions.size
    with_bias = k != 2
    obs0, obs, acts, cf = _dev(O[0]), _dev(O[1:]), _dev(actions), _dev(coef)
    rc = L.sgw_policy_accumulate(eng._h, C.byref(pol.native()), obs0.data_ptr(), obs.data_ptr(), rows, T, acts.data_ptr(), cf.data_ptr(), FRAC,
                                 acc_w.data_ptr(), acc_b.data_ptr() if with_bias else None, None)
    if plain and T > 2 and (rows * row) % 16:
      assert rc == -1 and b"16-byte" in L.sgw_last_error(), "row blocks that are not 16-byte aligned are refused"
      continue
    assert rc == 0, L.sgw_last_error()
    layouts.add(plain)
    live = R.accumulate(want_w, want_b if with_bias else None, O[:, :n], code_of, idx, c_a, off_a, actions, coef, FRAC, lo)
    live_all.append(live.reshape(-1)); q_all.append(R.quantise(coef, FRAC).reshape(-1)); act_all.append(actions.reshape(-1))
    for a in range(A):
      for t in range(T):
        seen[np.arange(c_a[a])[None, :], O[t, :n, off_a[a]:off_a[a] + c_a[a]]] = True
    what = "%s n=%d T=%d P=%d call %d (%s rows)" % (geo, n, T, P, k, "plain" if plain else "padded")
    assert np.array_equal(acc_w.cpu().numpy(), want_w), what
    assert np.array_equal(acc_b.cpu().numpy(), want_b), what
  # the inputs do their job, checked on the reference side
  q, acts, live = np.concatenate(q_all), np.concatenate(act_all), np.concatenate(live_all)
  assert (q != 0).mean() >= 0.5
  assert set(range(lo, lo + NA)) <= set(acts.tolist()) and -1 in acts and lo + NA in acts
  assert live.any() and (~live & (q != 0)).any(), "transitions are skipped for their action or table alone, too"
  assert (q == R.Q_MAX).any() and (q == -R.Q_MAX).any(), "both saturations occur"
  codes_seen = np.array([len(set(code_of[np.flatnonzero(seen[c])])) for c in range(max(c_a))])
  assert (codes_seen >= 2).mean() > 0.5
  assert layouts == {False, True} or (n * row) % 16
  eng.close()


# ---- apply ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo,P", [("island_l9_board", 1), ("island_ma_board", 3)])
def test_apply_matches_the_numpy_statement(geo, P):
  L = N.lib()
  spec, eng, rng, pol, w, b, idx, c_a, off_a, row = _setup(geo, 70, P, 31 + P)
  w = w.copy(); b = b.copy()
  w.reshape(-1)[:4] = [-0.0, 0.0, np.inf, 1.0]
  b.reshape(-1)[:2] = [-0.0, 1.0]
  for clear, with_bias, lr in ((False, True, 0.1), (True, True, -0.37), (True, False, 1e-3), (False, False, 0.0)):
    acc_w = rng.integers(-2 ** 36, 2 ** 36, size=w.shape).astype(np.int64)
    acc_w[rng.random(w.shape) < 0.4] = 0
    acc_b = rng.integers(-2 ** 36, 2 ** 36, size=b.shape).astype(np.int64)
    acc_b[rng.random(b.shape) < 0.4] = 0
    acc_w.reshape(-1)[:4] = [0, 0, 7, 2 ** 53 + 1]
    acc_b.reshape(-1)[:2] = [0, -(2 ** 62)]
    pol.weights.copy_(_dev(w)); pol.bias.copy_(_dev(b))
    aw, ab = _dev(acc_w), _dev(acc_b)
    rc = L.sgw_policy_apply(eng._h, C.byref(pol.native()), lr, FRAC, aw.data_ptr(), ab.data_ptr() if with_bias else None,
                            N.APPLY_CLEAR if clear else 0, None)
    assert rc == 0, L.sgw_last_error()
    got_w, got_b = pol.weights.cpu().numpy(), pol.bias.cpu().numpy()
    what = "%s clear=%r bias=%r lr=%r" % (geo, clear, with_bias, lr)
    assert R.same_f32(got_w, R.apply(w, acc_w, lr, FRAC)), what
    assert R.same_f32(got_b, R.apply(b, acc_b, lr, FRAC) if with_bias else b), what
    still = acc_w == 0
    assert np.array_equal(got_w.view(np.uint32)[still], w.view(np.uint32)[still]), "untouched elements keep their bytes"
    assert got_w.view(np.uint32).reshape(-1)[0] == 0x80000000
    assert np.array_equal(aw.cpu().numpy(), np.zeros_like(acc_w) if clear else acc_w), what
    assert np.array_equal(ab.cpu().numpy(), np.zeros_like(acc_b) if clear and with_bias else acc_b), what
  eng.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments():
  L = N.lib()
  spec, eng, rng, pol, w, b, idx, c_a, off_a, row = _setup("island_l9_board", 70, 1, 2)
  n, n_pad, A, NA, T = 70, eng.n_pad, spec.A, pol.n_actions, 3
  O = _dev(_observations(rng, spec, T + 1, n_pad, n, row))
  obs0, obs = O[0], O[1:]
  acts = torch.zeros((T, n, A), dtype=torch.int8, device=U.DEV)
  coef = torch.zeros((T, n, A), dtype=torch.float64, device=U.DEV)
  spare = torch.zeros(T * n * A * NA + 8, dtype=torch.float64, device=U.DEV)
  aw, ab = pol.acc_weights, pol.acc_bias
  p = pol.native()

  def variant(**kw):
    q = N.Policy.from_buffer_copy(p)
    for k, v in kw.items():
      setattr(q, k, v)
    return q

  def scores(pp=None, o0=obs0.data_ptr(), o=obs.data_ptr(), rows=n_pad, T_=T, a=acts.data_ptr(), s=spare.data_ptr(), v=None, c=None):
    return L.sgw_policy_scores(eng._h, C.byref(pp or p), o0, o, rows, T_, a, s, v, c, None)

  def accumulate(pp=None, o0=obs0.data_ptr(), o=obs.data_ptr(), rows=n_pad, T_=T, a=acts.data_ptr(), cf=coef.data_ptr(), f=FRAC,
                 w_=aw.data_ptr(), b_=ab.data_ptr()):
    return L.sgw_policy_accumulate(eng._h, C.byref(pp or p), o0, o, rows, T_, a, cf, f, w_, b_, None)

  def apply(pp=None, f=FRAC, w_=aw.data_ptr(), b_=ab.data_ptr(), flags=0):
    return L.sgw_policy_apply(eng._h, C.byref(pp or p), 0.0, f, w_, b_, flags, None)

  assert scores() == 0 and accumulate() == 0 and apply() == 0, L.sgw_last_error()
  assert scores(T_=0, o=None, a=None) == 0, "T = 0 needs no obs"
  ARG, UNSUPPORTED = -1, -3
  for rc in (scores(T_=-1), scores(o0=None), scores(o=None), scores(s=None), scores(rows=n - 1), scores(o0=obs0.data_ptr() + 8),
             scores(o=obs.data_ptr() + 4), scores(s=None, c=spare.data_ptr(), a=None), scores(s=spare.data_ptr() + 2),
             scores(v=spare.data_ptr() + 4), scores(pp=variant(n_codes=65)), scores(pp=variant(cells=47)), scores(pp=variant(weights=None)),
             accumulate(T_=0), accumulate(a=None), accumulate(cf=None), accumulate(w_=None), accumulate(o0=None), accumulate(o=None),
             accumulate(f=-1), accumulate(f=53), accumulate(cf=coef.data_ptr() + 4), accumulate(w_=aw.data_ptr() + 4),
             accumulate(b_=ab.data_ptr() + 4), accumulate(o0=obs0.data_ptr() + 8), accumulate(o=obs.data_ptr() + 8),
             accumulate(w_=coef.data_ptr()), accumulate(b_=coef.data_ptr()), accumulate(w_=ab.data_ptr()), accumulate(rows=n - 1),
             accumulate(pp=variant(n_policies=0)), accumulate(pp=variant(source=7)),
             apply(w_=None), apply(f=-1), apply(f=53), apply(flags=2), apply(flags=-1), apply(w_=aw.data_ptr() + 4),
             apply(w_=pol.weights.data_ptr()), apply(pp=variant(code_of=None))):
    assert rc == ARG, L.sgw_last_error()
  assert accumulate(T_=1, o=None) == 0, "with T = 1 only O[0] is read"
  assert scores(rows=n, T_=1) == 0 and scores(rows=n + 1, T_=1) == 0, "one row block has no second block to align"
  big = make_spec("island_navigation_ex", level=9)
  big.native.n_actions = 17
  e17 = BatchedEngine(big, 4, device=U.DEV, outputs=("board", "step_type"))
  for rc in (L.sgw_policy_scores(e17._h, C.byref(p), obs0.data_ptr(), None, 4, 0, None, spare.data_ptr(), None, None, None),
             L.sgw_policy_accumulate(e17._h, C.byref(p), obs0.data_ptr(), None, 4, 1, acts.data_ptr(), coef.data_ptr(), FRAC, aw.data_ptr(), None, None),
             L.sgw_policy_apply(e17._h, C.byref(p), 0.0, FRAC, aw.data_ptr(), None, 0, None)):
    assert rc == UNSUPPORTED, L.sgw_last_error()
  torch.cuda.synchronize()
  assert not aw.any() and not ab.any(), "zero coefficients and refused calls leave the accumulators alone"
  # the Python surface raises in the style of td_targets
  with pytest.raises(N.SgwError, match="coef"):
    eng.policy_accumulate(pol, coef.float(), T, obs0, obs, acts)
  with pytest.raises(N.SgwError, match="obs0"):
    eng.policy_scores(pol, T)
  with pytest.raises(ValueError):
    eng.policy_accumulate(pol, coef, 0, obs0)
  eng.close(); e17.close()


# ---- the engine's composition -----------------------------------------------------------------------------------------------------
def _numpy_q_learn(eng, pol, traj, w, b, T, gamma, lr):
  """One q_learn iteration redone from what the device left: (weights, bias, delta, valid) as numpy has them."""
  spec, n, A = eng.spec, eng.n_envs, eng.spec.A
  c_a, off_a, row = policy_ref.geometry(spec, pol.source)
  obs0 = traj["obs0"].cpu().numpy()
  boards = traj["board"].cpu().numpy().reshape(T, n, row)
  actions = traj["actions"].cpu().numpy()
  reward = traj["reward"].cpu().numpy().reshape(T, n, A, spec.K)
  step_type = traj["step_type"].cpu().numpy().reshape(T, n, A)
  code_of = pol.code_of.cpu().numpy()
  O = R.observations(obs0, boards, n)
  _, vmax, chosen = R.scores(O, code_of, w, b, None, c_a, off_a, actions, pol.action_lo)
  ks = eng._agent_ks()
  scalar = np.stack([scalarise_ref.loop_sums(reward[:, :, a], ks[a]) for a in range(A)], axis=2)
  _, adv, valid = targets_ref.td_targets(scalar[..., None], step_type, None, vmax[1:][..., None], vmax[0][..., None], np.array([gamma]), 0.0)
  delta = (adv[..., 0] + vmax[:-1]) - chosen
  delta = np.where(valid.astype(bool), delta, 0.0)
  acc_w, acc_b = np.zeros(w.shape, np.int64), np.zeros(b.shape, np.int64)
  R.accumulate(acc_w, acc_b, O, code_of, None, c_a, off_a, actions, delta, FRAC, pol.action_lo)
  return R.apply(w, acc_w, lr, FRAC), R.apply(b, acc_b, lr, FRAC), delta, valid.astype(bool), step_type


@pytest.mark.parametrize("name", ["island_navigation_ex", "island_navigation_ex_ma"])
def test_q_learn_equals_the_update_redone_in_numpy(name):
  T, n, gamma, lr = 12, 70, 0.9, 0.05
  spec = make_spec(name, level=9, max_iterations=7) if name == "island_navigation_ex" else make_spec(name, max_iterations=7)
  outs = ("board", "reward", "cumulative", "step_type", "term_reason", "frame", "actual_action")
  eng = BatchedEngine(spec, n, device=U.DEV, outputs=outs)
  if name in U.GENERATOR_ENVS:
    eng.seed_rng(base=7)
  eng.reset()
  pol = TablePolicy(eng, seed=11, epsilon=0.5)
  rng = np.random.default_rng(4)
  w = rng.normal(size=tuple(pol.weights.shape)).astype(np.float32) * np.float32(0.1)
  b = rng.normal(size=tuple(pol.bias.shape)).astype(np.float32)
  pol.weights.copy_(_dev(w)); pol.bias.copy_(_dev(b))
  first_board = eng._bufs["board"][:n].cpu().numpy().copy()
  kinds = set()
  for it in range(2):
    traj = eng.q_learn(pol, T, gamma, lr)
    if it == 0:
      assert np.array_equal(traj["obs0"].cpu().numpy(), first_board), "obs0: the rows the first action was chosen on"
      want_first = U.ref_actions(pol, first_board, w, b, None, 0, 0)
      assert (traj["actions"][0].cpu().numpy() == want_first).all()
    w, b, delta, valid, step_type = _numpy_q_learn(eng, pol, traj, w, b, T, gamma, lr)
    assert R.same_f64(traj["delta"].cpu().numpy(), delta) and np.array_equal(traj["valid"].cpu().numpy(), valid)
    assert R.same_f32(pol.weights.cpu().numpy(), w), "weights after q_learn call %d" % it
    assert R.same_f32(pol.bias.cpu().numpy(), b), "bias after q_learn call %d" % it
    assert not pol.acc_weights.any() and not pol.acc_bias.any(), "the accumulators are cleared behind the update"
    assert int(pol.step.item()) == T * (it + 1)
    kinds |= set(np.unique(step_type).tolist())
    assert valid.any() and (~valid).any() and (delta[valid] != 0).any()
  assert {N.FIRST, N.MID, N.LAST} <= kinds, "episodes end and auto-reset inside the buffer"
  if name.endswith("_ma"):
    assert N.DEAD in kinds, "an agent finishes before the other"
  assert np.isfinite(w).all()
  eng.close()


def test_policy_step_n_is_what_it_was_and_rollout_keeps_obs0():
  """Two engines from the same state and the same policy tables: policy_step_n and policy_rollout play the same tape and write the
  same buffers; the rollout also returns the rows the first action was chosen on, which the write_every call overwrote."""
  T, n = 9, 70
  spec = make_spec("island_navigation_ex", level=9, max_iterations=7)
  outs = ("board", "reward", "step_type")
  res = []
  for keep in (False, True):
    eng = BatchedEngine(spec, n, device=U.DEV, outputs=outs)
    eng.reset()
    pol = TablePolicy(eng, seed=3, epsilon=0.3)
    U.fill_policy(pol, np.random.default_rng(6), True, with_index=False)
    start = eng._bufs["board"][:n].cpu().numpy().copy()
    out = eng.policy_rollout(pol, T) if keep else eng.policy_step_n(pol, T, write_every=True)
    assert ("obs0" in out) == keep
    if keep:
      assert np.array_equal(out["obs0"].cpu().numpy(), start)
      assert not np.array_equal(out["board"][-1].cpu().numpy().reshape(n, -1), start), "the last step overwrote the row obs0 was read from"
    res.append({k: v.cpu().numpy() for k, v in out.items() if k != "obs0"})
    eng.close()
  assert sorted(res[0]) == sorted(res[1])
  for k in res[0]:
    assert np.array_equal(res[0][k], res[1][k]), k


# ---- capture --------------------------------------------------------------------------------------------------------------------
def test_scores_accumulate_apply_under_graph_capture():
  """One serial chain on the caller's stream: scores -> accumulate -> apply captured by torch.cuda.graph on a side stream after a
  warm-up outside the capture, replayed twice over inputs refilled in place."""
  T, n = 4, 70
  spec, eng, rng, pol, w, b, idx, c_a, off_a, row = _setup("island_l9_board", n, 1, 77, mixed=False)
  A, NA, n_pad, lr = spec.A, pol.n_actions, eng.n_pad, 0.01
  code_of = pol.code_of.cpu().numpy()
  obs0 = torch.zeros((n_pad, row), dtype=torch.uint8, device=U.DEV)
  obs = torch.zeros((T, n_pad, row), dtype=torch.uint8, device=U.DEV)
  acts = torch.zeros((T, n, A), dtype=torch.int8, device=U.DEV)
  coef = torch.zeros((T, n, A), dtype=torch.float64, device=U.DEV)
  cases = []
  for k in range(3):
    O = _observations(rng, spec, T + 1, n_pad, n, row)
    actions, cf = _transition_inputs(rng, 17 * k, T, n, A, NA, pol.action_lo)
    cases.append((O, actions, cf))

  def fill(c):
    obs0.copy_(_dev(c[0][0])); obs.copy_(_dev(c[0][1:])); acts.copy_(_dev(c[1])); coef.copy_(_dev(c[2]))
    pol.weights.copy_(_dev(w)); pol.bias.copy_(_dev(b))

  def chain():
    res = eng.policy_scores(pol, T, obs0, obs, acts)
    eng.policy_accumulate(pol, coef, T, obs0, obs, acts, frac_bits=FRAC)
    eng.policy_apply(pol, lr, clear=True)
    return res

  fill(cases[0])
  torch.cuda.synchronize()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    res = chain()                                            # warm-up outside the capture: the result tensors and accumulators exist
  side.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    res2 = chain()
  assert all(res2[k].data_ptr() == res[k].data_ptr() for k in res)
  for c in cases[1:]:
    fill(c)
    for k in res:
      res[k].fill_(-777.25)
    graph.replay()
    torch.cuda.synchronize()
    want = R.scores(c[0][:, :n], code_of, w, b, None, c_a, off_a, c[1], pol.action_lo)
    assert R.same_f32(res["scores"].cpu().numpy(), want[0]) and R.same_f64(res["vmax"].cpu().numpy(), want[1])
    assert R.same_f64(res["chosen"].cpu().numpy(), want[2])
    acc_w, acc_b = np.zeros(w.shape, np.int64), np.zeros(b.shape, np.int64)
    live = R.accumulate(acc_w, acc_b, c[0][:, :n], code_of, None, c_a, off_a, c[1], c[2], FRAC, pol.action_lo)
    assert live.any()
    assert R.same_f32(pol.weights.cpu().numpy(), R.apply(w, acc_w, lr, FRAC))
    assert R.same_f32(pol.bias.cpu().numpy(), R.apply(b, acc_b, lr, FRAC))
    assert not pol.acc_weights.any() and not pol.acc_bias.any()
  eng.close()
