"""Every output subset of tests/output_subsets.py against the full-output run, on every launch path of every row of
tests/launch_paths.py.  The requested outputs are the runtime mask from which the host lays out every env-wave's LDS
(csrc/sgw_common.hpp lds_plan): a dropped output moves every later region, picks one of four homes for the parked cumulative
vectors, decides whether the board image is staged, and the small outputs leave through LDS on the pipelined rollout and from
registers elsewhere.  So each subset must give, byte for byte, what the same fields of the full-output run hold (the
sgw_step record of test_launch_paths_gpu.case(), which that module pins to the C oracle at every step), the same state and
finished-episode returns, and must write nothing outside its buffers (GuardedEngine: 4096 guard bytes around every output)."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import EngineGroup
from tests import launch_paths as LP
from tests import output_subsets as OS
from tests.launch_paths import DEV, start
from tests.test_launch_paths_gpu import CALLS, SEED, T, case, check_returns

pytestmark = pytest.mark.gpu
PATHS = ("step_n", "replay", "rollout")
MAX_REPORTED = 8

_EXPECTED = {}


def expected_dev(c, field):
  """OS.expected(c, field) as a time-major device tensor [S + 1, E, ...] (cached: computed once per row and field)."""
  key = (c["row"]["id"], field)
  if key not in _EXPECTED:
    _EXPECTED[key] = torch.from_numpy(np.ascontiguousarray(np.moveaxis(OS.expected(c, field), 0, 1))).to(DEV)
  return _EXPECTED[key]


def _equal_dev(g, w):
  if g.shape != w.shape or g.dtype != w.dtype:
    return torch.zeros((), dtype=torch.bool, device=g.device)
  same = g == w
  if g.is_floating_point():
    same = same | ((g != g) & (w != w))                   # NaN == NaN (metrics, discount), as LP._same
  return same.all()


def compare(got, want, s0, label, errors):
  """got {field: [S, n, ...] device tensor} against want {field: [S, n, ...] device tensor}, exactly; every difference is added to
  `errors` with the field and the first differing (env, step), steps counted from s0.  One synchronisation per call."""
  fields = sorted(got)
  if not fields:
    return
  flags = torch.stack([_equal_dev(got[f], want[f]) for f in fields]).cpu().numpy()
  for f, ok in zip(fields, flags):
    if ok:
      continue
    g, w = got[f].cpu().numpy(), want[f].cpu().numpy()
    if g.shape != w.shape or g.dtype != w.dtype:
      errors.append("%s: %s is %s %s, expected %s %s" % (label, f, g.dtype, g.shape, w.dtype, w.shape))
      continue
    e, t = OS.first_difference(g, w)
    errors.append("%s: field %s first differs at (env %d, step %d)" % (label, f, e, s0 + t))


def lead(o, single):
  """The engine's views as [S, n, ...]: a single step's [n, ...] gets a leading axis."""
  return {f: (v[None] if single else v) for f, v in o.items()}


def want_steps(c, fields, s0, S):
  return {f: expected_dev(c, f)[s0:s0 + S] for f in fields}


def finish(errors):
  assert not errors, "%d difference(s):\n%s" % (len(errors), "\n".join(errors[:MAX_REPORTED]))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS])
def test_subset_outputs_equal_full_run(row_id, path):
  """Each entry of subsets(row): the row's calls of the path with exactly those outputs; after every call each requested field
  equals the full run's on that call's steps and the returned dict has exactly the requested keys; at the end the state, the
  returns (accumulate on: the oracle's finished episodes; off: all zeros) and the guard bytes."""
  c = case(row_id)
  row, spec, acts = c["row"], c["spec"], c["acts"]
  n, n_calls = row["n"], row["calls"]
  errors = []
  buf = torch.empty_like(acts[:T])
  for outputs, acc in OS.subsets(row, spec, path):
    label = "%s %s outputs=%s accumulate=%s" % (row_id, path, outputs, acc)
    try:
      eng = OS.make_guarded(row, spec, c["inp"], outputs)
      start(eng, row)
      for k in range(n_calls):
        if path == "step_n":                      # one buffer refilled in place: call 0 direct, call 1 the capture, then replays
          buf.copy_(acts[k * T:(k + 1) * T])
          o = eng.step_n(buf, write_every=True, accumulate=acc)
        elif path == "replay":
          o = eng.replay(acts[k * T:(k + 1) * T], write_every=True, accumulate=acc)
        else:
          o = eng.rollout(T, SEED, step0=k * T, write_every=True, accumulate=acc)
        assert sorted(o) == sorted(outputs), "%s: call %d returned %s" % (label, k, sorted(o))
        compare(o, want_steps(c, outputs, 1 + k * T, T), 1 + k * T, "%s call %d" % (label, k), errors)
      if not torch.equal(eng.get_state()[:, :n], c["states"][n_calls * T]):
        errors.append("%s: final state differs from the sgw_step engine" % label)
      ret = eng.read_returns()
      if acc:
        check_returns(c, ret, n_calls * T, label)
      elif bool((ret != 0).any()):
        errors.append("%s: accumulate off, read_returns() = %s" % (label, ret.cpu().numpy()))
      broken = eng.guards_intact()
      if broken:
        errors.append("%s: guard bytes changed next to %s" % (label, broken))
      eng.close()
    except N.SgwError as ex:                      # a subset of a set the row runs needs less LDS: nothing documents a refusal
      pytest.fail("%s: refused or failed: %s" % (label, ex))
    if len(errors) >= MAX_REPORTED:
      break
  finish(errors)


def reset_sequence(c, outputs, on_call):
  """start, four sgw_step calls, reset(mask[e] = e % 3 == 0), four more, reset() of everything, two more: 13 calls (the families
  whose oracle records two resets start with both and count them as one).  on_call(index, label, views) after each; returns the
  engine (open)."""
  row, acts = c["row"], c["acts"]
  eng = OS.make_guarded(row, c["spec"], c["inp"], outputs)
  mask = (torch.arange(row["n"], device=DEV) % 3 == 0).to(torch.uint8)
  i = 0
  on_call(i, "start", start(eng, row))
  t = 0
  for what, steps in (("step", 4), ("reset(mask)", None), ("step", 4), ("reset()", None), ("step", 2)):
    for _ in range(steps or 1):
      i += 1
      if what == "step":
        o = eng.step(acts[t]); t += 1
      else:
        o = eng.reset(mask) if what == "reset(mask)" else eng.reset()
      on_call(i, what, o)
  assert i == 12
  return eng


@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS])
def test_subset_resets_equal_full_run(row_id):
  """The one-step kernel and both resets with every subset, against a full-output engine run through the same 13 calls: after
  each call the requested fields are equal over all n rows -- the unmasked rows of the masked reset included, which must keep
  what the previous step wrote (the masked reset drains per active lane, not cooperatively) -- the states are equal at the end
  and the guards intact.  The start and the first four steps are also compared with the sgw_step record.  The full-output side
  of a masked reset is what tests/test_masked_reset_gpu.py pins to the oracle on every family; here it is the reference (run
  once per row and kept)."""
  c = case(row_id)
  row, spec = c["row"], c["spec"]
  n = row["n"]
  errors, full_rec = [], []
  full = OS.full_outputs(row, spec)

  def keep(i, what, o):
    full_rec.append({f: v.clone() for f, v in o.items()})
    if i <= 4:
      compare(lead(o, True), want_steps(c, full, i, 1), i, "%s full outputs call %d (%s)" % (row_id, i, what), errors)

  eng = reset_sequence(c, full, keep)
  full_state = eng.get_state()[:, :n].clone()
  assert not eng.guards_intact(), "%s full outputs: guard bytes changed next to %s" % (row_id, eng.guards_intact())
  eng.close()
  finish(errors)
  for outputs in dict.fromkeys(o for o, _ in OS.subsets(row, spec, "reset")):
    label = "%s resets outputs=%s" % (row_id, outputs)

    def same(i, what, o):
      assert sorted(o) == sorted(outputs), "%s: call %d returned %s" % (label, i, sorted(o))
      compare(lead(o, True), lead({f: full_rec[i][f] for f in outputs}, True), i, "%s call %d (%s)" % (label, i, what), errors)
      if i <= 4:
        compare(lead(o, True), want_steps(c, outputs, i, 1), i, "%s call %d (%s) against sgw_step" % (label, i, what), errors)

    try:
      eng = reset_sequence(c, outputs, same)
      if not torch.equal(eng.get_state()[:, :n], full_state):
        errors.append("%s: final state differs from the full-output engine's" % label)
      broken = eng.guards_intact()
      if broken:
        errors.append("%s: guard bytes changed next to %s" % (label, broken))
      eng.close()
    except N.SgwError as ex:
      pytest.fail("%s: refused or failed: %s" % (label, ex))
    if len(errors) >= MAX_REPORTED:
      break
  finish(errors)


def member_outputs(i, c):
  return [(), ("reward",), ("board", "done"), OS.full_outputs(c["row"], c["spec"])][i]


@pytest.mark.parametrize("gid,members", LP.GROUPS, ids=[g for g, _ in LP.GROUPS])
def test_group_members_with_different_subsets(gid, members):
  """One launch over members that ask for different outputs (the launch takes the largest member's LDS, each member keeps its own
  plan): CALLS calls of EngineGroup.step_n (direct, capture, replay) with accumulate on, then one group rollout."""
  cs = [case(m) for m in members]
  outs_of = [member_outputs(i, c) for i, c in enumerate(cs)]
  engines = [OS.make_guarded(c["row"], c["spec"], c["inp"], o) for c, o in zip(cs, outs_of)]
  for c, e in zip(cs, engines):
    start(e, c["row"])
  grp = EngineGroup(engines)
  bufs = [torch.empty_like(c["acts"][:T]) for c in cs]
  errors = []
  for k in range(CALLS):
    for b, c in zip(bufs, cs):
      b.copy_(c["acts"][k * T:(k + 1) * T])
    outs = grp.step_n(bufs, write_every=True, accumulate=True)
    for c, o, want in zip(cs, outs, outs_of):
      label = "%s member %s outputs=%s group step_n call %d" % (gid, c["row"]["id"], want, k)
      assert sorted(o) == sorted(want), "%s returned %s" % (label, sorted(o))
      compare(o, want_steps(c, want, 1 + k * T, T), 1 + k * T, label, errors)
  for c, e in zip(cs, engines):
    check_returns(c, e.read_returns(), CALLS * T, "%s member %s group step_n" % (gid, c["row"]["id"]))
    if not torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][CALLS * T]):
      errors.append("%s member %s: state after the step_n calls" % (gid, c["row"]["id"]))
  outs = grp.rollout(T, SEED, step0=CALLS * T, write_every=True)
  for c, o, e, want in zip(cs, outs, engines, outs_of):
    label = "%s member %s outputs=%s group rollout" % (gid, c["row"]["id"], want)
    assert sorted(o) == sorted(want), "%s returned %s" % (label, sorted(o))
    compare(o, want_steps(c, want, 1 + CALLS * T, T), 1 + CALLS * T, label, errors)
    if not torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][(CALLS + 1) * T]):
      errors.append("%s: state after the rollout" % label)
    check_returns(c, e.read_returns(), CALLS * T, label)         # the rollout ran with accumulate off: the sums stay
    broken = e.guards_intact()
    if broken:
      errors.append("%s: guard bytes changed next to %s" % (label, broken))
  grp.close()
  for e in engines:
    e.close()
  finish(errors)

