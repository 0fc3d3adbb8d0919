"""Every launch path of every row of tests/launch_paths.py against the C oracle, byte for byte, on every output the oracle
records at every step: sgw_step_n over ONE actions buffer refilled in place (call 0 direct, call 1 captured, later calls
hipGraph replays) on the default and on a side stream, sgw_replay, sgw_rollout (its in-kernel Philox stream =
sgw_fill_actions, copied back for the oracle), and every group member through sgw_group_step_n (direct, capture, replay) and
sgw_group_rollout.  Each path also equals an engine stepped one sgw_step at a time (the outputs the oracle has no counterpart
for, the final state), and read_returns() equals the summed returns of the oracle's finished episodes.  Setters called after
a capture (new episode-bit seed, new explicit bits, a second random stream, a new stream seed) must reach the next three calls
of an engine and of a group: the stale graph's direct launch, the recapture and its replay."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine, EngineGroup
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests.launch_paths import DEV, make_engine, split_views, start, to_np

pytestmark = pytest.mark.gpu
T, CALLS, SEED = 16, 3, 0x1A7C        # T >= step_graphs_min_T (8): the second call of a buffer is captured
AFTER = 3                             # setter tests: calls after the setter (the stale graph's direct launch, capture, replay)


def steps_of(row):
  """Steps a row's action stream covers: its step_n / replay / rollout calls; groups: CALLS step_n calls, then one rollout;
  setter tests: CALLS calls, then AFTER more."""
  return max(row["calls"], CALLS + 1, CALLS + AFTER) * T


_CASES = {}


def case(row_id):
  """Per row (cached): spec, inputs, the device action stream of steps_of(row) steps, the oracle's arrays, and a reference engine's
  outputs of every step (reset, then one sgw_step per step) with its state after every multiple of T steps.  The reference
  engine itself is compared with the oracle at every step, and its generator position with the oracle's at every multiple of T
  (the multi-agent families)."""
  if row_id in _CASES:
    return _CASES[row_id]
  row = LP.BY_ID[row_id]
  spec = make_spec(row["name"], **row["kw"])
  inp = LP.inputs(row, spec, LP.ROWS.index(row))
  ref = make_engine(row, spec, inp)
  S = steps_of(row)
  acts = ref.fill_actions(S, SEED).clone()
  rec = {k: [v.clone()] for k, v in start(ref, row).items()}
  states = {}
  for t in range(S):
    for k, v in ref.step(acts[t]).items():
      rec[k].append(v.clone())
    if (t + 1) % T == 0:
      states[t + 1] = ref.get_state()[:, :row["n"]].clone()
  torch.cuda.synchronize()
  got = to_np({k: torch.stack(v) for k, v in rec.items()}, True)
  want = LP.run_oracle(row, acts.cpu().numpy(), inp)
  c = dict(row=row, spec=spec, inp=inp, acts=acts, want=want, ref=got, states=states)
  check(c, {k: v[:, 1:] for k, v in got.items()}, 1, "sgw_step")
  if row["rng"]:
    for s, st in states.items():
      assert not LP.rng_mismatch(row, st.cpu().numpy(), want, s), "%s sgw_step: generator position after %d steps" % (row_id, s)
  if row["oracle"] == "scalar":
    st, cum = want["step_type"][..., None], want["cumulative"]
  else:
    st, cum = got["step_type"], got["cumulative"].reshape(row["n"], S + 1, -1)
  # read_returns after the row's own calls and after the groups' CALLS step_n calls
  c["returns"] = {s: LP.finished_returns(st[:, :s + 1], cum[:, :s + 1]) for s in {row["calls"] * T, CALLS * T}}
  assert c["returns"][row["calls"] * T][-1] > 0, "no episode ends inside the run: pick kwargs with shorter episodes"
  ref.close()
  _CASES[row_id] = c
  return c


def check(c, got, s0, label):
  """got {field: [E, S, ...]} = the outputs of steps s0 .. s0 + S - 1: equal to the oracle and to the sgw_step engine."""
  row, spec = c["row"], c["spec"]
  S = next(iter(got.values())).shape[1]
  views = split_views(spec, got["views"]) if "views" in got else None
  bad = LP.oracle_mismatches(row, spec, got, c["want"], s0, views=views)
  assert not bad, "%s %s steps %d..%d differ from the oracle in %s" % (row["id"], label, s0, s0 + S - 1, bad)
  if label != "sgw_step":
    for k in row["outs"]:
      g, w = got[k], c["ref"][k][:, s0:s0 + S]
      assert LP._same(g, w), "%s %s steps %d..%d: %s differs from the sgw_step engine" % (row["id"], label, s0, s0 + S - 1, k)


def check_returns(c, r, steps, label):
  """read_returns after `steps` steps: the count of finished episodes exactly; the sums up to the order of the device's
  float64 atomic adds."""
  r, w = r.cpu().numpy(), c["returns"][steps]
  assert r[-1] == w[-1], "%s %s: %d finished episodes, the oracle has %d" % (c["row"]["id"], label, r[-1], w[-1])
  assert np.allclose(r[:-1], w[:-1], rtol=1e-12, atol=1e-9), "%s %s: returns %s, the oracle's %s" % (c["row"]["id"], label, r, w)


PATHS = ("step_n", "step_n_side", "replay", "rollout")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS])
def test_launch_path_matches_oracle(row_id, path):
  c = case(row_id)
  row, spec, acts = c["row"], c["spec"], c["acts"]
  eng = make_engine(row, spec, c["inp"])
  start(eng, row)
  buf = torch.empty_like(acts[:T])
  torch.cuda.synchronize()
  stream = torch.cuda.Stream(DEV) if path == "step_n_side" else torch.cuda.current_stream(DEV)
  calls, n_calls = [], row["calls"]
  with torch.cuda.stream(stream):
    for k in range(n_calls):
      if path.startswith("step_n"):               # call 0: direct launches, call 1: capture + replay, call 2: replay
        buf.copy_(acts[k * T:(k + 1) * T])
        o = eng.step_n(buf, write_every=True, accumulate=True)
      elif path == "replay":
        o = eng.replay(acts[k * T:(k + 1) * T], write_every=True, accumulate=True)
      else:
        o = eng.rollout(T, SEED, step0=k * T, write_every=True, accumulate=True)
      calls.append({f: v.clone() for f, v in o.items()})
    ret = eng.read_returns()
    state = eng.get_state()[:, :row["n"]]
  torch.cuda.synchronize()
  for k, o in enumerate(calls):
    check(c, to_np(o, True), 1 + k * T, "%s call %d" % (path, k))
  assert torch.equal(state, c["states"][n_calls * T]), "%s %s: final state differs from the sgw_step engine" % (row_id, path)
  check_returns(c, ret, n_calls * T, path)
  eng.close()


@pytest.mark.parametrize("gid,members", LP.GROUPS, ids=[g for g, _ in LP.GROUPS])
def test_group_paths_match_oracle(gid, members):
  cs = [case(m) for m in members]
  engines = [make_engine(c["row"], c["spec"], c["inp"]) for c in cs]
  for c, e in zip(cs, engines):
    start(e, c["row"])
  grp = EngineGroup(engines)
  bufs = [torch.empty_like(c["acts"][:T]) for c in cs]
  torch.cuda.synchronize()
  for k in range(CALLS):                           # direct, capture, replay; the actions refilled in place
    for b, c in zip(bufs, cs):
      b.copy_(c["acts"][k * T:(k + 1) * T])
    outs = grp.step_n(bufs, write_every=True, accumulate=True)
    torch.cuda.synchronize()
    for c, o in zip(cs, outs):
      check(c, to_np(o, True), 1 + k * T, "%s group step_n call %d" % (gid, k))
  for c, e in zip(cs, engines):
    check_returns(c, e.read_returns(), CALLS * T, "%s group step_n" % gid)
    assert torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][CALLS * T]), "%s %s: state" % (gid, c["row"]["id"])
  outs = grp.rollout(T, SEED, step0=CALLS * T, write_every=True)
  torch.cuda.synchronize()
  for c, o, e in zip(cs, outs, engines):
    check(c, to_np(o, True), 1 + CALLS * T, "%s group rollout" % gid)
    assert torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][(CALLS + 1) * T]), "%s %s: state after the rollout" % (gid, c["row"]["id"])
  grp.close()
  for e in engines:
    e.close()


def test_groups_cover_every_member_row():
  members = [m for _, ms in LP.GROUPS for m in ms]
  assert sorted(members) == sorted(r["id"] for r in LP.ROWS if r["tag"]), "every member row is in exactly one group"
  assert any(len(ms) == 4 for _, ms in LP.GROUPS) and any(LP.BY_ID[m]["n"] < 64 for m in members)
  assert all(LP.BY_ID[m]["n"] % 64 for m in members)


@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS if r["state_words"]])
def test_island_rows_run_the_declared_state_variant(row_id):
  """TAG_ISLAND_PACKED runs the 10-word packed state, TAG_ISLAND the 22-word plain one."""
  row = LP.BY_ID[row_id]
  e = BatchedEngine(make_spec(row["name"], **row["kw"]), 64, device=DEV)
  assert N.lib().sgw_state_words(e._h) == row["state_words"]
  e.close()


@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS if not r["tag"]])
def test_group_refuses_non_member_rows(row_id):
  row = LP.BY_ID[row_id]
  a = BatchedEngine(make_spec("island_navigation_ex"), 128, device=DEV)
  b = BatchedEngine(make_spec(row["name"], **row["kw"]), 65, device=DEV, outputs=("board",))
  with pytest.raises(N.SgwError, match="not a group member"):
    EngineGroup([a, b])
  a.close(); b.close()


# setter changes after a capture: (row, change) -- the second value differs from the first
def _new_seed(kind):
  def f(e, c):
    if kind == "ep_seed":
      e.set_episode_bits(None, seed=c["inp"]["bits_seed"] + 77)
    elif kind == "ep_bits":
      e.set_episode_bits(1 - c["inp"]["bits"])
    elif kind == "rand_stream":
      e.set_random_stream(np.random.default_rng(99).random(c["inp"]["rand"].shape))
    else:
      e.set_random_stream(None, seed=c["inp"]["rand_seed"] + 77)
  return f


SETTERS = [("ep_seed", "safe_interruptibility_ex"), ("ep_bits", "safe_interruptibility"), ("rand_stream", "tomato_watering"),
           ("rand_seed", "tomato_crmdp")]


def _stepped(c, change, at):
  """One sgw_step per step from a reset over (CALLS + AFTER) * T steps, `change` applied before step `at`: outputs
  [E, S, ...] and state."""
  e = make_engine(c["row"], c["spec"], c["inp"])
  rec = {k: [v.clone()] for k, v in start(e, c["row"]).items()}
  for t in range((CALLS + AFTER) * T):
    if t == at:
      change(e, c)
    for k, v in e.step(c["acts"][t]).items():
      rec[k].append(v.clone())
  st = e.get_state()[:, :c["row"]["n"]].clone()
  torch.cuda.synchronize()
  e.close()
  return to_np({k: torch.stack(v) for k, v in rec.items()}, True), st


@pytest.mark.parametrize("kind,row_id", SETTERS)
def test_engine_setter_after_capture_reaches_the_next_call(kind, row_id):
  c = case(row_id)
  change = _new_seed(kind)
  want, want_state = _stepped(c, change, CALLS * T)
  e = make_engine(c["row"], c["spec"], c["inp"])
  start(e, c["row"])
  buf = torch.empty_like(c["acts"][:T])
  for k in range(CALLS + AFTER):                   # direct, capture, replay; the setter; direct, capture, replay again
    if k == CALLS:
      change(e, c)
    buf.copy_(c["acts"][k * T:(k + 1) * T])
    o = to_np(e.step_n(buf, write_every=True), True)
    if k >= CALLS:
      for f in c["row"]["outs"]:
        assert LP._same(o[f], want[f][:, 1 + k * T:1 + (k + 1) * T]), \
            "%s: %s of call %d after the setter differs from sgw_step" % (kind, f, k - CALLS)
  assert torch.equal(e.get_state()[:, :c["row"]["n"]], want_state)
  e.close()


@pytest.mark.parametrize("kind,row_id", SETTERS)
def test_group_setter_after_capture_reaches_the_next_call(kind, row_id):
  """A member setter after EngineGroup.step_n captured: the group's next call must use the new value (the capture holds the
  members' launch arguments by value, so it is stale), and so must the recapture and its replay in the two calls after it."""
  cs = [case(row_id), case("island_ex_packed")]
  change = _new_seed(kind)
  want = [_stepped(cs[0], change, CALLS * T), _stepped(cs[1], lambda e, c: None, CALLS * T)]
  engines = [make_engine(c["row"], c["spec"], c["inp"]) for c in cs]
  for c, e in zip(cs, engines):
    start(e, c["row"])
  grp = EngineGroup(engines)
  bufs = [torch.empty_like(c["acts"][:T]) for c in cs]
  for k in range(CALLS + AFTER):
    if k == CALLS:
      change(engines[0], cs[0])
    for b, c in zip(bufs, cs):
      b.copy_(c["acts"][k * T:(k + 1) * T])
    outs = [to_np(o, True) for o in grp.step_n(bufs, write_every=True)]
    if k >= CALLS:
      for c, o, (w, _) in zip(cs, outs, want):
        for f in c["row"]["outs"]:
          assert LP._same(o[f], w[f][:, 1 + k * T:1 + (k + 1) * T]), \
              "%s: member %s, %s of call %d after the setter differs from sgw_step" % (kind, c["row"]["id"], f, k - CALLS)
  for c, (_, ws), e in zip(cs, want, engines):
    assert torch.equal(e.get_state()[:, :c["row"]["n"]], ws), "%s: member %s state" % (kind, c["row"]["id"])
  grp.close()
  for e in engines:
    e.close()
