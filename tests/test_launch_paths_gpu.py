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
# the matrix itself (case, check, check_returns, run_path, run_group) lives in launch_paths.py; other test modules import it from here
from tests.launch_paths import (AFTER, CALLS, DEV, PATHS, SEED, T, case, check, check_returns, make_engine, start, steps_of,  # noqa: F401
                                to_np)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS])
def test_launch_path_matches_oracle(row_id, path):
  LP.run_path(row_id, path)


@pytest.mark.parametrize("gid,members", LP.GROUPS, ids=[g for g, _ in LP.GROUPS])
def test_group_paths_match_oracle(gid, members):
  LP.run_group(gid, members)


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
