"""The masked-reset schedule of tests/reset_schedules.py, checked on the host for every row it is meant for: the forced calls are there, the
tapes and the cursor restate the calls, and -- from the ORACLE's records of those tapes alone -- the schedule issues at least
MIN_COVER explicit resets to an env whose latest record was FIRST, MID, LAST for every agent, and the record right after an
auto-reset, so a GPU test cannot run a schedule that misses one of them.  island_navigation_ex_ma additionally needs
MIN_PARTIAL resets while one agent is LAST or DEAD and the other is not.  (firemaker_ex_ma and aintelope_savanna have no such
state: in the reference, as in every fixture of theirs, all agents of an episode finish on the same tick.)"""
import numpy as np
import pytest

from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import reset_schedules as RS
from tests.reset_schedules import ALL_ROWS, BY_ID


@pytest.mark.parametrize("row_id", [r["id"] for r in ALL_ROWS])
def test_schedule_covers_every_class_of_reset(row_id):
  row = BY_ID[row_id]
  c = RS.oracle_case(row, make_spec(row["name"], **row["kw"]))
  sched, named, n = c["sched"], c["named"], c["row"]["n"]
  assert n == min(row["n"], 333) and all(len(call[1]) == n for call in sched if call[0] == "reset")
  n_random = len(sched) - (len(named) + 1) - (RS.LONG_STEPS + 1 if row["name"] in RS.LONG else 0)
  assert 90 <= len(sched) - (RS.LONG_STEPS if row["name"] in RS.LONG else 0) <= 100 and n_random == RS.RANDOM_CALLS
  assert not sched[named["zero"]][1].any() and sched[named["ones"]][1].all()
  assert list(np.nonzero(sched[named["lone"]][1])[0]) == [n - 1]
  assert list(np.nonzero(sched[named["wave"]][1])[0]) == list(range(64, min(128, n)))
  a, b = sched[named["overlap"]][1], sched[named["overlap"] + 1][1]
  assert (a & b).any() and (a & ~b).any() and (b & ~a).any()
  named_at = set(named.values()) | {named["overlap"] + 1}
  random_masks = [call[1] for i, call in enumerate(sched) if call[0] == "reset" and i not in named_at]
  assert 0.15 * RS.RANDOM_CALLS <= len(random_masks) <= 0.35 * RS.RANDOM_CALLS          # about one random call in four
  if n >= 256:                                                               # (a mask of 1/64 of fewer envs is often empty)
    drawn = {min(RS.DENSITIES, key=lambda d: abs(np.log(max(float(m.mean()), 1e-9) / d))) for m in random_masks}
    assert drawn == set(RS.DENSITIES), "the random resets draw 1/64, 1/8 and 1/2: %s" % sorted(drawn)
  # tapes and cursor restate the calls
  idx, tapes = c["idx"], c["tapes"]
  slot0 = tapes.reshape(n, tapes.shape[1], -1)[:, :, 0]
  assert idx.shape == (len(sched), n) and idx[-1].max() == tapes.shape[1] and idx[-1].min() < idx[-1].max()
  for e in (0, n // 2, n - 1):
    mine = [("reset" if call[0] == "reset" else "step") for call in sched if call[0] == "step" or call[1][e]]
    assert mine == ["reset" if v == RS.RESET else "step" for v in slot0[e, :len(mine)]]
    assert not (slot0[e, len(mine):] == RS.RESET).any()
  cov = RS.coverage(c["row"], sched, tapes, c["want"])
  for k in ("first", "mid", "last", "auto"):
    assert cov[k] >= RS.MIN_COVER, "%s: %s" % (row_id, cov)
  if row["oracle"] == "ima":
    assert cov["partial"] >= RS.MIN_PARTIAL, "%s: %s" % (row_id, cov)
  else:           # no per-agent termination in firemaker_ex_ma / aintelope_savanna (see above): if that changes, they need MIN_PARTIAL too
    assert cov["partial"] == 0, "%s: %s" % (row_id, cov)
