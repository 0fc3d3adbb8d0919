"""Every packed state field at its limit (tests/state_fields.py), on the device.  Per case:

  step path   the tape through sgw_step_n, so the state goes through memory after every step: calls of up to 4096 steps whose
              last row is compared with the C oracle, and around every crossing (255 / 256, 32767 / 32768, the episode's end and 8
              steps into the next episode) calls of at most 64 steps with every row of every output compared, bit for bit
  fused path  sgw_replay of the same tape (state in registers): the same rows and the same final state as the step path
  checkpoint  a snapshot one step before the limit (the countdown cases: while the countdown is above 255) restored into a new
              engine continues like the first one to the end of the window
  log         sgw_log_episodes over the window of the episode's end: one record per env, its length the oracle's end frame
  packed      sgw_state_words on both sides of packable()'s boundary; the packed cases once more under SGW_ISLAND_PLAIN_STATE

tests/test_state_fields.py shows on the oracle alone that each tape reaches its limit.

Measured on one MI355X (E envs, T steps, what the oracle shows; seconds: oracle with 8 threads / step path / replay):
  island_l9_65535                 131  65543  frame 65535, the five visit counters >= 65529, satiations -65535    1.0 / 0.50 / 0.09
  island_{default,saturating,saturating_packed}_{655,656}
                                  131  663|4  cumulative +-32750 (655: 10 words where it packs), +-32800 (656)    0.0 / 0.01 / 0.00
  firemaker_duration_{3,254,255,300,1000}
                                  131    700  countdown 4, 255, 256, 301, 1001 in every env                      0.3 / 0.06 / 0.05
  firemaker_32769                  65  10931  ends on frame 32769                                                3.4 / 1.32 / 1.17
  firemaker_32769_withheld         65  16393  ends on frame 32770 (two plays a round)                            3.3 / 1.35 / 1.11
  island_ma_65534_odd              67  32776  ends on frame 65535, GapVisits 32768 / 32767, 3 idle rounds        0.4 / 0.65 / 0.18
  savanna_1_65535                  67  65543  ends on frame 65535, 3 idle rounds                                 2.7 / 6.96 / 0.46
  savanna_2_65534_odd              67  32776  ends on frame 65535, 3 idle rounds                                 2.1 / 3.63 / 0.36
  {boat_race_ex,island_navigation,safe_interruptibility,conveyor_belt}_65535
                                  131  65543  ends on frame 65535                                                0.2 / 0.39 / 0.09
  {side_effects_sokoban,tomato_watering,rocks_diamonds,whisky_gold,friend_foe}_100
                                  131    108  ends on frame 100, the families' own limit                         0.0 / 0.00 / 0.00
Before the fixes the firemaker rows with a duration >= 255 failed on every test here (the state held 0, 45 and 233 where the
oracle's countdown is 256, 301 and 1001; boards, rewards and windows differed from step 1 on, and replay from step_n), and two
agents at max_iterations 65535 reported frame 0 instead of 65536 on the idle rounds after the episode's end."""
import time

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import EpisodeLog
from tests import launch_paths as LP
from tests import state_fields as SF

pytestmark = pytest.mark.gpu

CASE_IDS = [c["id"] for c in SF.CASES]
_RUNS = {}


def _tape(case, spec):
  acts = SF.actions(case, spec)                                           # [E, T(, A)]
  return torch.from_numpy(np.ascontiguousarray(np.moveaxis(acts, 0, 1))).to(LP.DEV)


def _rows(case, spec, out, every):
  got = LP.to_np({k: v.clone() for k, v in out.items()}, every)
  return got, (LP.split_views(spec, got["views"]) if "views" in got else None)


def _run(case, path, until=None, from_state=None):
  """The case's segments through `path` ("step_n" / "replay") on a fresh engine: {(a, b): rows}, the states after the
  checkpoint step and after the last step, the episode log of the end window.  from_state: (step, snapshot) to start from
  instead of a reset; until: the last step to run."""
  spec = SF.spec_of(case)
  inp = SF.inputs(case, spec)
  acts = _tape(case, spec)
  eng = LP.make_engine(case, spec, inp)
  if case["state_words"]:
    assert N.lib().sgw_state_words(eng._h) == case["state_words"]
  t0 = 0
  if from_state is None:
    LP.start(eng, case)
  else:
    t0, snap = from_state
    eng.set_state(snap)
  res = dict(rows={}, views={}, states={}, log=None, spec=spec)
  cp, end = SF.checkpoint_step(case), SF.end_step(case)
  torch.cuda.synchronize()
  tic = time.time()
  for a, b, every in SF.segments(case):
    if b <= t0 or (until is not None and a > until):
      continue
    assert a == t0 + 1, "a call starts where the last one ended"
    t0 = b
    out = getattr(eng, path)(acts[a - 1:b], write_every=every)
    if every and a <= end <= b and from_state is None and path == "step_n":
      log = EpisodeLog(eng, 2 * case["n"], fields=("env", "step", "length"))
      eng.log_episodes(log, step_base=a)
      res["log"] = {k: v.cpu().numpy() for k, v in log.records().items()}
    key = (a, b) if every else (b, b)
    res["rows"][key], res["views"][key] = _rows(case, spec, out, every)
    if b in (cp, case["T"]) or (until is not None and b == until):
      full = eng.get_state()
      res["states"][b] = full[:, :case["n"]].clone()
      if b == cp:
        res["snapshot"] = full.clone()                                  # [words, N_pad]: what sgw_set_state takes
  torch.cuda.synchronize()
  res["seconds"] = time.time() - tic
  eng.close()
  return res


def _step_run(case):
  if case["id"] not in _RUNS:
    _RUNS[case["id"]] = _run(case, "step_n")
  return _RUNS[case["id"]]


def _same_rows(case, label, got, ref, keys):
  for key in keys:
    for f in case["outs"]:
      g, w = got["rows"][key][f], ref["rows"][key][f]
      assert LP._same(g, w), "%s %s steps %d..%d: %s differs from the step path" % (case["id"], label, key[0], key[1], f)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_step_path_matches_the_oracle_at_the_limit(case_id):
  case = SF.BY_ID[case_id]
  o = SF.oracle_case(case)
  assert not SF.reached(case, o)
  run = _step_run(case)
  print("%s: E=%d T=%d oracle %.1f s, step path %.2f s" % (case_id, case["n"], case["T"], o["seconds"], run["seconds"]))
  bad = []
  for key in SF.compared(case):
    miss = LP.oracle_mismatches(case, run["spec"], run["rows"][key], o["want"][key], 0, views=run["views"][key])
    if miss:
      bad.append((key, miss))
  assert not bad, "%s: the step path differs from the oracle at steps %s%s" % (
      case_id, bad[:6], " and %d more ranges" % (len(bad) - 6) if len(bad) > 6 else "")
  log = run["log"]                                                     # one first episode per env, as long as the oracle's
  first = np.unique(log["env"], return_index=True)[1]
  assert len(first) == case["n"], "sgw_log_episodes: %d envs end an episode in the end window, not %d" % (len(first), case["n"])
  assert np.array_equal(log["length"][first], o["end_frame"][log["env"][first]]), "sgw_log_episodes: lengths differ from the oracle's end frames"
  assert np.array_equal(log["step"][first], o["end_step"][log["env"][first]])


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_fused_replay_matches_the_step_path_at_the_limit(case_id):
  case = SF.BY_ID[case_id]
  ref = _step_run(case)
  got = _run(case, "replay")
  print("%s: replay %.2f s" % (case_id, got["seconds"]))
  _same_rows(case, "replay", got, ref, SF.compared(case))
  T = case["T"]
  assert torch.equal(got["states"][T], ref["states"][T]), "%s: the final state of replay differs from the step path's" % case_id


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_checkpoint_one_step_before_the_limit_resumes_bit_for_bit(case_id):
  case = SF.BY_ID[case_id]
  ref = _step_run(case)
  cp = SF.checkpoint_step(case)
  if case["countdown"] and case["kw"]["STOP_BUTTON_PRESS_EFFECT_DURATION"] >= 255:
    above = SF.oracle_case(case)["countdown"][:, cp] > 255
    assert above.any(), "no env's countdown is above 255 at the checkpoint"
    st = ref["states"][cp].cpu().numpy().view(np.uint64)
    stored = ((st[0] >> np.uint64(16)) & np.uint64(0xff)) | ((st[0] >> np.uint64(48)) & np.uint64(0xff00))
    assert np.array_equal(stored, SF.oracle_case(case)["countdown"][:, cp].astype(np.uint64)), "the countdown in state word 0"
  (a, b), = [(a, b) for a, b, every in SF.segments(case) if a == cp + 1]
  got = _run(case, "step_n", until=b, from_state=(cp, ref["snapshot"]))
  _same_rows(case, "resumed", got, ref, [(a, b)])
  if b == case["T"]:
    assert torch.equal(got["states"][b], ref["states"][b]), "%s: the resumed engine's final state" % case_id


@pytest.mark.parametrize("case_id", [c["id"] for c in SF.CASES if c["plain_too"]])
def test_packed_plain_and_oracle_agree_at_the_boundary(case_id, monkeypatch):
  """The packed cases (sgw_state_words == 10 at max_iterations 655) once more through the plain 22-word state."""
  case = SF.BY_ID[case_id]
  ref = _step_run(case)
  monkeypatch.setenv("SGW_ISLAND_PLAIN_STATE", "1")
  plain = _run(dict(case, state_words=22), "step_n")
  _same_rows(case, "plain state", plain, ref, SF.compared(case))
  o = SF.oracle_case(case)
  for key in SF.compared(case):
    assert not LP.oracle_mismatches(case, plain["spec"], plain["rows"][key], o["want"][key], 0), key
