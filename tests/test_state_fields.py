"""CPU tier of tests/state_fields.py: the table names real layout files, cases and refusal tests; every driven case's tape does
what its row claims on the C oracle (every env's first episode lasts the full max_iterations and the field gets to the declared
value), so tests/test_state_fields_gpu.py cannot pass without having been at the limit; and the refusals that protect the
fields nothing drives."""
import ctypes as C
import os
import re

import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import specs
from ai_safety_gridworlds_amd.specs import make_spec
from tests import state_fields as SF

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ai_safety_gridworlds_amd", "csrc")


def test_the_table_names_layout_files_cases_and_refusal_tests():
  layouts = {f[:-4] for f in os.listdir(CSRC) if re.search(r"\bload\(State& s", open(os.path.join(CSRC, f)).read())}
  assert layouts == set(SF.LAYOUTS), "a family layout file without rows (or a row without a file): %s" % sorted(layouts ^ set(SF.LAYOUTS))
  here = open(__file__).read()
  driven = set()
  for row in SF.FIELDS:
    assert row["layout"] in layouts and row["bits"] <= 32, row
    assert row["bound"] in ("max_iterations", "spec", "board", "enum", "wraps", "i16"), row
    for c in row["cases"]:
      assert c in SF.BY_ID, "%s: no case %s" % (row["field"], c)
    driven.update(row["cases"])
    if row["bound"] == "spec":
      assert row["refusal"], "%s.%s: a field only a refusal protects names its test" % (row["layout"], row["field"])
    if row["refusal"]:
      assert "def %s(" % row["refusal"] in here, row["refusal"]
    if row["bound"] in ("wraps", "enum", "board"):
      assert not row["cases"], row
  assert driven == set(SF.BY_ID), "cases no field row names: %s" % sorted(set(SF.BY_ID) - driven)
  for lay in SF.LAYOUTS:                                   # every layout has a frame row; the ones that take max_iterations a long case
    assert any(r["layout"] == lay and r["field"] == "frame" for r in SF.FIELDS), lay


def test_every_16_bit_mask_of_a_layout_file_has_a_row():
  """Each `& 0xffff` / `& 0xff` / narrower mask in a family's load() belongs to a field some row of that layout names."""
  for lay in SF.LAYOUTS:
    text = open(os.path.join(CSRC, lay + ".hpp")).read()
    body = text[text.index("load(State& s"):text.index("store(const State& s")]
    fields = set()
    for statement in body.split(";"):
      mask = re.search(r"&\s*(0x[0-9a-f]+|\d+)\)", statement)
      name = re.search(r"s\.(\w+)", statement)
      if mask and name and int(mask.group(1), 0) >= 0xf:     # narrower: flags and enums of a few values, not counters
        fields.add(name.group(1))
    assert {"frame", "step_type", "term"} <= fields, (lay, fields)
    named = " ".join(r["field"] for r in SF.FIELDS if r["layout"] == lay)
    alias = dict(term="term_reason", actual="actual_action")
    for f in fields:
      assert alias.get(f, f) in named, "%s: load() unpacks s.%s and no row names it" % (lay, f)


@pytest.mark.parametrize("case_id", [c["id"] for c in SF.CASES])
def test_the_oracle_drives_the_field_to_its_limit(case_id):
  case = SF.BY_ID[case_id]
  o = SF.oracle_case(case)
  print("%s: E=%d T=%d oracle %.1f s; end frame %s; %s" % (case_id, case["n"], case["T"], o["seconds"], set(o["end_frame"].tolist()),
                                                          [(k, float(o[w][:, SF._column(o["dim_names"] if w == "cum_end" else o["metric_names"], k)].max()))
                                                           for w, k, _, _ in case["expect"]["reach"]]))
  bad = SF.reached(case, o)
  assert not bad, "%s: %s" % (case_id, "; ".join(bad))
  segs = SF.segments(case)
  assert segs[0][0] == 1 and segs[-1][1] == case["T"] and all(s[1] + 1 == t[0] for s, t in zip(segs, segs[1:]))
  assert all(b - a < 64 for a, b, every in segs if every)
  if case["countdown"] and case["kw"]["STOP_BUTTON_PRESS_EFFECT_DURATION"] >= 255:
    assert (o["countdown"] > 255).any(axis=0).sum() > 100, "the countdown is above 255 on too few steps to matter"


# ---- the refusals -----------------------------------------------------------------------------------------------------------------
def _create(spec_native):
  """sgw_create's return code for a spec struct: the argument checks run before the device is touched."""
  h = C.c_void_p()
  rc = N.lib().sgw_create(C.byref(spec_native), 64, 0, 0, C.byref(h))
  assert rc != 0 and not h.value
  return rc, N.lib().sgw_last_error().decode()


def test_firemaker_countdown_over_its_field_is_refused():
  """The countdown holds reload - 1 at most, in 16 bits: 1 + 1 + duration <= 65535 in make_spec (ValueError) and in sgw_create
  (SGW_ERR_ARG)."""
  ok = make_spec("firemaker_ex_ma", STOP_BUTTON_PRESS_EFFECT_DURATION=65533)
  assert ok.native.params[19] == 65535.0
  with pytest.raises(ValueError, match="16 bits"):
    make_spec("firemaker_ex_ma", STOP_BUTTON_PRESS_EFFECT_DURATION=65534)
  raw = type(ok.native).from_buffer_copy(ok.native)
  raw.params[19] = 65536.0
  rc, msg = _create(raw)
  assert rc == -1 and "countdown" in msg, (rc, msg)           # SGW_ERR_ARG


def test_max_iterations_above_the_frame_field_is_refused():
  with pytest.raises(ValueError, match="65535"):
    make_spec("island_navigation_ex", max_iterations=65536)
  ok = make_spec("island_navigation_ex", max_iterations=65535)
  raw = type(ok.native).from_buffer_copy(ok.native)
  raw.max_iterations = 65536
  rc, msg = _create(raw)
  assert rc == -1 and "max_iterations" in msg, (rc, msg)
  # A agents play a round: the episode ends on a frame of up to max_iterations + A - 1, which has to fit too
  for name, kw, agents in (("island_navigation_ex_ma", {}, 2), ("aintelope_savanna", dict(amount_agents=2), 2),
                           ("aintelope_savanna", dict(amount_agents=1), 1), ("firemaker_ex_ma", dict(amount_agents=3), 3),
                           ("firemaker_ex_ma", dict(amount_agents=2), 2), ("firemaker_ex_ma", dict(amount_agents=1), 1)):
    most = 65535 - (agents - 1)
    ok = make_spec(name, max_iterations=most, **kw)
    with pytest.raises(ValueError, match="max_iterations must be in"):
      make_spec(name, max_iterations=most + 1, **kw)
    raw = type(ok.native).from_buffer_copy(ok.native)
    raw.max_iterations = most + 1
    rc, msg = _create(raw)
    assert rc == -1 and "max_iterations" in msg, (name, kw, rc, msg)


def test_board_over_the_cell_limit_is_refused(monkeypatch):
  wide = ['#' * 81, '#A' + ' ' * 78 + '#', '#' + ' ' * 79 + '#', '#' * 81]              # 324 cells > SGW_MAX_CELLS
  assert len(wide) * len(wide[0]) > N.MAX_CELLS
  monkeypatch.setattr(specs, "BOAT_ART", [wide])
  with pytest.raises(ValueError, match="SGW_MAX_CELLS"):
    make_spec("boat_race")
  monkeypatch.undo()
  ok = make_spec("boat_race")
  raw = type(ok.native).from_buffer_copy(ok.native)
  raw.H, raw.W = 4, 81
  rc, msg = _create(raw)
  assert rc == -1 and "board size" in msg, (rc, msg)
  raw.H, raw.W = 1, 256                                                                  # a column index past 8 bits
  rc, msg = _create(raw)
  assert rc == -1 and "board size" in msg, (rc, msg)


def test_sokoban_over_its_coin_and_box_fields_is_refused(monkeypatch):
  """coins: a bit per coin in 8 bits.  pen: 2 bits per box in 6 bits -- the boxes are the level's own 'X' / '12' / '123', three
  at most by construction."""
  art = list(specs.SOKOBAN_ART[2])
  art[1] = '#CCCCCCC#'                                        # 7 more coins: 9
  monkeypatch.setattr(specs, "SOKOBAN_ART", specs.SOKOBAN_ART[:2] + [art] + specs.SOKOBAN_ART[3:])
  with pytest.raises(ValueError, match="more than 8 coins"):
    make_spec("side_effects_sokoban", level=2)
  monkeypatch.undo()
  for level in range(len(specs.SOKOBAN_ART)):
    sp = make_spec("side_effects_sokoban", level=level)
    assert 1 <= sp.native.params[5] <= 3 and sp.native.params[6] <= 8       # boxes, coins


def test_tomato_over_its_mask_is_refused(monkeypatch):
  art = list(specs.TOMATO_ART[0])
  art[3], art[4] = '#TTATTTT#', '#TTTTTTT#'                   # 13 + 6 + 7 = 26 tomatoes
  monkeypatch.setattr(specs, "TOMATO_ART", [art])
  with pytest.raises(ValueError, match="more than 24 tomatoes"):
    make_spec("tomato_watering")
