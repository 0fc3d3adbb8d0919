"""tests/grid_caps.py against the source: every named grid cap of csrc/sgw_api.hip has a row, every covered row's large shape walks
its stride loop at least three times with a ragged last trip inside the device-memory budget, the shapes the rest of the suite uses
make one trip (the gap the rows close -- and what fails here when a cap changes and a test is not resized), and a row that is not
covered shows by its own arithmetic that two trips do not fit."""
import pytest

from tests import grid_caps as GC

IDS = [r["id"] for r in GC.ROWS]
COVERED = [r["id"] for r in GC.ROWS if r["covered"]]


def test_every_named_cap_has_a_row_and_every_row_its_constants():
  consts = GC.constants()
  names = GC.cap_names()
  assert len(names) >= 10, "the naming pattern finds the caps: %s" % names
  used = {c for r in GC.ROWS for c in r["caps"]}
  for name in used | {"WAVE", "LEARN_THREADS", "LEARN_MAX_ROW_LDS", "LEARN_MAX_BIN_LDS", "LEARN_BLOCKS", "SGW_MAX_CELLS"}:
    assert name in consts, "%s was not found in the source" % name
  assert set(names) - used == set(), "caps without a row in tests/grid_caps.py: %s" % sorted(set(names) - used)
  assert len(set(IDS)) == len(IDS)
  with pytest.raises(AssertionError):
    GC.const("NO_SUCH_MAX_BLOCKS")


def test_the_caps_are_what_the_rows_were_sized_for():
  """A changed cap is fine; it has to come with resized rows.  (The values: 65 536 four times, 8 192 twice, 4 096 three times.)"""
  c = GC.constants()
  values = sorted(c[n] for n in GC.cap_names())
  assert values == sorted([65536] * 4 + [8192] * 2 + [4096] * 3 + [1024]), {n: c[n] for n in GC.cap_names()}
  assert c["AGENT_VIEWS_LDS_GROUP_ENVS"] == 4


@pytest.mark.parametrize("id", COVERED)
def test_large_shape_makes_three_trips_and_a_ragged_last_one(id):
  r = GC.BY_ID[id]
  t = r["fn"](**r["large"])
  assert t.max_trips >= 3, (id, t)
  assert t.min_trips < t.max_trips, (id, t, "the last trip is ragged")
  assert t.partial in (True, None), (id, t, "the last group, tile or wave is partial")
  assert t.min_trips >= 2, (id, t, "every strider comes back at least once")
  assert r["bytes"](r["large"]) <= GC.BUDGET, (id, r["bytes"](r["large"]))
  if r["path"]:
    assert r["path"](r["large"]) == r["kernel"], (id, r["path"](r["large"]))
  if r["per_env"]:                             # the per-env tests repeat B_ENVS envs: a stride must not map a unit of work onto its copy
    assert t.stride % (GC.B_ENVS * r["per_env"]) != 0, (id, t.stride)


@pytest.mark.parametrize("id", IDS)
def test_old_suite_shape_makes_one_trip(id):
  r = GC.BY_ID[id]
  t = r["fn"](**r["old"])
  assert t.max_trips == 1, (id, t)
  if r["path"]:
    assert r["path"](r["old"]) == r["kernel"], (id, r["path"](r["old"]))


def test_uncovered_rows_cannot_fit_two_trips():
  uncovered = [r for r in GC.ROWS if not r["covered"]]
  assert len(uncovered) <= 2
  assert [r["id"] for r in uncovered] == ["views_wave"]
  assert all(r["why"] for r in uncovered)
  n, total, nbytes = GC.views_wave_cheapest_two_trips()
  radii = [(0, 0, 0, total // 4 - 1)] * 3 + [(0, 0, 0, total - 3 * (total // 4) - 1)]       # rows of `total` bytes, whatever their windows
  assert GC.view_total(radii) == total
  assert GC.views_path(16, 20, radii) == "k_agent_views", "rows this long leave the LDS kernel"
  assert GC.views_wave(n, 16, 20, radii).max_trips == 2 and GC.views_wave(n - 1, 16, 20, radii).max_trips == 1
  assert nbytes > GC.BUDGET, (n, total, nbytes)              # 65 537 envs x 16 001 bytes: 1.05e9


def test_accumulate_rows_take_the_three_ways_through_the_tile_loop():
  x = {id: GC.BY_ID[id]["fn"](**GC.BY_ID[id]["large"]) for id in IDS if id.startswith("accumulate")}
  one, sliced, glob = x["accumulate_lds_one_slice"], x["accumulate_lds_sliced_window"], x["accumulate_global_atomics"]
  assert one.extra["in_lds"] and one.extra["slices"] == 1 and one.extra["E"] == 64 and one.extra["tiles"] == 2145 and one.workgroups == 1024
  assert sliced.extra["in_lds"] and sliced.extra["slices"] == 22 and sliced.extra["E"] == 16 and sliced.extra["tiles"] == 150
  assert sliced.extra["per_slice"] == 46 and sliced.extra["R"] < 33 * 33
  assert not glob.extra["in_lds"] and glob.extra["slices"] == 2 and glob.extra["per_slice"] == 512 and glob.extra["tiles"] == 1100
  old = GC.BY_ID["accumulate_lds_sliced_window"]
  assert old["fn"](**old["old"]).extra["tiles"] == 25
