"""CPU tier of the output-subset tests (tests/output_subsets.py, tests/test_output_subsets_gpu.py): the LDS plan of every row's
geometry is checked for every value of the output mask by a stand-alone host program (tests/host_shim/lds_plan_check.cpp, built
with UndefinedBehaviorSanitizer + AddressSanitizer and run as a subprocess), and the subset lists the GPU tier runs hold what
they claim to hold."""
import os
import subprocess

import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import DEFAULT_OUTPUTS
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import output_subsets as OS

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "lds_plan_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
  if cc == CLANG:
    flags.append("-ftrivial-auto-var-init=pattern")
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "lds_plan_check.cpp"), "-o", out])
  return out


def run_checker(exe, geometries):
  text = "".join(" ".join(str(int(v)) for v in g) + "\n" for g in geometries)
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  return subprocess.run([exe], input=text, capture_output=True, text=True, env=env)


def test_lds_plan_of_every_row_geometry_and_mask(exe):
  geos = []
  for r in LP.ROWS:
    for g in OS.plan_geometries(r, make_spec(r["name"], **r["kw"])):
      if g not in geos:
        geos.append(g)
  assert any(g[6] > 0 for g in geos) and any(g[5] > 0 and g[7] < 64 for g in geos) and any(g[4] > 1 for g in geos)
  p = run_checker(exe, geos)
  assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
  assert p.stdout.startswith("ok: %d geometries, %d plans" % (len(geos), len(geos) << 15)), p.stdout


def test_plan_checker_sees_a_region_that_is_too_small(exe):
  """The checker's extents are its own: parked vectors larger than the rows they alias (cs > A * K) must be reported, or the
  checker checks nothing."""
  p = run_checker(exe, [(77, 2, 6, 12, 2, 50, 14, 64)])       # island_navigation_ex_ma's geometry with two parked rows too many
  assert p.returncode == 1 and "cstash" in p.stdout, p.stdout + p.stderr


def test_view_chunk_restates_the_library():
  assert [OS.view_chunk(50, w) for w in (8, 16, 32, 64)] == [8, 16, 32, 64]
  assert [OS.view_chunk(441, w) for w in (8, 16, 32, 64)] == [16, 16, 32, 64]      # an odd row: a multiple of 16 envs
  src = open(os.path.join(os.path.dirname(HERE), "ai_safety_gridworlds_amd", "csrc", "sgw_common.hpp")).read()
  assert "while (g < WAVE && (g < want || ((g * vb) & 15) != 0)) g <<= 1;" in src, "lds_view_chunk changed: restate it in view_chunk"


# entries per row: singles + 2 state-only + leave-one-out + 3 further cstash shapes + ("reward",) with accumulate off +
# DEFAULT_OUTPUTS + 8 random (+ 4 window shapes on the window rows, + BENCH_OUTPUTS on island_navigation_ex); a lower bound, so
# an edit cannot shrink the list
MIN_ENTRIES = {False: 15 + 2 + 6 + 3 + 1 + 1 + 8, True: 19 + 2 + 7 + 3 + 1 + 4 + 1 + 8}


@pytest.mark.parametrize("row_id", [r["id"] for r in LP.ROWS])
def test_subset_lists_cover_what_they_claim(row_id):
  row = LP.BY_ID[row_id]
  spec = make_spec(row["name"], **row["kw"])
  full = OS.full_outputs(row, spec)
  window = OS.is_window_row(row)
  assert set(row["outs"]) <= set(full) and "done" in full and len(set(full)) == len(full)
  assert window == (spec.family in (N.FIREMAKER_EX_MA, N.ISLAND_NAVIGATION_EX_MA, N.AINTELOPE_SAVANNA))
  assert all((f in full) == window for f in ("views", "obs_views", "obs_dir", "act_dir"))
  lst = OS.subsets(row, spec)
  assert lst == OS.subsets(row, spec), "the list must be deterministic"
  assert len(set(lst)) == len(lst), "duplicate entries"
  assert all(isinstance(a, bool) and set(o) <= set(N.OUT_FIELDS) and set(o) <= set(full) and len(set(o)) == len(o) for o, a in lst)
  for f in full:
    assert ((f,), True) in lst, "%s alone is missing" % f
  assert ((), True) in lst and ((), False) in lst
  as_sets = [(frozenset(o), a) for o, a in lst]
  for f in OS.LEAVE_ONE_OUT:
    if f in full:
      assert (frozenset(full) - {f}, True) in as_sets, "leave-one-out of %s is missing" % f
  for o, a in OS.CSTASH_SHAPES:
    assert (frozenset(o), a) in as_sets, "cstash shape %s / accumulate %s is missing" % (o, a)
  for o, a in OS.MORE_SHAPES:
    assert (frozenset(o), a) in as_sets
  assert {a for _, a in lst} == {True, False}
  assert (frozenset(DEFAULT_OUTPUTS), True) in as_sets
  if row["name"] == "island_navigation_ex":
    assert (frozenset(OS.BENCH_OUTPUTS), True) in as_sets
  if window:
    assert any("views" in o and "board" not in o for o, _ in lst)
    for o in OS.WINDOW_SHAPES:
      assert (frozenset(o), True) in as_sets
  assert len(lst) >= MIN_ENTRIES[window] + (1 if row["name"] == "island_navigation_ex" else 0) + (1 if "safety2" in full else 0), len(lst)
  for rid, path, o, a in OS.REGRESSIONS:
    if rid == row_id:
      assert (frozenset(o), a) in [(frozenset(x), y) for x, y in OS.subsets(row, spec, path)]


def test_bench_outputs_are_the_benchmarks():
  src = open(os.path.join(os.path.dirname(HERE), "bench.py")).read()
  assert "outputs=(%s))" % ", ".join('"%s"' % f for f in OS.BENCH_OUTPUTS) in src, "bench.py's headline output set changed"


def test_expected_derives_the_fields_the_record_does_not_hold():
  import numpy as np
  row = LP.BY_ID["island_ex_ma"]
  spec = make_spec(row["name"], **row["kw"])
  rs = np.random.default_rng(5)
  ref = dict(step_type=rs.integers(0, 4, (3, 5, 2)).astype(np.uint8), agent_flags=rs.integers(0, 256, (3, 5, 2)).astype(np.uint8),
             views=rs.integers(0, 256, (3, 5, 50)).astype(np.uint8), reward=rs.random((3, 5, 2, 6)))
  c = dict(ref=ref, spec=spec)
  assert OS.expected(c, "reward") is ref["reward"]
  assert np.array_equal(OS.expected(c, "done"), ref["step_type"] >= 2) and OS.expected(c, "done").dtype == np.uint8
  assert np.array_equal(OS.expected(c, "obs_dir"), (ref["agent_flags"] // 8) % 4)
  assert np.array_equal(OS.expected(c, "act_dir"), (ref["agent_flags"] // 2) % 4)
  ov = OS.expected(c, "obs_views")
  vm = np.ctypeslib.as_array(spec.native.value_map)
  assert ov.dtype == np.float32 and ov.shape == ref["views"].shape and ov[1, 2, 3] == np.float32(vm[ref["views"][1, 2, 3] % 128])
  a = np.zeros((4, 6, 2)); b = a.copy(); a[0, 0, 0] = b[0, 0, 0] = np.nan
  assert OS.first_difference(a, b) is None
  b[2, 1, 1] = 1; b[3, 0, 0] = 1
  assert OS.first_difference(a, b) == (1, 2)
