"""GPU tier: a bounded, fixed-seed slice of the randomised configuration sweep (tests/fuzz_cases.py; the open-ended tool is
tools/diag/fuzz_parity.py): HIP engine vs the C oracle on random levels / flags / tile amounts / map sizes / direction modes /
single-agent rounds / explicit resets of island_navigation_ex, island_navigation_ex_ma, aintelope_savanna and firemaker_ex_ma --
every output of every step, the metrics and the numpy generator position.  Every kernel edit is validated by this in the GPU
tier, not only by a tool somebody has to remember to run.  The `_numeric` tests also draw the numeric rule parameters, the reward
values and lopsided observation windows (tests/fuzz_cases.py NUMERIC_*); tests/test_fuzz_draws.py checks on the CPU what every
seed here selects."""
import numpy as np
import pytest

from tests import fuzz_cases as F

pytestmark = pytest.mark.gpu


def _run(case, n_cases, seed=0):
  rnd = np.random.default_rng(seed)
  ran, tries = 0, 0
  while ran < n_cases and tries < 4 * n_cases:
    tries += 1
    res = case(rnd)
    if res is None:                      # a configuration the reference (and make_spec) refuses
      continue
    assert res[2] is True, "mismatch: %s %r -> %r" % (res[0], res[1], res[2])
    ran += 1
  assert ran == n_cases


def _island(r, **kw): return F.island_case(r, E=512, T=120, nthreads=8, **kw)
def _ima(r, **kw): return F.ma_case(r, "ima", E=320, T=100, nthreads=8, **kw)
def _sav(r, **kw): return F.ma_case(r, "sav", E=256, T=100, nthreads=8, **kw)
def _firemaker(r, **kw): return F.firemaker_case(r, E=192, T=110, nthreads=8, **kw)


def _numeric(case):
  return lambda r, **kw: case(r, numeric=True, **kw)


# family -> (case, configurations, seed)
CASES = {"island": (_island, 150, 20261), "ima": (_ima, 150, 20262), "sav": (_sav, 150, 20263), "firemaker": (_firemaker, 60, 20264)}
NUMERIC_CASES = {"island": (_numeric(_island), 24, 20271), "ima": (_numeric(_ima), 24, 20272), "sav": (_numeric(_sav), 24, 20273),
                 "firemaker": (_numeric(_firemaker), 24, 20274)}


def test_fuzz_island_navigation_ex():
  _run(*CASES["island"])


def test_fuzz_island_navigation_ex_ma():
  _run(*CASES["ima"])


def test_fuzz_aintelope_savanna():
  _run(*CASES["sav"])


def test_fuzz_firemaker_ex_ma():
  _run(*CASES["firemaker"])


def test_fuzz_island_navigation_ex_numeric():
  _run(*NUMERIC_CASES["island"])


def test_fuzz_island_navigation_ex_ma_numeric():
  _run(*NUMERIC_CASES["ima"])


def test_fuzz_aintelope_savanna_numeric():
  _run(*NUMERIC_CASES["sav"])


def test_fuzz_firemaker_ex_ma_numeric():
  _run(*NUMERIC_CASES["firemaker"])
