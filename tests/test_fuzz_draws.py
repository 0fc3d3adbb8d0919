"""What the seeded fuzz tests of tests/test_fuzz_gpu.py select, checked without a GPU (draw_only=True stops a case once its
configuration is accepted).  The numeric draws of tests/fuzz_cases.py were added behind numeric=False: the four older tests must
go on selecting the configurations they always did.  The digests below were computed from the kwargs lists of the code before
that argument existed."""
import hashlib

import numpy as np
import pytest

from tests import flag_fixtures as FF
from tests import fuzz_cases as F
from tests import test_fuzz_gpu as TF


def _select(case, n_cases, seed):
  """The kwargs of the configurations _run() of tests/test_fuzz_gpu.py runs for this case and seed."""
  rnd = np.random.default_rng(seed)
  picked, tries = [], 0
  while len(picked) < n_cases and tries < 4 * n_cases:
    tries += 1
    res = case(rnd)
    if res is not None:
      assert res[2] is None
      picked.append(res[1])
  assert len(picked) == n_cases
  return picked


def _digest(picked):
  return hashlib.sha256(repr([sorted(kw.items()) for kw in picked]).encode()).hexdigest()


@pytest.mark.parametrize("family,digest", [
    ("island", "2cccc59b70ed2783bd591c2b39671cf150f66e2c1c23b56849f3b08fe3027d93"),
    ("ima", "2b4be722f58e9bbcf0214f8f715a707f974da1fbd5c5ae024914cee1e489c441"),
    ("sav", "c2c345be1220851a3cfb1b33f1bca9207d5691e7429b7b01f302a9e68955797b"),
    ("firemaker", "d2f8d75a5f17220d4fdcf411520aa03234a8cacb8cbd8fdcbe2260777fe14a4b"),
])
def test_seeded_tests_select_the_configurations_they_always_did(family, digest):
  case, n_cases, seed = TF.CASES[family]
  assert _digest(_select(lambda r: case(r, draw_only=True), n_cases, seed)) == digest


@pytest.mark.parametrize("family", sorted(TF.NUMERIC_CASES))
def test_numeric_draws_move_flags_and_windows(family):
  """The 24 numeric configurations of a family together move most of what the flag fixtures pin, and some windows are lopsided."""
  case, n_cases, seed = TF.NUMERIC_CASES[family]
  picked = _select(lambda r: case(r, draw_only=True), n_cases, seed)
  key = {"island": "island_ex", "ima": "ima", "sav": "sav", "firemaker": "ma"}[family]
  flags = set(FF.moved_flags(key))
  moved = {k for kw in picked for k in kw if k in flags}
  assert len(moved) >= 0.7 * len(flags - set(FF.DEAD[key])), sorted(flags - moved)
  if family != "island":
    radii = [v for kw in picked for k, v in kw.items() if k.endswith("observation_radius") and v != [2, 2, 2, 2]]
    assert len(radii) >= 2 and all(r[0] != r[1] and r[2] != r[3] for r in radii)
