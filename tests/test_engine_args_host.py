"""engine._require, the one check of a tensor argument, on CPU tensors: what it accepts, what it returns and what it refuses."""
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import _require

CPU = torch.device("cpu")


def _check(t, dtype=torch.uint8, numel=12, **kw):
  return _require("some_call", "arg", t, CPU, dtype, numel, "[3, 4]", **kw)


def test_accepts_a_matching_tensor_and_returns_the_count_that_matched():
  t = torch.zeros((3, 4), dtype=torch.uint8)
  assert _check(t) == 12
  assert _check(t, numel=(6, 12)) == 12 and _check(t[:, :2].contiguous(), numel=(6, 12)) == 6
  assert _check(t, numel=None) is None                                       # any count
  assert _check(t.float(), dtype=(torch.float64, torch.float32)) == 12       # one of several dtypes
  assert _check(t.t(), contiguous=False) == 12
  assert _check(t, shape=(3, 4)) == 12 and _check(t, also=lambda x: x.dim() == 2) == 12


@pytest.mark.parametrize("why,make,kw", [
    ("not a tensor", lambda: [[0] * 4] * 3, {}),
    ("dtype", lambda: torch.zeros((3, 4), dtype=torch.int8), {}),
    ("count", lambda: torch.zeros((3, 5), dtype=torch.uint8), {}),
    ("count of a tuple", lambda: torch.zeros((3, 5), dtype=torch.uint8), {"numel": (6, 12)}),
    ("strides", lambda: torch.zeros((4, 3), dtype=torch.uint8).t(), {}),
    ("device", lambda: torch.zeros((3, 4), dtype=torch.uint8, device=torch.device("meta")), {}),
    ("shape", lambda: torch.zeros((4, 3), dtype=torch.uint8), {"shape": (3, 4)}),
    ("also", lambda: torch.zeros((3, 4), dtype=torch.uint8), {"also": lambda x: x.dim() == 3}),
])
def test_refuses(why, make, kw):
  t = make()
  if why == "strides":
    assert tuple(t.shape) == (3, 4) and not t.is_contiguous()
  with pytest.raises(N.SgwError) as info:
    _check(t, **kw)
  assert str(info.value) == "some_call: arg must be a contiguous uint8 [3, 4] tensor on cpu (there is no CPU path)"


def test_the_sentence_follows_the_arguments():
  with pytest.raises(N.SgwError) as info:
    _require("fold", "q", None, CPU, (torch.float64, torch.float32), None, contiguous=False)
  assert str(info.value) == "fold: q must be a float64 (or float32) tensor on cpu (there is no CPU path)"
