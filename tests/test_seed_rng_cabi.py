"""CPU tier of device-side seeding (sgw_seed_rng / sgw_pcg64_from_seeds): declared in include/sgw.h, exported by libsgw.so,
listed in the binding with argument types, the ABI version where it was, the argument checks that need no device, and the
Python surface (BatchedEngine.seed_rng, GridworldZooVectorEnv.reset(seed=, options=)) as signatures."""
import ctypes as C
import inspect
import os
import re

import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sgw_seed_rng", "sgw_pcg64_from_seeds")


def test_symbols_are_declared_exported_and_listed():
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)
  L = N.lib()
  for s in SYMBOLS:
    assert re.search(r"\bint\s+%s\s*\(" % s, header), s
    assert hasattr(L, s), s
    assert s in N.EXPORTS, s
    assert getattr(L, s).argtypes, s
  assert re.search(r"#define\s+SGW_SEED_LOW32\s+1\b", header) and N.SEED_LOW32 == 1
  assert len(L.sgw_seed_rng.argtypes) == 7 and len(L.sgw_pcg64_from_seeds.argtypes) == 9
  assert re.search(r"\bint\s+sgw_set_rng_state\s*\(\s*sgw_engine\s*\*\s*e\s*,\s*const\s+uint64_t\s*\*\s*pcg_state_dev\s*\)", header), "stays as it is"
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "entry points only: the ABI version does not move"
  assert "#define SGW_ABI_VERSION 8" in header


def test_bad_arguments_are_refused_before_any_device_call():
  L = N.lib()
  fake = C.c_void_p(8)                  # never dereferenced: the checks come first
  assert L.sgw_seed_rng(None, None, 0, None, None, 0, None) == -1
  assert b"sgw_seed_rng" in L.sgw_last_error()
  assert L.sgw_seed_rng(None, fake, 5, fake, fake, 1, None) == -1
  assert L.sgw_pcg64_from_seeds(None, 0, 0, None, 0, 4, None, 0, None) == -1, "null output"
  assert b"sgw_pcg64_from_seeds" in L.sgw_last_error()
  assert L.sgw_pcg64_from_seeds(None, 0, 0, None, 0, -1, fake, 0, None) == -1, "n < 0"
  assert L.sgw_pcg64_from_seeds(None, 0, 0, None, 2, 4, fake, 0, None) == -1, "unknown flag bits"
  assert L.sgw_pcg64_from_seeds(None, 0, 0, None, 1, 0, fake, 0, None) == 0, "n == 0: nothing to do, nothing launched"


def test_python_surface():
  p = inspect.signature(BatchedEngine.seed_rng).parameters
  assert list(p)[1:] == ["seeds", "base", "layout_seeds", "mask", "low32"]
  assert p["seeds"].default is None and p["base"].default == 0 and p["layout_seeds"].default is None and p["low32"].default is False
  assert "set_rng_seeds" in vars(BatchedEngine), "the host-side path stays"
  p = inspect.signature(GridworldZooVectorEnv.reset).parameters
  assert list(p)[1:] == ["mask", "seed", "options"] and all(p[k].default is None for k in ("mask", "seed", "options"))


def _shell(seed_base, env_id_base, n):
  env = object.__new__(GridworldZooVectorEnv)
  env._has_rng, env._seed_base, env._env_id_base, env.num_envs = True, seed_base, env_id_base, n
  return env


def test_layout_seed_overflow_is_raised_before_the_engine_is_touched():
  """to_bytes(4) of the reference (safety_game_moma.py:851) raises OverflowError for an original seed or a layout seed that
  does not fit 32 bits; the shell has no engine, so reaching it would be an AttributeError."""
  with pytest.raises(OverflowError):
    _shell(2000, 0, 3)._reseed(None, None, 1 << 32)
  with pytest.raises(OverflowError):
    _shell(2000, 0, 3)._reseed(None, None, -1)
  with pytest.raises(OverflowError):
    _shell((1 << 32) - 2, 0, 3)._reseed(None, None, 2)          # env 2's original seed is 2^32
  with pytest.raises(OverflowError):
    _shell(0, (1 << 32) - 1, 2)._reseed(None, None, 2)          # the global id counts
  env = _shell(0, 0, 2)
  env._has_rng = False
  with pytest.raises(N.SgwError):
    env._reseed(None, 5, None)
