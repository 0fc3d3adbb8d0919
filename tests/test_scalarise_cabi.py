"""CPU tier of sgw_scalarise: declared in include/sgw.h, exported by libsgw.so, listed in the binding with argument types, the
ABI version and struct sizes where they were, the argument checks that need no device, and the Python surface
(BatchedEngine.scalarise, the facades' `scalarise` argument) as signatures."""
import ctypes as C
import inspect
import os
import re

import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.environments import BatchedSafetyEnvironment
from ai_safety_gridworlds_amd.specs import make_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_listed():
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)
  L = N.lib()
  m = re.search(r"\bint\s+sgw_scalarise\s*\(([^)]*)\)", header)
  assert m, "include/sgw.h declares sgw_scalarise"
  params = [p.strip() for p in m.group(1).split(",")]
  assert len(params) == 10 and params[0].startswith("sgw_engine*") and params[4] == "int T" and params[-1] == "void* stream"
  assert hasattr(L, "sgw_scalarise") and "sgw_scalarise" in N.EXPORTS
  assert len(L.sgw_scalarise.argtypes) == 10
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "an entry point only: the ABI version does not move"
  assert "#define SGW_ABI_VERSION 8" in header
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p) == C.sizeof(N.Out), "no struct change: 20 outputs"
  assert L.sgw_sizeof_extras() == C.sizeof(N.Extras)


def test_null_engine_is_refused_before_any_device_call():
  L = N.lib()
  out = C.c_void_p(16)                   # never dereferenced: the checks come first
  assert L.sgw_scalarise(None, out, out, out, 1, None, out, out, out, None) == -1
  assert b"sgw_scalarise" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()


def test_the_kernel_is_built_without_scratch():
  """The unrolled sums index nothing at run time: the installed build's assembly reports no private segment for k_scalarise."""
  from ai_safety_gridworlds_amd import build
  N.lib()
  if os.path.exists(build.ASM):           # (a prebuilt library that travelled without its assembly: the flags below still hold)
    m = re.search(r"\.set (\S*k_scalarise\S*)\.private_seg_size, (\d+)", open(build.ASM).read())
    assert m, "k_scalarise is in the build"
    assert int(m.group(2)) == 0
  fast = [f for f in build.FLAGS if "fast-math" in f or f.startswith("-Ofast") or "reciprocal" in f or "unsafe" in f]
  assert fast in ([], ["-fno-fast-math"]), "no fast-math flag on the build line: the order of the additions is the contract"


def test_scalar_reward_envs_take_no_scalarise():
  with pytest.raises(TypeError, match="scalarise"):
    make_spec("boat_race", scalarise=True)
  with pytest.raises(TypeError, match="scalarise"):      # the flag never reaches make_spec: the MO specs do not know it either
    make_spec("island_navigation_ex", scalarise=True)
  for name in ("boat_race", "safe_interruptibility", "island_navigation", "side_effects_sokoban", "conveyor_belt", "tomato_watering",
               "friend_foe", "whisky_gold", "rocks_diamonds"):
    with pytest.raises(TypeError, match="scalarise"):    # refused before a device is asked for
      BatchedSafetyEnvironment(name, num_envs=1, device="cuda:0", scalarise=True)


def test_python_surface():
  p = inspect.signature(BatchedEngine.scalarise).parameters
  assert list(p)[1:] == ["T", "buffers"] and p["T"].default == 1 and p["buffers"].default is None
  p = inspect.signature(BatchedSafetyEnvironment.__init__).parameters
  assert p["scalarise"].default is False
