"""CPU tier of sgw_copy_envs / sgw_out_row_bytes: declared in include/sgw.h, exported by libsgw.so, listed in the binding with
argument types, the ABI version where it was, the argument checks that need no device, and the Python surface
(BatchedEngine.copy_envs / fork / lookahead) as signatures."""
import ctypes as C
import inspect
import os
import re

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_listed():
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)
  L = N.lib()
  assert re.search(r"\bint\s+sgw_copy_envs\s*\(", header) and re.search(r"\bint64_t\s+sgw_out_row_bytes\s*\(", header)
  for s in ("sgw_copy_envs", "sgw_out_row_bytes"):
    assert hasattr(L, s), s
    assert s in N.EXPORTS, s
    assert getattr(L, s).argtypes, s
  assert len(L.sgw_copy_envs.argtypes) == 8 and len(L.sgw_out_row_bytes.argtypes) == 2
  assert L.sgw_out_row_bytes.restype is C.c_int64
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "entry points only: the ABI version does not move"
  assert "#define SGW_ABI_VERSION 8" in header
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p) == C.sizeof(N.Out), "no struct change: 20 outputs"


def test_bad_arguments_are_refused_before_any_device_call():
  L = N.lib()
  fake = C.c_void_p(8)                  # never dereferenced: the checks come first
  assert L.sgw_copy_envs(None, None, None, None, 0, None, None, None) == -1
  assert b"sgw_copy_envs" in L.sgw_last_error()
  assert L.sgw_copy_envs(None, fake, None, None, 4, None, None, None) == -1, "null destination"
  assert L.sgw_copy_envs(fake, None, None, None, 4, None, None, None) == -1, "null source"
  assert b"null engine" in L.sgw_last_error()
  assert L.sgw_copy_envs(fake, fake, None, None, -1, None, None, None) == -1, "n < 0"
  assert b"n < 0" in L.sgw_last_error()
  assert L.sgw_out_row_bytes(None, 0) < 0
  assert b"sgw_out_row_bytes" in L.sgw_last_error()


def test_python_surface():
  p = inspect.signature(BatchedEngine.copy_envs).parameters
  assert list(p)[1:] == ["src", "src_idx", "dst_idx", "outputs"]
  assert p["src_idx"].default is None and p["dst_idx"].default is None and p["outputs"].default is True
  p = inspect.signature(BatchedEngine.fork).parameters
  assert list(p)[1:] == ["n_envs", "env_id_base", "outputs"] and all(p[k].default is None for k in list(p)[1:])
  assert list(inspect.signature(BatchedEngine.lookahead).parameters)[1:] == ["actions"]
