"""CPU tier of the table policy's C ABI: the struct mirror, the entry points' argument checks that need no device, the ABI
version where it was, and TablePolicy's epsilon -> explore_below."""
import ctypes as C
import inspect
import os
import re

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy, explore_below_of

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_mirror_and_symbols():
  L = N.lib()
  assert L.sgw_sizeof_policy() == C.sizeof(N.Policy) == 72
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)
  fields = re.search(r"typedef struct sgw_policy \{(.*?)\} sgw_policy;", header, flags=re.S).group(1)
  names = [n for decl in fields.split(";") for n in re.findall(r"\b(\w+)\s*(?:,|$)", decl.strip())]
  assert names == [f[0] for f in N.Policy._fields_]
  for name in ("sgw_sizeof_policy", "sgw_policy_act", "sgw_policy_step_n"):
    assert hasattr(L, name) and name in N.EXPORTS
  assert len(L.sgw_policy_act.argtypes) == 6 and len(L.sgw_policy_step_n.argtypes) == 9
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8 and "#define SGW_ABI_VERSION 8" in header
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p), "no struct of the existing ABI moved"
  assert (N.POLICY_BOARD, N.POLICY_VIEWS) == (0, 1) and "SGW_POLICY_BOARD = 0, SGW_POLICY_VIEWS = 1" in header


def test_null_engine_is_refused_before_any_device_call():
  L = N.lib()
  p = N.Policy()
  ptr = C.c_void_p(16)                   # never dereferenced: the checks come first
  assert L.sgw_policy_act(None, C.byref(p), ptr, 0, ptr, None) == -1
  assert b"sgw_policy_act" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()
  assert L.sgw_policy_step_n(None, C.byref(p), ptr, 8, 0, C.byref(N.Out()), ptr, 0, None) == -1
  assert b"sgw_policy_step_n" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()


def test_epsilon_maps_to_the_draw_threshold():
  assert explore_below_of(0.0) == 0                     # never
  assert explore_below_of(0.25) == 1 << 30
  assert explore_below_of(1.0) == 1 << 32               # always: every 32-bit draw is below it
  assert explore_below_of(1.0 - 2.0 ** -40) == (1 << 32) - 1


def test_python_surface_and_the_reserved_tag():
  assert philox.TAG_POLICY == 2 and len({philox.TAG_ACTION, philox.TAG_EPISODE, philox.TAG_POLICY}) == 3
  p = inspect.signature(TablePolicy.__init__).parameters
  assert list(p)[1:] == ["engine", "source", "chars", "n_policies", "seed", "epsilon"]
  assert (p["source"].default, p["chars"].default, p["n_policies"].default, p["seed"].default, p["epsilon"].default) == ("board", None, 1, 0, 0.0)
  p = inspect.signature(BatchedEngine.act).parameters
  assert list(p)[1:] == ["policy", "obs", "out", "t"] and p["t"].default == 0
  p = inspect.signature(BatchedEngine.policy_step_n).parameters
  assert list(p)[1:] == ["policy", "T", "write_every", "accumulate"] and p["write_every"].default is False
  assert list(inspect.signature(TablePolicy.from_cell_actions).parameters) == ["engine", "table", "agent_chr"]
