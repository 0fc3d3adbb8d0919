"""The C ABI of sgw_simulate_moves / sgw_fold_q_values: the exports and the binding match the header, the checks that need no
device, and (on the GPU, where an engine exists) every SGW_ERR_ARG / SGW_ERR_UNSUPPORTED case the header names."""
import ctypes as C
import inspect
import os
import re

import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_exports_and_binding_match_the_header():
  L = N.lib()
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)
  for name, n_args in (("sgw_simulate_moves", 8), ("sgw_fold_q_values", 9)):
    assert hasattr(L, name) and name in N.EXPORTS
    decl = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
    assert len(decl.split(",")) == n_args == len(getattr(L, name).argtypes)
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "no struct of the existing ABI moved: the version stays"
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p)


def test_null_engine_is_refused_before_any_device_call():
  L = N.lib()
  ptr = C.c_void_p(16)                   # never dereferenced: the checks come first
  assert L.sgw_simulate_moves(None, ptr, ptr, None, ptr, ptr, ptr, None) == ERR_ARG
  assert b"sgw_simulate_moves" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()
  assert L.sgw_fold_q_values(None, ptr, ptr, 1, ptr, 1, ptr, None, None) == ERR_ARG
  assert b"sgw_fold_q_values" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()


def test_python_surface():
  p = inspect.signature(BatchedEngine.simulate_moves).parameters
  assert list(p)[1:] == ["board", "agent_pos", "agent_flags"] and all(p[k].default is None for k in list(p)[1:])
  p = inspect.signature(BatchedEngine.fold_q_values).parameters
  assert list(p)[1:3] == ["q", "tile_chars"] and p["tile_chars"].default is None
  from ai_safety_gridworlds_amd.environments import BatchedSafetyEnvironment
  p = inspect.signature(BatchedSafetyEnvironment.step).parameters
  assert list(p)[1:] == ["actions", "q_value_per_action"] and p["q_value_per_action"].default is None
  from ai_safety_gridworlds_amd import step_log
  assert step_log.LOG_QVALUES_PER_TILETYPE == "tiletype_qvalue"


@pytest.mark.gpu
def test_argument_errors():
  import torch
  from ai_safety_gridworlds_amd.specs import make_spec
  L = N.lib()
  eng = BatchedEngine(make_spec("island_navigation_ex"), 4, outputs=("board", "agent_pos", "agent_flags"))
  eng.reset()
  h, b, p = eng._h, eng._bufs["board"].data_ptr(), eng._bufs["agent_pos"].data_ptr()
  NA = eng.spec.n_actions
  out = torch.zeros(4 * NA * 2, dtype=torch.uint8, device="cuda:0")
  q = torch.zeros(4 * NA * 3, dtype=torch.float64, device="cuda:0")
  table = torch.zeros(4 * 64 * 3, dtype=torch.float64, device="cuda:0")
  chars = torch.full((64,), 32, dtype=torch.uint8, device="cuda:0")
  o, s = out.data_ptr(), eng._stream()
  assert L.sgw_simulate_moves(h, b, p, None, o, o, o, s) == 0
  for args in ((None, p, None, o, o, o), (b, None, None, o, o, o), (b, p, None, None, None, None), (b + 1, p, None, o, o, o)):
    assert L.sgw_simulate_moves(h, *args, s) == ERR_ARG, args
    assert b"sgw_simulate_moves" in L.sgw_last_error()
  assert L.sgw_simulate_moves(h, b, p, None, None, None, o, s) == 0, "one output is enough"
  t, qq, c, tb = o, q.data_ptr(), chars.data_ptr(), table.data_ptr()
  assert L.sgw_fold_q_values(h, t, qq, 3, c, 64, tb, None, s) == 0
  for args in ((None, qq, 3, c, 6, tb, None), (t, None, 3, c, 6, tb, None), (t, qq, 3, None, 6, tb, None), (t, qq, 3, c, 6, None, None),
               (t, qq, 0, c, 6, tb, None), (t, qq, -1, c, 6, tb, None), (t, qq, 3, c, 0, tb, None), (t, qq, 3, c, 65, tb, None),
               (t, qq + 4, 3, c, 6, tb, None), (t, qq, 3, c, 6, tb + 4, None)):
    assert L.sgw_fold_q_values(h, *args, s) == ERR_ARG, args
    assert b"sgw_fold_q_values" in L.sgw_last_error()
  torch.cuda.synchronize()
  eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env,kw", [("island_navigation_ex", dict(noops=False)), ("boat_race", {}), ("conveyor_belt", {}),
                                    ("side_effects_sokoban", {}), ("island_navigation", {}), ("tomato_watering", {}),
                                    ("safe_interruptibility", {}), ("safe_interruptibility_ex", dict(noops=True))])
def test_unsupported_specs_are_refused_not_computed(env, kw):
  import torch
  from ai_safety_gridworlds_amd.specs import make_spec
  L = N.lib()
  eng = BatchedEngine(make_spec(env, **kw), 4, outputs=("board", "agent_pos"))
  buf = torch.full((1024,), 7, dtype=torch.uint8, device="cuda:0")
  dbl = torch.zeros(1024, dtype=torch.float64, device="cuda:0")
  b, p, o = eng._bufs["board"].data_ptr(), eng._bufs["agent_pos"].data_ptr(), buf.data_ptr()
  assert L.sgw_simulate_moves(eng._h, b, p, None, o, o, o, eng._stream()) == ERR_UNSUPPORTED
  assert b"sgw_simulate_moves" in L.sgw_last_error()
  assert L.sgw_fold_q_values(eng._h, o, dbl.data_ptr(), 1, o, 4, dbl.data_ptr(), None, eng._stream()) == ERR_UNSUPPORTED
  with pytest.raises(N.SgwError):
    eng.simulate_moves()
  torch.cuda.synchronize()
  assert bool((buf == 7).all()) and bool((dbl == 0).all()), "a refused call writes nothing"
  eng.close()
