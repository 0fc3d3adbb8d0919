"""CPU tier of the learning calls (sgw_policy_scores, sgw_policy_accumulate, sgw_policy_apply): declared in include/sgw.h, exported
by libsgw.so, listed in the binding with argument types, the ABI version and the structs where they were, the null-engine check that
needs no device, no scratch in the installed kernels, and the Python surface as signatures."""
import ctypes as C
import inspect
import os
import re

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sgw_policy_scores": 11, "sgw_policy_accumulate": 12, "sgw_policy_apply": 8}


def _header():
  return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)


def _params(header, name):
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
  assert m, "include/sgw.h declares %s" % name
  return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_symbols_are_declared_exported_and_listed():
  header, L = _header(), N.lib()
  assert _params(header, "sgw_policy_scores") == [
      "sgw_engine* e", "const sgw_policy* p", "const uint8_t* obs0_dev", "const uint8_t* obs_dev", "int64_t obs_rows", "int T",
      "const int8_t* actions_dev", "float* scores_dev", "double* vmax_dev", "double* chosen_dev", "void* stream"]
  assert _params(header, "sgw_policy_accumulate") == [
      "sgw_engine* e", "const sgw_policy* p", "const uint8_t* obs0_dev", "const uint8_t* obs_dev", "int64_t obs_rows", "int T",
      "const int8_t* actions_dev", "const double* coef_dev", "int frac_bits", "int64_t* acc_weights_dev", "int64_t* acc_bias_dev",
      "void* stream"]
  assert _params(header, "sgw_policy_apply") == [
      "sgw_engine* e", "const sgw_policy* p", "double lr", "int frac_bits", "int64_t* acc_weights_dev", "int64_t* acc_bias_dev",
      "int flags", "void* stream"]
  assert "#define SGW_APPLY_CLEAR 1" in header and N.APPLY_CLEAR == 1
  for name, n_args in SYMBOLS.items():
    assert hasattr(L, name) and name in N.EXPORTS
    assert len(getattr(L, name).argtypes) == n_args
  assert L.sgw_policy_apply.argtypes[2] is C.c_double and L.sgw_policy_scores.argtypes[4] is C.c_int64


def test_the_existing_abi_did_not_move():
  header, L = _header(), N.lib()
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "entry points only: the ABI version does not move"
  assert "#define SGW_ABI_VERSION 8" in header
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p) == C.sizeof(N.Out), "no struct change: 20 outputs"
  assert L.sgw_sizeof_policy() == C.sizeof(N.Policy) == 4 * 4 + 4 * 8 + 2 * 8 + 8, "sgw_policy did not move"
  body = re.search(r"typedef struct sgw_policy \{(.*?)\} sgw_policy;", header, flags=re.S).group(1)
  declared = []
  for stmt in body.split(";"):
    stmt = stmt.strip()
    if stmt:
      declared += [w.strip().split()[-1].lstrip("*") for w in stmt.split(",")]
  assert declared == [n for n, _ in N.Policy._fields_]


def test_null_engine_is_refused_before_any_device_call():
  L = N.lib()
  pol = N.Policy(source=0, n_policies=1, n_codes=2, cells=4, code_of=16, weights=16, step_dev=16)      # never dereferenced: the checks come first
  assert L.sgw_policy_scores(None, C.byref(pol), 16, None, 0, 0, None, 16, None, None, None) == -1
  assert b"sgw_policy_scores" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()
  assert L.sgw_policy_accumulate(None, C.byref(pol), 16, None, 0, 1, 16, 16, 24, 32, None, None) == -1
  assert b"sgw_policy_accumulate" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()
  assert L.sgw_policy_apply(None, C.byref(pol), 0.1, 24, 32, None, 0, None) == -1
  assert b"sgw_policy_apply" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()


def test_the_kernels_are_built_without_scratch():
  """The score registers are picked by selects, the slice tables by compares, the bins live in LDS: the installed build's assembly
  reports no private segment for the three kernels.  The contract's one-rounding-per-operation needs -ffp-contract=off."""
  from ai_safety_gridworlds_amd import build
  N.lib()
  if not os.path.exists(build.ASM):       # a library that travelled without its assembly: build() writes both (as test_isa_lint does)
    build.build(force=True)
  asm = open(build.ASM).read()
  for kernel in ("k_policy_scores", "k_policy_accumulate", "k_policy_apply"):
    m = re.search(r"\.set (\S*%s\S*)\.private_seg_size, (\d+)" % kernel, asm)
    assert m, "%s is in the build" % kernel
    assert int(m.group(2)) == 0, kernel
  assert "-ffp-contract=off" in build.FLAGS


def test_python_surface():
  p = inspect.signature(BatchedEngine.policy_scores).parameters
  assert list(p)[1:] == ["policy", "T", "obs0", "obs", "actions"]
  assert p["T"].default == 0 and all(p[k].default is None for k in ("obs0", "obs", "actions"))
  p = inspect.signature(BatchedEngine.policy_accumulate).parameters
  assert list(p)[1:] == ["policy", "coef", "T", "obs0", "obs", "actions", "frac_bits"]
  assert p["frac_bits"].default == 24 and p["obs"].default is None and p["actions"].default is None
  p = inspect.signature(BatchedEngine.policy_apply).parameters
  assert list(p)[1:] == ["policy", "lr", "clear"] and p["clear"].default is True
  p = inspect.signature(BatchedEngine.policy_step_n).parameters
  assert list(p)[1:] == ["policy", "T", "write_every", "accumulate"], "the closed-loop call's own signature did not move"
  p = inspect.signature(BatchedEngine.policy_rollout).parameters
  assert list(p)[1:] == ["policy", "T", "write_every", "accumulate"]
  assert p["write_every"].default is True and p["accumulate"].default is False
  p = inspect.signature(BatchedEngine.q_learn).parameters
  assert list(p)[1:] == ["policy", "T", "gamma", "lr", "bootstrap_truncated", "frac_bits"]
  assert p["bootstrap_truncated"].default is False and p["frac_bits"].default == 24
  assert isinstance(TablePolicy.acc_weights, property) and isinstance(TablePolicy.acc_bias, property)
