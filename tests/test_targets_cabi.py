"""CPU tier of sgw_td_targets: declared in include/sgw.h, exported by libsgw.so, listed in the binding with argument types, the
struct mirror the size the library compiled, the ABI version and sgw_out where they were, the null-engine check that needs no
device, no scratch in the installed kernel, and the Python surface (BatchedEngine.td_targets) as a signature."""
import ctypes as C
import inspect
import os
import re

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
  return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sgw.h")).read(), flags=re.S)


def test_symbol_is_declared_exported_and_listed():
  header, L = _header(), N.lib()
  m = re.search(r"\bint\s+sgw_td_targets\s*\(([^)]*)\)", header)
  assert m, "include/sgw.h declares sgw_td_targets"
  params = [p.strip() for p in m.group(1).split(",")]
  assert params == ["sgw_engine* e", "const sgw_td* td", "void* stream"]
  assert re.search(r"\bint\s+sgw_sizeof_td\s*\(\s*void\s*\)", header)
  assert "#define SGW_TD_BOOTSTRAP_TRUNCATED 1" in header and N.TD_BOOTSTRAP_TRUNCATED == 1
  for name in ("sgw_td_targets", "sgw_sizeof_td"):
    assert hasattr(L, name) and name in N.EXPORTS
  assert len(L.sgw_td_targets.argtypes) == 3


def test_struct_mirror_matches_the_header():
  header, L = _header(), N.lib()
  assert L.sgw_sizeof_td() == C.sizeof(N.Td) == 8 * 8 + 2 * 8 + 4 * 4 + 8 + 8
  body = re.search(r"typedef struct sgw_td \{(.*?)\} sgw_td;", header, flags=re.S).group(1)
  declared = []
  for stmt in body.split(";"):
    stmt = stmt.strip()
    if stmt:
      declared += [w.strip().split()[-1].lstrip("*") for w in stmt.split(",")]
  mirror = [n.rstrip("_") if n == "lambda_" else n for n, _ in N.Td._fields_]
  assert declared == mirror, "the fields of struct sgw_td in their order"


def test_the_existing_abi_did_not_move():
  header, L = _header(), N.lib()
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "an entry point only: the ABI version does not move"
  assert "#define SGW_ABI_VERSION 8" in header
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p) == C.sizeof(N.Out), "no struct change: 20 outputs"


def test_null_engine_is_refused_before_any_device_call():
  L = N.lib()
  gamma = (C.c_double * 1)(0.99)
  td = N.Td(reward=16, step_type=16, ret=32, src_rows=64, dst_rows=64, T=1, C=1, gamma=gamma)      # never dereferenced: the checks come first
  assert L.sgw_td_targets(None, C.byref(td), None) == -1
  assert b"sgw_td_targets" in L.sgw_last_error() and b"null engine" in L.sgw_last_error()


def test_the_kernel_is_built_without_scratch():
  """Every row of a load group is a named register and gamma is picked by selects: the installed build's assembly reports no
  private segment for k_td_targets.  The contract's one-rounding-per-operation needs the build line's -ffp-contract=off and no
  fast-math flag."""
  from ai_safety_gridworlds_amd import build
  N.lib()
  if not os.path.exists(build.ASM):       # a library that travelled without its assembly: build() writes both (as test_isa_lint does)
    build.build(force=True)
  m = re.search(r"\.set (\S*k_td_targets\S*)\.private_seg_size, (\d+)", open(build.ASM).read())
  assert m, "k_td_targets is in the build"
  assert int(m.group(2)) == 0
  assert "-ffp-contract=off" in build.FLAGS
  fast = [f for f in build.FLAGS if "fast-math" in f or f.startswith("-Ofast") or "reciprocal" in f or "unsafe" in f]
  assert fast in ([], ["-fno-fast-math"])


def test_python_surface():
  p = inspect.signature(BatchedEngine.td_targets).parameters
  assert list(p)[1:] == ["T", "gamma", "lam", "values", "value0", "buffers", "bootstrap_truncated", "scalar"]
  assert all(p[k].default is None for k in ("lam", "values", "value0", "buffers"))
  assert p["bootstrap_truncated"].default is False and p["scalar"].default is False
