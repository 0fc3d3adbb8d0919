"""CPU tier of the softmax table-policy calls (sgw_policy_sample, sgw_policy_sample_step_n, sgw_policy_probs,
sgw_policy_accumulate_softmax): declared in include/sgw.h, exported by libsgw.so, listed in the binding with argument types, the ABI
version and the structs where they were, the refusals that need no device (the others, which need an engine, are in
tests/test_softmax_gpu.py), no scratch in the installed kernels, and the Python surface."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy, beta2_of
from tests import softmax_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"sgw_policy_sample": 7, "sgw_policy_sample_step_n": 10, "sgw_policy_probs": 11, "sgw_policy_accumulate_softmax": 13}


def _header(comments=False):
  text = open(os.path.join(REPO, "include", "sgw.h")).read()
  return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _params(header, name):
  m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
  assert m, "include/sgw.h declares %s" % name
  return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_symbols_are_declared_exported_and_listed():
  header, L = _header(), N.lib()
  assert _params(header, "sgw_policy_sample") == [
      "sgw_engine* e", "const sgw_policy* p", "float beta2", "const uint8_t* obs_dev", "int64_t t", "int8_t* actions_dev", "void* stream"]
  assert _params(header, "sgw_policy_sample_step_n") == [
      "sgw_engine* e", "const sgw_policy* p", "float beta2", "const uint8_t* obs0_dev", "int T", "int write_every", "const sgw_out* out",
      "int8_t* actions_out_dev", "int accumulate", "void* stream"]
  assert _params(header, "sgw_policy_probs") == [
      "sgw_engine* e", "const sgw_policy* p", "float beta2", "const uint8_t* obs0_dev", "const uint8_t* obs_dev", "int64_t obs_rows", "int T",
      "const int8_t* actions_dev", "float* probs_dev", "double* p_chosen_dev", "void* stream"]
  assert _params(header, "sgw_policy_accumulate_softmax") == [
      "sgw_engine* e", "const sgw_policy* p", "float beta2", "const uint8_t* obs0_dev", "const uint8_t* obs_dev", "int64_t obs_rows", "int T",
      "const int8_t* actions_dev", "const double* coef_dev", "int frac_bits", "int64_t* acc_weights_dev", "int64_t* acc_bias_dev", "void* stream"]
  for name, n_args in SYMBOLS.items():
    assert hasattr(L, name) and name in N.EXPORTS, name
    assert len(getattr(L, name).argtypes) == n_args and getattr(L, name).argtypes[2] is C.c_float, name
  assert L.sgw_policy_probs.argtypes[5] is C.c_int64 and L.sgw_policy_accumulate_softmax.argtypes[5] is C.c_int64


def test_the_header_spells_the_arithmetic_out():
  text = " ".join(_header(comments=True).split())
  for h in ("0x1.62e430p-1", "0x1.ebfbe0p-3", "0x1.c6b08ep-5", "0x1.3b2ab6p-7", "0x1.5d87fep-10", "0x1.430912p-13"):
    assert h in text, h
  for phrase in ("if !(z >= -125.0f) -> +0.0f", "k = rintf(z) (ties to even)", "E = ldexpf(p, (int)k)", "degenerate iff !(total > 0.0)",
                 "u = ((double)x0 + 0.5) * 2^-32", "NOT folded in", "beta2 * ln 2"):
    assert phrase in text, phrase
  # the reference holds the same constants, and they are float32((ln 2)^i / i!)
  want = [np.float32(math.log(2.0) ** i / math.factorial(i)) for i in range(1, 7)]
  assert [softmax_ref.C1, softmax_ref.C2, softmax_ref.C3, softmax_ref.C4, softmax_ref.C5, softmax_ref.C6] == want
  assert softmax_ref.TAG_SAMPLE == 3 and "counter = (step, 3, a, env_id >> 32)" in text
  assert "enum { TAG_SAMPLE = 3 }" in open(os.path.join(REPO, "ai_safety_gridworlds_amd", "csrc", "sgw_softmax.hpp")).read()
  assert len({philox.TAG_ACTION, philox.TAG_EPISODE, philox.TAG_POLICY, softmax_ref.TAG_SAMPLE}) == 4, "a stream of its own"


def test_the_existing_abi_did_not_move():
  header, L = _header(), N.lib()
  assert L.sgw_abi_version() == 8 and N.ABI_VERSION == 8, "entry points only: the ABI version does not move"
  assert "#define SGW_ABI_VERSION 8" in header
  assert L.sgw_sizeof_out() == 20 * C.sizeof(C.c_void_p) == C.sizeof(N.Out), "no struct change: 20 outputs"
  assert L.sgw_sizeof_policy() == C.sizeof(N.Policy) == 4 * 4 + 4 * 8 + 2 * 8 + 8, "sgw_policy did not move"


def test_refusals_that_need_no_device():
  L = N.lib()
  pol = N.Policy(source=0, n_policies=1, n_codes=2, cells=4, code_of=16, weights=16, step_dev=16)      # never dereferenced: the checks come first
  calls = {
      "sgw_policy_sample": lambda: L.sgw_policy_sample(None, C.byref(pol), 1.0, 16, 0, 16, None),
      "sgw_policy_sample_step_n": lambda: L.sgw_policy_sample_step_n(None, C.byref(pol), 1.0, 16, 8, 0, C.byref(N.Out()), 16, 0, None),
      "sgw_policy_probs": lambda: L.sgw_policy_probs(None, C.byref(pol), 1.0, 16, None, 0, 0, None, 16, None, None),
      "sgw_policy_accumulate_softmax": lambda: L.sgw_policy_accumulate_softmax(None, C.byref(pol), 1.0, 16, None, 0, 1, 16, 16, 24, 32, None, None)}
  for name, call in calls.items():
    assert call() == -1
    assert name.encode() in L.sgw_last_error() and b"null engine" in L.sgw_last_error()


def test_the_kernels_are_built_without_scratch():
  """Registers are picked by selects and the per-action terms of a transition live in LDS: the installed build's assembly reports
  no private segment and no AGPRs for the three new kernels.  One rounding per operation needs -ffp-contract=off."""
  from ai_safety_gridworlds_amd import build
  N.lib()
  if not os.path.exists(build.ASM):       # a library that travelled without its assembly: build() writes both (as test_isa_lint does)
    build.build(force=True)
  asm = open(build.ASM).read()
  for kernel in ("k_policy_sample", "k_policy_probs", "k_policy_accumulate_softmax"):
    for what in ("private_seg_size", "num_agpr"):
      m = re.search(r"\.set (\S*%s\S*)\.%s, (\d+)" % (kernel, what), asm)
      assert m, "%s is in the build" % kernel
      assert int(m.group(2)) == 0, (kernel, what)
  assert "-ffp-contract=off" in build.FLAGS


def test_temperature_maps_to_beta2():
  assert beta2_of(None) is None
  b = beta2_of(1.0)
  assert isinstance(b, np.float32) and b == np.float32(1.4426950408889634)
  assert beta2_of(0.5) == np.float32(1.4426950408889634 / 0.5)
  assert beta2_of(math.inf) == 0.0 and isinstance(beta2_of(math.inf), np.float32)
  for bad in (0.0, -1.0, float("nan"), 1e-40):
    with pytest.raises(ValueError):
      beta2_of(bad)


def test_python_surface():
  p = inspect.signature(TablePolicy.set_temperature).parameters
  assert list(p)[1:] == ["tau"]
  assert isinstance(TablePolicy.temperature, property)
  p = inspect.signature(BatchedEngine.policy_probs).parameters
  assert list(p)[1:] == ["policy", "T", "obs0", "obs", "actions"]
  assert p["T"].default == 0 and all(p[k].default is None for k in ("obs0", "obs", "actions"))
  p = inspect.signature(BatchedEngine.policy_accumulate_softmax).parameters
  assert list(p)[1:] == list(inspect.signature(BatchedEngine.policy_accumulate).parameters)[1:], "the arguments of policy_accumulate"
  assert p["frac_bits"].default == 24
  p = inspect.signature(BatchedEngine.pg_learn).parameters
  assert list(p)[1:] == ["policy", "T", "gamma", "lr", "lam", "critic", "critic_lr", "bootstrap_truncated", "frac_bits"]
  assert (p["lam"].default, p["critic"].default, p["critic_lr"].default, p["bootstrap_truncated"].default, p["frac_bits"].default) == \
      (1.0, None, None, False, 24)
