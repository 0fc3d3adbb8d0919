"""CPU tier of sgw_copy_envs: the per-item logic of csrc/sgw_copy.hpp (the row copy at every alignment, the state pair move
through state_index, the work mapping of one launch) compiled for the host by a stand-alone program
(tests/host_shim/copy_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a subprocess), which compares
every case with a naive loop and reports how many it checked."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "copy_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "copy_check.cpp"), "-o", out])
  return out


def ask(exe, mode):
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe, mode], capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  kind, count = r.stdout.split()
  assert kind == mode
  return int(count)


def test_row_copy_equals_a_byte_loop_at_every_alignment(exe):
  """Row sizes 1..40, 48, 289, 441; source and destination misalignment 0..15 each; 1, 2, 4 .. 64 cooperating lanes; the guard
  regions around both buffers keep their fill byte."""
  assert ask(exe, "rows") == 43 * 16 * 16 * 7


def test_state_move_and_launch_grid(exe):
  """words 1, 2, 7, 10, 22; engines of 130 and 70 envs; index lists with repeats, -1 and out-of-range entries, NULL lists, one
  engine onto itself (40..71 -> 96..127); output planes ride along.  Untouched envs and every allocation word past n_pad keep
  their contents; the source is not written."""
  assert ask(exe, "state") == 5 * 4
