"""CPU tier: the two roles of the forked headline step kernel (k_step_fork, csrc/sgw_kernels.hpp) compute the same bytes.

tests/host_shim/island_fork_check.cpp runs them on the host, under the sanitizers and with pattern-initialised locals: 2 048 envs x
300 steps with 2 % QUIT / out-of-range actions.  The O role is handed the S role's state every step and plays the rules without
the regrowth pass: r[], discount, step_type, term, safety, frame, row, col, actual and cum are byte-identical to the S role's; with
the regrowth enabled (a launch that asks for `metrics`) the nine metrics are too."""
import os
import re
import subprocess

import pytest

from ai_safety_gridworlds_amd.specs import make_spec

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "island_fork_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
  if cc == CLANG:
    flags.append("-ftrivial-auto-var-init=pattern")
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "island_fork_check.cpp"), "-o", out])
  return out


@pytest.mark.parametrize("max_iterations", [100, 5])
def test_output_role_equals_state_role_on_the_host(max_iterations, exe, tmp_path):
  path = str(tmp_path / "spec.bin")
  with open(path, "wb") as f:
    f.write(bytes(make_spec("island_navigation_ex", max_iterations=max_iterations).native))
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  p = subprocess.run([exe, path], capture_output=True, text=True, env=env)
  assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
  m = re.search(r"steps (\d+) regrowths (\d+) mismatches (\d+)", p.stdout)
  assert m, p.stdout
  steps, regrowths, bad = (int(x) for x in m.groups())
  assert bad == 0
  assert steps == 2048 * 300
  if max_iterations == 100:
    assert regrowths > 1000, regrowths            # the skipped pass did change the state: the comparison is not vacuous
