"""island_navigation_ex's rules are stated once over a rules provider (csrc/sgw_island.hpp): IslandRulesRuntime reads flags,
parameters and level tables from the launch, IslandRulesL9 holds the default level-9 rule set as compile-time constants (the
headline's one-step kernel, k_engine<IslandL9Default, K_STEP, StepShape<6, 8, 10, ...>>).  No GPU needed:

* tests/host_shim/island_rules_check.cpp runs both on the host, under the sanitizers and with pattern-initialised locals, over
  trajectories and a sweep of single states: every state, reward vector and discount byte for byte, zero mismatches;
* `matches`, the only way into the constant provider, accepts the default spec and refuses every near miss;
* the build has the new kernel once, in registers only, and with fewer instructions than the shape-only kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.specs import make_spec

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
N_PARAMS = 34                                        # csrc/sgw_island.hpp enum P: P_COUNT
SHAPED_PREFIX = "_ZN3sgw8k_engineINS_7IslandTILb0ELb1EEELi0ENS_9StepShapeILi6ELi8ELi10E"   # k_engine<IslandPacked, K_STEP, StepShape<6, 8, 10, ...>>
RULES_PREFIX = "_ZN3sgw8k_engineINS_15IslandL9DefaultELi0ENS_9StepShapeILi6ELi8ELi10E"     # k_engine<IslandL9Default, K_STEP, the same shape>


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "island_rules_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-mfma", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]
  if cc == CLANG:
    flags.append("-ftrivial-auto-var-init=pattern")
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "island_rules_check.cpp"), "-o", out])
  return out


def _run(exe, mode, path):
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  return subprocess.run([exe, mode, path], capture_output=True, text=True, env=env)


@pytest.mark.parametrize("max_iterations", [100, 5])
def test_constant_rules_equal_runtime_rules_on_the_host(max_iterations, exe, tmp_path):
  """2 048 envs x 300 steps through k_engine's sequence (2 % QUIT / out-of-range actions), then about 2 x 10^6 single states:
  the constant providers (flags and parameters; plus level masks; the shipped IslandL9Default) against the runtime provider."""
  path = str(tmp_path / "spec.bin")
  with open(path, "wb") as f:
    f.write(bytes(make_spec("island_navigation_ex", max_iterations=max_iterations).native))
  p = _run(exe, "run", path)
  assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
  m = re.search(r"cells (\d+) trajectory_calls (\d+) calls (\d+) mismatches (\d+)", p.stdout)
  assert m, p.stdout
  cells, traj, calls, bad = (int(x) for x in m.groups())
  assert bad == 0
  assert cells == 35                                  # level 9: 48 cells, 13 walls
  assert traj == 3 * 2048 * 300                       # three providers against the runtime one
  assert calls - traj == 3 * 35 * 6 * 3 * 3200        # every (cell, action, frame), 3 200 seeded draws of the rest each


def _copy(sp):
  return N.Spec.from_buffer_copy(bytes(sp))


def _near_misses():
  base = make_spec("island_navigation_ex").native
  out = []
  for i in range(N_PARAMS):
    s = _copy(base); s.params[i] = base.params[i] + 1.0; out.append(("parameter %d + 1" % i, s))
    s = _copy(base); s.params[i] = float(np.nextafter(base.params[i], np.inf)); out.append(("parameter %d + 1 ulp" % i, s))
    if base.params[i] == 0.0:
      s = _copy(base); s.params[i] = -0.0; out.append(("parameter %d = -0.0" % i, s))
  for bit in (1, 2, 4, 8):
    s = _copy(base); s.flags = base.flags ^ bit; out.append(("flag bit %d toggled" % bit, s))
  out.append(("level 8", _copy(make_spec("island_navigation_ex", level=8).native)))
  HW = base.H * base.W
  for field, cell in (("static_board", 10), ("art", 27), ("aux", HW - 1), ("static_board", 0), ("art", 18), ("aux", 0)):
    s = _copy(base); getattr(s, field)[cell] ^= 1; out.append(("%s[%d] changed" % (field, cell), s))
  return out


def test_matches_accepts_the_default_spec_only(exe, tmp_path):
  accepted = [("default", make_spec("island_navigation_ex").native), ("max_iterations 5", make_spec("island_navigation_ex", max_iterations=5).native)]
  refused = _near_misses()
  assert sum(1 for what, _ in refused if what.endswith("-0.0")) == 8        # the eight parameters that are +0.0 by default
  assert len(refused) == 2 * N_PARAMS + 8 + 4 + 1 + 6
  path = str(tmp_path / "specs.bin")
  with open(path, "wb") as f:
    for _, s in accepted + refused:
      f.write(bytes(s))
  p = _run(exe, "matches", path)
  assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
  got = p.stdout.strip()
  assert len(got) == len(accepted) + len(refused), got
  for (what, _), c in zip(accepted + refused, got):
    assert c == ("1" if what in ("default", "max_iterations 5") else "0"), what


def _kernel(asm, prefix):
  names = sorted(set(re.findall(r"^(%s\w*):" % prefix, asm, re.M)))
  assert len(names) == 1, names
  k = names[0]
  body = asm[asm.index(k + ":"):]
  return k, body[:body.index(".Lfunc_end")]


def _instructions(body):
  return [l.split()[0] for l in body.splitlines() if re.match(r"\s+(s|v|ds|global|buffer|flat|scratch)_\w+", l)]


def test_rules_kernel_is_built_in_registers_and_is_shorter():
  if not os.path.exists("/opt/rocm/bin/hipcc"):
    pytest.skip("hipcc not present")
  from ai_safety_gridworlds_amd import build as B
  B.build()
  if not os.path.exists(B.ASM) or os.path.getmtime(B.ASM) < max(os.path.getmtime(d) for d in B._deps()):
    B.build(force=True)
  asm = open(B.ASM).read()
  k, body = _kernel(asm, RULES_PREFIX)
  _, shaped = _kernel(asm, SHAPED_PREFIX)                 # still there, once: every engine with SGW_GENERIC_RULES, near-miss specs
  assert re.search(r"\.set %s\.private_seg_size, 0$" % re.escape(k), asm, re.M), "the rules kernel uses scratch memory"
  assert not re.search(r"^\s+v_(writelane|readlane)_b32", body, re.M), "the rules kernel spills SGPRs"
  m = re.search(r"\.set %s\.num_vgpr, (\d+)$" % re.escape(k), asm, re.M)
  assert m and int(m.group(1)) <= 128, m and m.group(1)
  n_rules, n_shaped = len(_instructions(body)), len(_instructions(shaped))
  print("static instructions: rules kernel %d, shape-only kernel %d" % (n_rules, n_shaped))
  assert n_rules < n_shaped
