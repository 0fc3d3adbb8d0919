"""CPU tier of the table policy: the one definition of its choice (csrc/sgw_policy.hpp policy_choose: ordered float32 score,
first-maximum scan, Philox exploration) compiled for the host by a stand-alone program (tests/host_shim/policy_check.cpp, built with
AddressSanitizer + UndefinedBehaviorSanitizer and run as a subprocess) against tests/policy_ref.py, every action equal."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import policy_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CELLS, ACTIONS, CODES = [1, 25, 48, 289, 1089], [4, 5, 9], [1, 2, 17, 64]
EXPLORE = [0, 1, 2 ** 31, 2 ** 32]
ROWS = 16


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "policy_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "policy_check.cpp"), "-o", out])
  return out


def weights_of(kind, rng, C, G, NA, case):
  ints = rng.integers(-3, 4, size=(C, G, NA)).astype(np.float32)           # ties and cancellations
  if kind == "integer":
    return ints
  if kind == "mixed":                                                       # 1e-3 .. 1e6: the order of the additions shows in the last bits
    return (np.sign(ints + 0.5) * 10.0 ** rng.uniform(-3.0, 6.0, size=(C, G, NA))).astype(np.float32)
  assert kind == "nan"
  w = ints.copy()
  w[rng.integers(0, C), :, case % NA] = np.nan                              # one action column turns NaN (column 0 in some cases)
  return w


def run_cases(exe, tmp_path, kind):
  rng = np.random.default_rng({"integer": 1, "mixed": 2, "nan": 3}[kind])
  cases, blob = [], []
  for case, (C, NA, G) in enumerate(itertools.product(CELLS, ACTIONS, CODES)):
    code_of = rng.integers(0, G, size=256).astype(np.uint8)
    w = weights_of(kind, rng, C, G, NA, case)
    b = rng.integers(-2, 3, size=NA).astype(np.float32) if case % 2 else None
    obs = rng.integers(0, 256, size=(ROWS, C)).astype(np.uint8)
    seed, step, agent, env0 = 1234 + case, (1 << 32) - 3 + case, case % 4, (case % 3) * (1 << 32) + 77 * case
    cases.append((C, NA, G, code_of, w, b, obs, seed, step, agent, env0))
    blob.append(struct.pack("<10q", C, G, NA, ROWS, int(b is not None), len(EXPLORE), seed, step, agent, env0))
    blob.append(np.array(EXPLORE, np.uint64).tobytes() + code_of.tobytes() + w.tobytes() + (b.tobytes() if b is not None else b"") + obs.tobytes())
  path = tmp_path / ("cases_%s.bin" % kind)
  path.write_bytes(b"".join(blob))
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  lines = [[int(v) for v in l.split()] for l in r.stdout.splitlines()]
  assert len(lines) == len(cases) * len(EXPLORE)
  explored = 0
  for i, (C, NA, G, code_of, w, b, obs, seed, step, agent, env0) in enumerate(cases):
    s = policy_ref.scores(obs, code_of, np.broadcast_to(w, (ROWS,) + w.shape), None if b is None else np.broadcast_to(b, (ROWS, NA)))
    best = policy_ref.greedy(s)
    ids = env0 + np.arange(ROWS)
    for k, eb in enumerate(EXPLORE):
      want = policy_ref.explore(best, NA, eb, seed, ids, step, agent)
      assert lines[i * len(EXPLORE) + k] == list(want), "C=%d n_actions=%d G=%d explore_below=%d (%s weights)" % (C, NA, G, eb, kind)
    explored += int((policy_ref.explore(np.full(ROWS, -1), NA, 2 ** 31, seed, ids, step, agent) >= 0).sum())
  return cases, explored


def test_integer_weights_ties_and_cancellations(exe, tmp_path):
  cases, explored = run_cases(exe, tmp_path, "integer")
  # the inputs do what they are for: some rows tie at the top (the first maximum must win) ...
  C, NA, G, code_of, w, b, obs = cases[5][:7]
  s = policy_ref.scores(obs, code_of, np.broadcast_to(w, (ROWS,) + w.shape), None)
  assert any((row == row.max()).sum() > 1 for row in s)
  # ... and explore_below = 2^31 explores about half of the rows
  assert 0.4 < explored / (len(cases) * ROWS) < 0.6


def test_mixed_magnitudes_fix_the_order_of_the_additions(exe, tmp_path):
  cases, _ = run_cases(exe, tmp_path, "mixed")
  # a pairwise sum of the same terms differs from the ordered one somewhere: the comparison above is sensitive to the order
  differ = 0
  for (C, NA, G, code_of, w, b, obs, *_rest) in cases:
    if C < 289 or b is not None:
      continue
    terms = w[np.arange(C)[None, :], code_of[obs]]                         # [rows, C, NA]
    ordered = policy_ref.scores(obs, code_of, np.broadcast_to(w, (ROWS,) + w.shape), None)
    pairwise = np.ascontiguousarray(terms.transpose(0, 2, 1)).sum(axis=2, dtype=np.float32)   # (numpy sums the contiguous axis pairwise)
    differ += int((pairwise != ordered).sum())
  assert differ > 0


def test_a_nan_column_never_displaces_and_is_never_displaced(exe, tmp_path):
  cases, _ = run_cases(exe, tmp_path, "nan")
  seen_first = seen_later = 0
  for case, (C, NA, G, code_of, w, b, obs, *_rest) in enumerate(cases):
    s = policy_ref.scores(obs, code_of, np.broadcast_to(w, (ROWS,) + w.shape), None if b is None else np.broadcast_to(b, (ROWS, NA)))
    best = policy_ref.greedy(s)
    nan0 = np.isnan(s[:, 0])
    assert (best[nan0] == 0).all()
    seen_first += int(nan0.sum())
    later = np.isnan(s).any(axis=1) & ~nan0
    assert not np.isnan(s[later, best[later]]).any()
    seen_later += int(later.sum())
  assert seen_first > 0 and seen_later > 0
