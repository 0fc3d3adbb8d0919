"""CPU tier of the learning calls: the one definition of their element rules (csrc/sgw_learn.hpp: learn_scores_element over
sgw_policy.hpp's policy_score, learn_quantise, learn_apply_element) compiled for the host by a stand-alone program
(tests/host_shim/learn_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and -ffp-contract=off, run as a
subprocess) against tests/learn_ref.py: integers equal, float bits equal."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import learn_ref as R
from tests import policy_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ROWS = 24


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "learn_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "learn_check.cpp"), "-o", out])
  return out


def run(exe, tmp_path, blob):
  src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
  src.write_bytes(blob)
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  return dst.read_bytes()


@pytest.mark.parametrize("NA", [1, 5, 9, 16])
def test_scores_equal_the_policy_reference(exe, tmp_path, NA):
  rng = np.random.default_rng(40 + NA)
  cases, blob = [], []
  for C, G in ((0, 3), (1, 1), (48, 9), (289, 17), (1089, 64)):
    for has_bias in (False, True):
      for kind in ("integer", "mixed", "nan"):
        code_of = rng.integers(0, G, size=256).astype(np.uint8)
        w = rng.integers(-3, 4, size=(C, G, NA)).astype(np.float32)
        if kind != "integer":
          w = (np.sign(w + 0.5) * 10.0 ** rng.uniform(-3.0, 6.0, size=w.shape)).astype(np.float32)
        if kind == "nan" and C > 0:
          w[rng.integers(0, C), :, rng.integers(0, NA)] = np.nan
        b = rng.integers(-2, 3, size=NA).astype(np.float32) if has_bias else None
        obs = rng.integers(0, 256, size=(ROWS, C)).astype(np.uint8)
        j = rng.integers(-2, NA + 2, size=ROWS).astype(np.int32)
        cases.append((C, G, code_of, w, b, obs, j, kind))
        blob.append(struct.pack("<6q", 1, C, G, NA, ROWS, int(has_bias)) + code_of.tobytes() + w.tobytes() + (b.tobytes() if has_bias else b"") +
                    obs.tobytes() + j.tobytes())
  raw, at, nan_rows = run(exe, tmp_path, b"".join(blob)), 0, 0
  for (C, G, code_of, w, b, obs, j, kind) in cases:
    sc = np.frombuffer(raw, np.float32, ROWS * NA, at).reshape(ROWS, NA); at += 4 * ROWS * NA
    vmax = np.frombuffer(raw, np.float64, ROWS, at); at += 8 * ROWS
    chosen = np.frombuffer(raw, np.float64, ROWS, at); at += 8 * ROWS
    want = policy_ref.scores(obs, code_of, np.broadcast_to(w, (ROWS,) + w.shape), None if b is None else np.broadcast_to(b, (ROWS, NA)))
    what = "C=%d G=%d n_actions=%d bias=%r (%s weights)" % (C, G, NA, b is not None, kind)
    assert R.same_f32(sc, want), what
    best = policy_ref.greedy(want)
    assert R.same_f64(vmax, want[np.arange(ROWS), best].astype(np.float64)), what
    inside = (j >= 0) & (j < NA)
    assert R.same_f64(chosen, np.where(inside, want[np.arange(ROWS), np.clip(j, 0, NA - 1)].astype(np.float64), 0.0)), what
    assert not np.signbit(chosen[~inside]).any(), "an action outside the range gives +0.0"
    nan_rows += int(np.isnan(want).any(axis=1).sum())
    # the reference-side statement of learn_ref.scores is the same thing
    sc2, vmax2, chosen2 = R.scores(np.stack([obs, obs]), code_of, w[None, None], None if b is None else b[None, None], None, [C], [0],
                                   (j[None, :, None]).astype(np.int8), 0)
    assert R.same_f32(sc2[0, :, 0], want) and R.same_f64(vmax2[0, :, 0], vmax) and R.same_f64(chosen2[0, :, 0], chosen), what
  assert at == len(raw)
  assert nan_rows > 0 or NA == 1, "NaN weights reached the scores"


@pytest.mark.parametrize("frac_bits", [0, 1, 24, 31, 52])
def test_quantisation(exe, tmp_path, frac_bits):
  rng = np.random.default_rng(7 + frac_bits)
  u = 2.0 ** -frac_bits
  halves = (rng.integers(-2 ** 30, 2 ** 30, size=400).astype(np.float64) + 0.5) * u          # exact ties, both parities
  small = rng.uniform(-0.5, 0.5, size=200) * u                                                # below half a unit: 0
  near = (np.float64(R.Q_MAX) + rng.integers(-3, 4, size=50) + rng.choice([0.0, 0.25, 0.5, 0.75], size=50)) * u
  coef = np.concatenate([R.special_coefs(frac_bits), halves, small, near, -near, rng.normal(size=400) * 1e3, rng.normal(size=100) * 1e-9])
  raw = run(exe, tmp_path, struct.pack("<3q", 2, coef.size, frac_bits) + coef.tobytes())
  got = np.frombuffer(raw, np.int64)
  want = R.quantise(coef, frac_bits)
  assert np.array_equal(got, want)
  # the reference restated with exact integer arithmetic on the ties: round half to even
  k = np.floor(halves / u).astype(np.int64)                                                   # halves = (k + 0.5) u, exact for |k| < 2^30
  even = np.where(k % 2 == 0, k, k + 1)
  assert np.array_equal(want[len(R.special_coefs(frac_bits)):][:400], even)
  assert (np.abs(want) <= R.Q_MAX).all() and (want == R.Q_MAX).any() and (want == -R.Q_MAX).any()
  sp = want[:len(R.special_coefs(frac_bits))]
  assert list(sp[:9]) == [0, R.Q_MAX, -R.Q_MAX, 0, 0, R.Q_MAX, -R.Q_MAX, R.Q_MAX, -R.Q_MAX]
  assert (want[len(R.special_coefs(frac_bits)) + 400:][:200] == 0).all(), "values below half a unit are skipped"


def test_apply_rule(exe, tmp_path):
  rng = np.random.default_rng(3)
  n = 4000
  w = (np.sign(rng.normal(size=n)) * 10.0 ** rng.uniform(-6, 6, size=n)).astype(np.float32)
  acc = rng.integers(-2 ** 40, 2 ** 40, size=n).astype(np.int64)
  acc[rng.random(n) < 0.3] = 0
  w[:8] = [-0.0, 0.0, np.inf, -np.inf, np.nan, 1.0, -0.0, 3.4e38]
  acc[:8] = [0, 0, 5, 0, 0, 2 ** 53 + 1, 3, 2 ** 62]                   # acc == 0 on a -0.0; above 2^53: int64 -> double rounds
  acc[8], acc[9] = -(2 ** 63), 2 ** 63 - 1
  blob, cases = [], []
  for frac_bits, lr in ((24, 0.1), (0, 1e-3), (52, 0.5), (24, -0.25), (31, 1e30), (24, 0.0)):
    cases.append((frac_bits, lr))
    blob.append(struct.pack("<3q", 3, n, frac_bits) + struct.pack("<d", lr) + w.tobytes() + acc.tobytes())
  raw = run(exe, tmp_path, b"".join(blob))
  for i, (frac_bits, lr) in enumerate(cases):
    got = np.frombuffer(raw, np.float32, n, 4 * n * i)
    want = R.apply(w, acc, lr, frac_bits)
    assert R.same_f32(got, want), "frac_bits=%d lr=%r" % (frac_bits, lr)
    assert got.view(np.uint32)[0] == 0x80000000 and got.view(np.uint32)[1] == 0, "acc == 0: the bits stay, a -0.0 included"
    still = acc == 0
    assert np.array_equal(got.view(np.uint32)[still], w.view(np.uint32)[still])
  # the double rounding is in the rule: a float32-only update would differ
  want = R.apply(w, acc, 0.1, 24)
  f32 = (w + np.float32(0.1) * (acc.astype(np.float32) * np.float32(2.0 ** -24))).astype(np.float32)
  assert (want[acc != 0].view(np.uint32) != f32[acc != 0].view(np.uint32)).any()
  assert float(np.float64(2 ** 53 + 1)) == float(2 ** 53), "the accumulator above 2^53 is rounded once on the way to double"
