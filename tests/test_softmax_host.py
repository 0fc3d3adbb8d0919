"""CPU tier of the softmax table policy: the one definition of its element rules (csrc/sgw_softmax.hpp: softmax_exp2,
softmax_weights, softmax_choose, softmax_pi, softmax_grad over sgw_policy.hpp's policy_score) compiled for the host by a stand-alone
program (tests/host_shim/softmax_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and -ffp-contract=off, run as a
subprocess) against tests/softmax_ref.py: integers equal, float bits equal; E against np.exp2 within a derived margin; the edge rows
of the rule; and the sampler's frequencies on the reference alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import learn_ref
from tests import policy_ref
from tests import softmax_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ROWS = 24
BETAS = (0.0, 2.0 ** -10, 1.4427, 64.0)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "softmax_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "softmax_check.cpp"), "-o", out])
  return out


def run(exe, tmp_path, blob):
  src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
  src.write_bytes(blob)
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  return dst.read_bytes()


def rows_section(C, G, NA, code_of, w, b, obs, j, env_id, coef, beta2, frac_bits=24, step=0, agent=0, explore_below=0, seed=0):
  rows = obs.shape[0]
  return (struct.pack("<9q", 2, C, G, NA, rows, int(b is not None), frac_bits, step, agent) + struct.pack("<2Q", explore_below, seed) +
          struct.pack("<2f", beta2, 0.0) + code_of.tobytes() + np.ascontiguousarray(w, np.float32).tobytes() +
          (np.ascontiguousarray(b, np.float32).tobytes() if b is not None else b"") + np.ascontiguousarray(obs, np.uint8).tobytes() +
          np.ascontiguousarray(j, np.int32).tobytes() + np.ascontiguousarray(env_id, np.int64).tobytes() +
          np.ascontiguousarray(coef, np.float64).tobytes())


def rows_result(raw, at, rows, NA):
  out = {}
  for name, dt, n in (("w", np.float32, rows * NA), ("total", np.float64, rows), ("index", np.int32, rows), ("probs", np.float32, rows * NA),
                      ("pi", np.float64, rows * NA), ("q", np.int64, rows * NA)):
    out[name] = np.frombuffer(raw, dt, n, at)
    at += n * np.dtype(dt).itemsize
  for name in ("w", "probs", "pi", "q"):
    out[name] = out[name].reshape(rows, NA)
  return out, at


def score_rows(scores, beta2, j=None, coef=None, **kw):
  """A section whose score vector IS the bias (C = 0): one row per call of the rule on hand-made scores."""
  scores = np.asarray(scores, np.float32)
  NA = scores.size
  j = np.zeros(1, np.int32) if j is None else np.array([j], np.int32)
  coef = np.ones(1) if coef is None else np.array([coef], np.float64)
  return rows_section(0, 1, NA, np.zeros(256, np.uint8), np.zeros((0, 1, NA), np.float32), scores, np.zeros((1, 0), np.uint8), j,
                      np.zeros(1, np.int64), coef, beta2, **kw)


@pytest.mark.parametrize("NA", [1, 5, 9, 16])
def test_rules_equal_the_numpy_statement(exe, tmp_path, NA):
  rng = np.random.default_rng(60 + NA)
  cases, blob = [], []
  for C, G in ((0, 3), (1, 1), (48, 9), (1089, 64)):
    for kind in ("integer", "mixed", "nan", "inf"):
      for bi, beta2 in enumerate(BETAS):
        code_of = rng.integers(0, G, size=256).astype(np.uint8)
        w = rng.integers(-3, 4, size=(C, G, NA)).astype(np.float32)
        if kind != "integer":
          w = (np.sign(w + 0.5) * 10.0 ** rng.uniform(-3.0, 2.0, size=w.shape)).astype(np.float32)
        if kind == "nan" and C > 0:
          w[rng.integers(0, C), :, rng.integers(0, NA)] = np.nan
        if kind == "inf" and C > 0:
          w[rng.integers(0, C), :, rng.integers(0, NA)] = np.inf
          w[rng.integers(0, C), :, rng.integers(0, NA)] = -np.inf
        b = rng.integers(-2, 3, size=NA).astype(np.float32) if (bi + C) % 2 else None
        if C == 0:
          b = rng.integers(-2, 3, size=NA).astype(np.float32)
          if kind == "nan":
            b[rng.integers(0, NA)] = np.nan
          if kind == "inf":
            b[rng.integers(0, NA)] = [np.inf, -np.inf][bi % 2]
        obs = rng.integers(0, 256, size=(ROWS, C)).astype(np.uint8)
        j = rng.integers(-1, NA + 1, size=ROWS).astype(np.int32)
        env_id = rng.integers(0, 2 ** 40, size=ROWS).astype(np.int64)
        coef = rng.normal(size=ROWS) * 10.0 ** rng.uniform(-3, 3, size=ROWS)
        coef[:4] = learn_ref.special_coefs(24)[[0, 1, 7, 13]]
        frac_bits = (0, 24, 52, 24)[bi]
        explore_below = (0, 2 ** 31)[bi % 2]
        step, agent, seed = int(rng.integers(0, 2 ** 33)), int(rng.integers(0, 4)), int(rng.integers(0, 2 ** 63))
        cases.append((C, G, code_of, w, b, obs, j, env_id, coef, beta2, frac_bits, explore_below, step, agent, seed, kind))
        blob.append(rows_section(C, G, NA, code_of, w, b, obs, j, env_id, coef, beta2, frac_bits, step, agent, explore_below, seed))
  raw, at = run(exe, tmp_path, b"".join(blob)), 0
  degenerate = sampled = explored = 0
  for (C, G, code_of, w, b, obs, j, env_id, coef, beta2, frac_bits, explore_below, step, agent, seed, kind) in cases:
    got, at = rows_result(raw, at, ROWS, NA)
    what = "C=%d G=%d n_actions=%d bias=%r beta2=%r (%s weights)" % (C, G, NA, b is not None, beta2, kind)
    s = policy_ref.scores(obs, code_of, np.broadcast_to(w, (ROWS,) + w.shape), None if b is None else np.broadcast_to(b, (ROWS, NA)))
    best, ww, total = S.weights(s, beta2)
    assert learn_ref.same_f32(got["w"], ww), what
    assert learn_ref.same_f64(got["total"], total), what
    assert not np.isnan(total).any() and (ww >= 0).all()
    idx = S.sample(s, beta2, explore_below, seed, env_id, step, agent)
    assert np.array_equal(got["index"], idx), what
    pi, live = S.pi_of(s, beta2)
    assert learn_ref.same_f64(got["pi"], pi) and learn_ref.same_f32(got["probs"], pi.astype(np.float32)), what
    assert np.array_equal(live, total > 0.0)
    assert (live == np.isfinite(s[np.arange(ROWS), best])).all(), "degenerate exactly when top is NaN or infinite"
    inside = (j >= 0) & (j < NA)
    q = S.grad_terms(pi, np.clip(j, 0, NA - 1), coef, frac_bits)
    q[~(live & inside)] = 0
    assert np.array_equal(got["q"], q), what
    plain = S.sample(s, beta2, 0, seed, env_id, step, agent)
    assert (plain[~live] == best[~live]).all(), "a degenerate row falls back to the first maximum"
    assert (ww[np.arange(ROWS), plain][live] > 0).all(), "a weight of 0 is never sampled"
    degenerate += int((~live).sum()); sampled += int(live.sum())
    explored += int((idx != plain).sum())
    if beta2 == 0.0:
      finite = np.isfinite(s)
      assert ((ww == 1.0) == finite)[live].all() and (ww[live][~finite[live]] == 0).all(), "beta2 = 0: uniform over the finite scores"
  assert at == len(raw)
  assert sampled > 0 and (degenerate > 0 or NA == 1) and (explored > 0 or NA == 1)


def _rel_err(e, z):
  want = np.exp2(z.astype(np.float64))
  return np.abs(e.astype(np.float64) - want) / want


# The margin of E against 2^z.  Truncation: the degree-6 Taylor polynomial of 2^g on |g| <= 0.5 is off by at most
# 0.5^7 (ln 2)^7 / 7! = 1.2e-7, relative to 2^g >= 0.707: 1.7e-7.  Rounding: each float32 operation of the Horner chain is off by at
# most 2^-24 of a value below 1.5, and an error made d levels inside the chain reaches the result scaled by |g|^d <= 0.5^d: with
# two operations per level below 1.5 * 2^-24 * (1 + 2 * (0.5 + 0.25 + ...)) = 2.7e-7, relative 3.8e-7.  The scaling by 2^k is exact.
# Together below 5.5e-7, and 2^-20 = 9.5e-7 holds it.  Measured: 2^-21.96.
BOUND = 2.0 ** -20


def test_exp2_against_numpy_over_the_top_two_units(exe, tmp_path):
  """Every float32 of [-2, 0] at stride 7 (153 million values, a chunk at a time): within BOUND of np.exp2 in double, and bit for
  bit the numpy statement on every 16th of them."""
  lo, hi, worst = 0x80000000, 0xC0000000, 0.0
  chunk = 7 * (1 << 24)
  for start in range(lo, hi + 1, chunk):
    bits = np.arange(start, min(start + chunk, hi + 1), 7, dtype=np.uint64).astype(np.uint32)
    z = bits.view(np.float32)
    raw = run(exe, tmp_path, struct.pack("<2q", 1, z.size) + z.tobytes())
    e = np.frombuffer(raw, np.float32)
    worst = max(worst, float(_rel_err(e, z).max()))
    assert learn_ref.same_f32(e[::16], S.exp2_rule(z[::16]))
  print("E against np.exp2 on [-2, 0]: max relative error 2^%.2f" % np.log2(worst))
  assert worst <= BOUND


def test_exp2_against_numpy_down_to_the_cut(exe, tmp_path):
  rng = np.random.default_rng(5)
  z = np.concatenate([rng.uniform(-125.0, -2.0, size=10 ** 6), np.arange(-125, 1), np.arange(-125, 0) + 0.5]).astype(np.float32)
  assert z.min() == -125.0
  raw = run(exe, tmp_path, struct.pack("<2q", 1, z.size) + z.tobytes())
  e = np.frombuffer(raw, np.float32)
  assert learn_ref.same_f32(e, S.exp2_rule(z))
  worst = float(_rel_err(e, z).max())
  print("E against np.exp2 on [-125, -2]: max relative error 2^%.2f" % np.log2(worst))
  assert worst <= BOUND
  assert e.min() == 2.0 ** -125 and (e >= 2.0 ** -126).all(), "never subnormal: the smallest non-zero E is 2^-125"
  k = np.arange(-125, 1).astype(np.float32)
  assert np.array_equal(S.exp2_rule(k), np.exp2(k)), "integers are exact"
  g = (z - np.rint(z)).astype(np.float64)
  assert np.array_equal(g, z.astype(np.float64) - np.rint(z.astype(np.float64))), "z - k is exact"


def test_edge_rows(exe, tmp_path):
  below = np.nextafter(np.float32(-125.0), np.float32(-np.inf))
  rows = [([np.nan, 1.0, 2.0], 1.0, 0),                  # top NaN (score[0] is never displaced): best = 0
          ([1.0, np.inf, 2.0, np.inf], 1.0, 1),          # top +inf: best = the first of them
          ([-np.inf, -np.inf, -np.inf], 1.0, 0),         # all -inf
          ([-np.inf, 3.0, np.nan, 2.0], 1.4427, None),   # -inf and NaN scores beside a finite top: never sampled
          ([0.0, -125.0], 1.0, None),                    # z = -125.0f is kept
          ([0.0, below], 1.0, None),                     # the next float below it gives 0
          ([0.0, -1e30, 5.0], 64.0, None),               # z overflows to -inf: 0
          ([2.0, 2.0, 2.0], 0.0, None)]                  # beta2 = 0
  blob = b"".join(score_rows(s, beta2, j=len(s) - 1, coef=0.75, seed=9) for s, beta2, _ in rows)
  raw, at, results = run(exe, tmp_path, blob), 0, []
  for s, beta2, fallback in rows:
    NA = len(s)
    got, at = rows_result(raw, at, 1, NA)
    results.append(got)
    sc = np.array([s], np.float32)
    best, w, total = S.weights(sc, beta2)
    pi, live = S.pi_of(sc, beta2)
    assert learn_ref.same_f32(got["w"], w) and learn_ref.same_f64(got["total"], total) and learn_ref.same_f64(got["pi"], pi), s
    assert got["index"][0] == S.sample(sc, beta2, 0, 9, np.zeros(1, np.int64), 0, 0)[0]
    if fallback is not None:
      assert not live[0] and total[0] == 0.0 and got["index"][0] == fallback == best[0], s
      assert list(got["probs"][0]) == [1.0 if k == fallback else 0.0 for k in range(NA)] and not got["q"].any(), s
    else:
      assert live[0] and total[0] > 0.0
      assert np.array_equal(got["q"][0], S.grad_terms(pi, np.array([NA - 1]), np.array([0.75]), 24)[0])
  assert at == len(raw)
  never, kept, cut, far = results[3], results[4], results[5], results[6]
  assert list(never["w"][0]) == [0.0, 1.0, 0.0, S.exp2_rule(np.float32(-1.0) * np.float32(1.4427))], "a -inf or NaN score is never sampled"
  assert kept["w"][0, 1] == np.float32(2.0 ** -125), "z = -125.0f is kept"
  assert cut["w"][0, 1] == 0.0 and not np.signbit(cut["w"][0, 1]), "the next float below -125 gives +0.0"
  assert list(far["w"][0]) == [0.0, 0.0, 1.0]


SAMPLER_SEED = 17        # confirmed on the CPU: this seed satisfies the bound below (the test is deterministic)


def test_sampler_frequencies_on_the_reference():
  """Scores [0, 1, 2, 3, 4], beta2 = 1, env ids 0 .. 65535, one step: every action's count within 5 sqrt(n pi (1 - pi)) of n pi."""
  n = 65536
  s = np.broadcast_to(np.arange(5, dtype=np.float32), (n, 5))
  idx = S.sample(s, 1.0, 0, SAMPLER_SEED, np.arange(n), 0, 0)
  pi = S.pi_of(s[:1], 1.0)[0][0]
  assert np.allclose(pi, 2.0 ** np.arange(5) / 31.0, rtol=0, atol=1e-6)
  counts = np.bincount(idx, minlength=5)
  print("counts", counts, "expected", n * pi)
  assert counts.sum() == n
  assert (np.abs(counts - n * pi) <= 5.0 * np.sqrt(n * pi * (1.0 - pi))).all()
