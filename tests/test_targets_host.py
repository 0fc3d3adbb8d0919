"""CPU tier of sgw_td_targets: the one definition of its rule (csrc/sgw_targets.hpp td_element: one element's backward loop over
T with the grouped loads) compiled for the host by a stand-alone program (tests/host_shim/targets_check.cpp, built with
AddressSanitizer + UndefinedBehaviorSanitizer and -ffp-contract=off, run as a subprocess) against tests/targets_ref.py over random
step-type sequences and the edge cases of the GPU tier, every double's bits equal."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import targets_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "targets_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "targets_check.cpp"), "-o", out])
  return out


def run_cases(exe, tmp_path, calls):
  """calls: (case, flags, with_value, asked) -> per call (ret, adv, valid) as the program left them."""
  blob = []
  for c, flags, with_value, asked in calls:
    outs = sum(1 << i for i, on in enumerate(asked) if on)
    blob.append(struct.pack("<10q", c["T"], c["n"], c["A"], c["C"], c["R"], flags, int(with_value), outs, c["src_rows"], c["dst_rows"]))
    blob.append(struct.pack("<d", c["lam"]) + c["gamma"].astype(np.float64).tobytes() + c["reward"].tobytes() + c["step_type"].tobytes() +
                c["term_reason"].tobytes())
    if with_value:
      blob.append(c["value"].tobytes() + c["value0"].tobytes())
  src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
  src.write_bytes(b"".join(blob))
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  raw, at, out = dst.read_bytes(), 0, []
  for c, _, _, _ in calls:
    shape = (c["T"], c["dst_rows"], c["A"], c["C"])
    nd = int(np.prod(shape))
    ret = np.frombuffer(raw, np.float64, nd, at).reshape(shape); at += 8 * nd
    adv = np.frombuffer(raw, np.float64, nd, at).reshape(shape); at += 8 * nd
    valid = np.frombuffer(raw, np.uint8, nd // c["C"], at).reshape(shape[:3]); at += nd // c["C"]
    out.append((ret, adv, valid))
  assert at == len(raw)
  return out


def check(exe, tmp_path, calls):
  for (c, flags, with_value, asked), got in zip(calls, run_cases(exe, tmp_path, calls)):
    want = R.expected(c, flags, with_value, want_adv=asked[1])
    R.check_outputs(c, got, want, asked, "T=%d n=%d A=%d C=%d R=%d flags=%d value=%r" % (c["T"], c["n"], c["A"], c["C"], c["R"], flags, with_value))


def test_the_vectorised_reference_is_the_element_loop():
  """tests/targets_ref.py states the rule twice: vectorised over the elements (what the larger shapes use) and element by element
  with Python floats.  They agree bit for bit, with and without values, with and without the bootstrap flag."""
  rng = np.random.default_rng(11)
  for (A, C, Rr) in ((1, 3, 1), (2, 2, 2), (3, 1, 1)):
    c = R.make_case(rng, 9, 14, A, C, Rr, 14, 14, 0.95)
    for flags in (0, 1):
      for with_value in (False, True):
        n = c["n"]
        args = (c["reward"], c["step_type"], c["term_reason"], c["value"] if with_value else None, c["value0"] if with_value else None,
                c["gamma"], c["lam"], flags)
        a, b = R.td_targets(*args), R.td_targets_scalar_loop(*args)
        assert R.same_bits(a[0], b[0]) and np.array_equal(a[2], b[2])
        assert (a[1] is None) == (b[1] is None) and (a[1] is None or R.same_bits(a[1], b[1]))


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 9, 13])          # around the depth of a load group (4 rows), one row, several groups
def test_random_sequences_bit_equal(exe, tmp_path, T):
  rng = np.random.default_rng(100 + T)
  calls = []
  for n, (A, C), lam in ((1, (1, 10), 0.95), (7, (2, 4), 0.0), (33, (1, 1), 1.0), (20, (3, 3), 0.95), (5, (4, 16), 0.95)):
    for Rr in sorted({1, A}):
      for pad in (0, 3):
        c = R.make_case(rng, T, n, A, C, Rr, n + 5, n + pad, lam)
        for flags in (0, 1):
          calls.append((c, flags, True, (True, True, True)))
        calls.append((c, 1, False, (True, False, True)))
  check(exe, tmp_path, calls)


def test_output_subsets_and_special_elements(exe, tmp_path):
  rng = np.random.default_rng(5)
  c = R.make_case(rng, 9, 12, 2, 4, 2, 64, 12, 0.95)
  calls = [(c, 1, True, asked) for asked in ((True, False, False), (False, True, False), (False, False, True), (True, True, True))]
  calls.append((c, 0, False, (True, False, False)))
  check(exe, tmp_path, calls)
  ret, adv, valid = run_cases(exe, tmp_path, calls[3:4])[0]
  t, i, a = c["special"]["negzero"]
  assert (ret[t, i, a] == 0).all() and np.signbit(ret[t, i, a]).all(), "a terminated LAST returns its reward itself: -0.0 stays -0.0"
  t, i, a = c["special"]["nan"]
  assert np.isnan(ret[t, i, a, 0]) and np.isnan(adv[t, i, a, 0]) and valid[t, i, a] == 1
  t, i, a = c["special"]["inf"]
  assert not np.isfinite(adv[t, i, a, -1]) or c["step_type"][t, i, a] != R.MID      # (a terminated LAST does not read its own value)
  # the inputs do what they are for: every pattern was drawn, dead rows are invalid, both reasons occur at LAST rows
  st = c["step_type"][:, :c["n"]]
  assert set(np.unique(c["which"])) == set(range(len(R.PATTERNS)))
  assert (valid[:, :c["n"]][(st != R.MID) & (st != R.LAST)] == 0).all() and (st == R.DEAD).any() and (st == 77).any() and (st == R.FIRST).any()
  last = st == R.LAST
  reasons = {int(c["term_reason"][t, i, a]) for t, i, a in np.argwhere(last)}
  assert reasons == {R.TERMINATED, R.MAX_STEPS}
  boot, plain = R.expected(c, 1), R.expected(c, 0)
  assert not R.same_bits(boot[0], plain[0]), "the bootstrap flag changes the returns of the truncated episodes"


def test_a_fused_multiply_add_would_show():
  """The generator tells a contracted build from the contract: the correctly rounded r + g * v differs from the two-rounding value
  on far more than 5 % of the elements at g = 0.99."""
  rng = np.random.default_rng(9)
  r, v = R.numbers(rng, (4000,)), R.numbers(rng, (4000,))
  assert R.fused_differs(r, 0.99, v) >= 0.05
