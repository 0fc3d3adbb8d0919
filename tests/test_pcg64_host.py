"""CPU tier of the env-owned generator: the one definition of numpy's PCG64 stream and of the draws built on it
(csrc/sgw_pcg64.hpp: random01, lemire, interval, interval_guarded_clamped) compiled for the host by a stand-alone program
(tests/host_shim/pcg64_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a subprocess) against numpy's
Generator(PCG64(SeedSequence(seed))), every value exactly equal.  Each numpy call used here maps one-for-one onto a function of
the header: random() -> random01, integers(0, n) -> lemire(n - 1), shuffle(list) -> Fisher-Yates from the top over interval."""
import os
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
M64 = (1 << 64) - 1
SEEDS = [0, 1, 1 << 32, 17122023]          # 2^32: two entropy words


def generator(seed):
  return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


def words(seed):
  st = generator(seed).bit_generator.state["state"]
  return "%d %d %d %d" % (st["state"] >> 64, st["state"] & M64, st["inc"] >> 64, st["inc"] & M64)


def bits(x):
  return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "pcg64_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "pcg64_check.cpp"), "-o", out])
  return out


def ask(exe, lines):
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  rows = [l.split() for l in r.stdout.splitlines()]
  assert len(rows) == len(lines)
  return [[int(v) for v in row[1:]] for row in rows]


# lower case: Pcg64; upper case: Pcg64BufFirst (the same functions on the other member order)
@pytest.mark.parametrize("r", ["r", "R"])
def test_random01_matches_numpy(exe, r):
  got = ask(exe, ["%s %s 0 64" % (r, words(s)) for s in SEEDS])
  for s, g in zip(SEEDS, got):
    rng = generator(s)
    assert g == [bits(rng.random()) for _ in range(64)], "seed %d" % s


@pytest.mark.parametrize("i", ["i", "I"])
@pytest.mark.parametrize("n", [1, 2, 4, 5, 10000])
def test_lemire_matches_numpy_integers(exe, n, i):
  """65 draws: an odd count leaves the second half of a 64-bit draw buffered, and the random() that follows must not disturb it
  nor be disturbed by it (n == 1 draws nothing at all)."""
  got = ask(exe, ["%s %s %d 65" % (i, words(s), n - 1) for s in SEEDS])
  for s, g in zip(SEEDS, got):
    rng = generator(s)
    want = [int(rng.integers(0, n)) for _ in range(65)]
    assert g[:65] == want, "seed %d" % s
    assert g[65] == bits(rng.random()), "seed %d: random() after 65 32-bit draws" % s


@pytest.mark.parametrize("kind", ["s", "g", "S"])
@pytest.mark.parametrize("n", [2, 3, 7])
def test_shuffle_matches_numpy(exe, kind, n):
  """Generator.shuffle of a list, as the families apply interval: i from the top, j = interval(i), swap.  A live stream never
  reaches the guarded form's cap, so it gives the same permutation."""
  got = ask(exe, ["%s %s %d 0" % (kind, words(s), n) for s in SEEDS])
  for s, g in zip(SEEDS, got):
    want = list(range(n))
    generator(s).shuffle(want)
    assert g == want, "seed %d" % s
