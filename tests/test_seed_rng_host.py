"""CPU tier of device-side seeding: the arithmetic of csrc/sgw_seed.hpp (numpy's SeedSequence + PCG64 seeding, the reference's
crc32 layout-seed rule, the SGW_SEED_LOW32 cut and the `base + index` form) compiled for the host by a stand-alone program
(tests/host_shim/seed_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a subprocess) against numpy
and zlib."""
import os
import subprocess
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
EDGE_SEEDS = [0, 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) + 3, 1 << 63, (1 << 64) - 1]


def numpy_words(seed):
  st = np.random.PCG64(np.random.SeedSequence(int(seed))).state["state"]
  return [st["state"] >> 64, st["state"] & M64, st["inc"] >> 64, st["inc"] & M64]


def reference_crc(original_seed, layout_seed):
  """safety_game_moma.py:850-852"""
  return zlib.crc32(b"".join(int(x).to_bytes(4, byteorder="big") for x in (original_seed, layout_seed, 17122023)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "seed_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "seed_check.cpp"), "-o", out])
  return out


def ask(exe, lines):
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  rows = [l.split() for l in r.stdout.splitlines()]
  assert len(rows) == len(lines)
  return [[int(v) for v in row[1:]] for row in rows]


def test_pcg_words_match_numpy(exe):
  rng = np.random.Generator(np.random.PCG64(20251))
  seeds = EDGE_SEEDS + [int(s) for s in rng.integers(0, 1 << 63, size=2000, dtype=np.uint64)]
  got = ask(exe, ["p %d 0" % s for s in seeds])
  for s, g in zip(seeds, got):
    assert g == numpy_words(s), "seed %d" % s


def test_crc_matches_zlib(exe):
  assert reference_crc(7, 2) == 0x27220714
  rng = np.random.Generator(np.random.PCG64(20252))
  pairs = [(0, 0), (M32, M32), (7, 2)] + [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, size=(500, 2), dtype=np.uint64)]
  got = ask(exe, ["c %d %d" % p for p in pairs])
  for p, g in zip(pairs, got):
    assert g == [reference_crc(*p)], p
  assert got[2] == [0x27220714]


def test_low32_cut_and_layout_rule(exe):
  """SGW_SEED_LOW32 (flags = 1) cuts the seed before anything else; a layout seed replaces the seed by the crc of its low 32
  bits, with or without the flag; the generator is numpy's for the resolved seed."""
  rng = np.random.Generator(np.random.PCG64(20253))
  seeds = EDGE_SEEDS + [int(s) for s in rng.integers(0, 1 << 63, size=200, dtype=np.uint64)]
  got = ask(exe, ["p %d 1" % s for s in seeds])
  for s, g in zip(seeds, got):
    assert g == numpy_words(s & M32), "seed %d" % s
  assert got[4] == numpy_words(0) and got[5] == numpy_words(1), "2^32 and 2^32 + 1 under the cut"
  layouts = [0, 1, 2, M32] + [int(x) for x in rng.integers(0, 1 << 32, size=len(seeds) - 4, dtype=np.uint64)]
  for flags in (0, 1):
    got = ask(exe, ["l %d %d %d" % (s, l, flags) for s, l in zip(seeds, layouts)])
    for s, l, g in zip(seeds, layouts, got):
      want = reference_crc(s & M32, l)
      assert g[0] == want and g[1:] == numpy_words(want), (s, l, flags)


def test_base_plus_index_wraps_mod_2_64(exe):
  cases = [(0, 0, 0), (2000, 5, 0), (M64, 1, 0), (M64 - 2, 7, 0), ((1 << 32) - 1, 1, 0), ((1 << 32) - 1, 1, 1), (M64, 1, 1), (1 << 63, 1 << 40, 1)]
  got = ask(exe, ["b %d %d %d" % c for c in cases])
  for (base, i, flags), g in zip(cases, got):
    want = (base + i) & M64
    assert g == [want & M32 if flags else want], (base, i, flags)
