"""CPU tier of the what-if kernels: the one definition of their rule (csrc/sgw_whatif.hpp whatif_moves: the ordered loop over
the actions with the carried position; whatif_fold: the ordered mean per tile type) compiled for the host by a stand-alone program
(tests/host_shim/whatif_check.cpp, built with AddressSanitizer + UndefinedBehaviorSanitizer and run as a subprocess) against
tests/whatif_ref.py over the reference's fixture rows and over random boards, every byte and every double's bits equal."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import whatif_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "host_shim")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
  out = str(tmp_path_factory.mktemp("host") / "whatif_check")
  cc = CLANG if os.path.exists(CLANG) else "g++"
  flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
  subprocess.check_call([cc] + flags + ["-I" + SHIM, os.path.join(SHIM, "whatif_check.cpp"), "-o", out])
  return out


def pack_set(chars):
  return sum(ord(c) << (8 * k) for k, c in enumerate(chars))


def run_cases(exe, path, cases):
  """cases: dicts of board [rows, H, W], where [rows, 3], relative, impassable str, NA, q [rows, NA, D], chars [L], table, seen.
  -> per case (pos, tile, blocked, table, seen) as the program printed them."""
  blob = []
  for c in cases:
    rows, H, W = c["board"].shape
    D, L = c["q"].shape[-1], len(c["chars"])
    blob.append(struct.pack("<7q", H, W, c["NA"], rows, int(c["relative"]), D, L) + struct.pack("<Q", pack_set(c["impassable"])))
    blob.append(bytes(c["chars"]) + c["board"].astype(np.uint8).tobytes() + c["where"].astype(np.uint8).tobytes() +
                c["q"].astype(np.float64).tobytes() + c["table"].astype(np.float64).tobytes() + c["seen"].astype(np.uint8).tobytes())
  path.write_bytes(b"".join(blob))
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
  r = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
  assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
  lines = [[int(v) for v in l.split()] for l in r.stdout.splitlines()]
  out, at = [], 0
  for c in cases:
    rows, NA, D, L = c["board"].shape[0], c["NA"], c["q"].shape[-1], len(c["chars"])
    a = np.array(lines[at:at + rows], dtype=np.int64).reshape(rows, 4 * NA + L * D + L)
    at += rows
    out.append((a[:, :2 * NA].reshape(rows, NA, 2), a[:, 2 * NA:3 * NA], a[:, 3 * NA:4 * NA], a[:, 4 * NA:4 * NA + L * D].reshape(rows, L, D),
                a[:, 4 * NA + L * D:]))
  assert at == len(lines)
  return out


def expect(c):
  rows = c["board"].shape[0]
  flags = (c["where"][:, 2] << 1).astype(np.uint8)[:, None]
  pos, tile, blocked = R.simulate(c["board"], c["where"][:, None, :2], flags, c["relative"], [c["impassable"]], c["NA"])
  table, seen = c["table"].copy()[:, None], c["seen"].copy()[:, None]
  R.fold(tile, c["q"][:, None], c["chars"], table, seen)
  return pos[:, 0], tile[:, 0], blocked[:, 0], R.bits(table[:, 0]), seen[:, 0]


def check(exe, path, cases):
  for c, got in zip(cases, run_cases(exe, path, cases)):
    for name, g, w in zip(("target_pos", "target_tile", "blocked", "table", "seen"), got, expect(c)):
      assert np.array_equal(g, w.astype(np.int64)), "%s differs (%dx%d, %d actions, relative=%r)" % (name, c["board"].shape[1], c["board"].shape[2],
                                                                                                  c["NA"], c["relative"])


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_rows(exe, tmp_path, name):
  """Every step of the reference's run is one row; the table each row starts from is the reference's table of the step before."""
  fx, meta, _ = R.load_fixture(name)
  T = len(fx["frame"])
  chars = [ord(ch) for ch in meta["tile_types"] + [meta["agent_chr"]]]
  before = np.concatenate([np.zeros_like(fx["table"][:1]), fx["table"][:-1]])
  seen0 = np.concatenate([np.zeros_like(fx["seen"][:1]), fx["seen"][:-1]])
  c = dict(board=fx["board"], where=np.concatenate([fx["agent_pos"], np.full((T, 1), R.UP, np.uint8)], axis=1), relative=False,
           impassable=meta["impassable"], NA=fx["target_tile"].shape[1], q=fx["q"], chars=chars, table=before, seen=seen0)
  (pos, tile, blocked, table, seen), = run_cases(exe, tmp_path / "fx.bin", [c])
  assert np.array_equal(pos, fx["target_pos"]) and np.array_equal(tile, fx["target_tile"])
  assert np.array_equal(table, R.bits(fx["table"])) and np.array_equal(seen, fx["seen"])
  check(exe, tmp_path / "fx2.bin", [c])


def random_case(rng, H, W, NA, relative, D, rows=24):
  alphabet = np.frombuffer(b"# #WDF12S ", np.uint8)            # walls and blockers are common: most rows have a refused action
  board = alphabet[rng.integers(0, len(alphabet), size=(rows, H, W))]
  where = np.stack([rng.integers(0, H, rows), rng.integers(0, W, rows), rng.integers(0, 4, rows)], axis=1).astype(np.uint8)
  where[0] = (0, 0, R.LEFT); where[1] = (H - 1, W - 1, R.DOWN)  # corners: targets off the board on two sides
  where[2, 0] = H                                              # a position outside the board: reports itself, everything refused
  board[np.arange(rows), np.minimum(where[:, 0], H - 1), where[:, 1]] = ord('1')
  chars = [ord(ch) for ch in " WDF1"] + [0]                    # (tile 0 is what the off-board row reports)
  L = len(chars)
  q = rng.standard_normal((rows, NA, D)) * 10.0 ** rng.integers(-3, 7, size=(rows, NA, D))
  q[3] = -0.0                                                  # a mean of -0.0 stays -0.0: the sum starts from the first vector
  q[4, 0, 0] = np.nan
  q[5, :, 0] = np.inf
  return dict(board=board, where=where, relative=relative, impassable="#2S", NA=NA, q=q, chars=chars,
              table=rng.standard_normal((rows, L, D)), seen=rng.integers(0, 2, size=(rows, L)).astype(np.uint8))


def test_random_boards_every_action_count_and_direction(exe, tmp_path):
  rng = np.random.default_rng(7)
  cases = [random_case(rng, H, W, NA, relative, D) for (H, W) in ((1, 1), (3, 5), (6, 8), (13, 13)) for NA in range(1, 10)
           for relative, D in ((False, 1), (True, 3))]
  check(exe, tmp_path / "random.bin", cases)
  # the inputs do what they are for: refused actions that report another cell, relative envs that differ from absolute ones,
  # an untouched tile type that keeps its table row, a mean whose order of additions shows
  c = next(c for c in cases if c["relative"] and c["NA"] == 9 and c["board"].shape[1] == 6)
  pos, tile, blocked, table, seen = expect(c)
  assert (blocked.astype(bool) & (pos != c["where"][:, None, :2]).any(axis=-1)).any()
  absolute = R.simulate(c["board"], c["where"][:, None, :2], None, False, [c["impassable"]], 9)[0][:, 0]
  assert not np.array_equal(absolute, pos)
  untouched = ~np.array([[ch in row for ch in c["chars"]] for row in tile])
  assert untouched.any() and np.array_equal(table[untouched], R.bits(c["table"])[untouched]) and np.array_equal(seen[untouched], c["seen"][untouched])
  assert np.signbit(table.view(np.float64)[3][~untouched[3]]).all(), "a mean of -0.0 vectors is -0.0"


def test_the_order_of_the_additions_shows():
  """The restatement is sensitive to what it pins: adding the same vectors in another order changes the last bits somewhere."""
  rng = np.random.default_rng(3)
  q = rng.standard_normal((200, 1, 5, 1)) * 10.0 ** rng.integers(-3, 7, size=(200, 1, 5, 1))
  tile = np.full((200, 1, 5), 32, np.uint8)
  fwd, rev = np.zeros((200, 1, 1, 1)), np.zeros((200, 1, 1, 1))
  R.fold(tile, q, [32], fwd, np.zeros((200, 1, 1), np.uint8))
  R.fold(tile, q[:, :, ::-1], [32], rev, np.zeros((200, 1, 1), np.uint8))
  assert (R.bits(fwd) != R.bits(rev)).any()
