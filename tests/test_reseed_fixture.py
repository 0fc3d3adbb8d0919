"""A reseeding reset on the reference is "new stream, then an ordinary first reset": the fixture of tests/golden/
make_fixtures_reseed.py (island_navigation_ex_ma, map randomisation per episode, three envs; a segment from construction, one
after reset(options={"env_layout_seed": 2}), one after reset(env_layout_seed=3, seed=2**32 + 77 + e)) against the CPU oracle
started afresh, per segment, from numpy's PCG64(SeedSequence(seed of that segment)).

What the reference REPORTS as get_env_seed() after reset(seed=s) is s itself (safety_game_moma.py:708-709 stores the argument),
while the generator is seeded with s & 0xFFFFFFFF (safety_game_moma.py:859-864).  The fixture holds the reported value; the
stream comparison below pins the masked one."""
import zlib

import numpy as np

from oracle import oracle_ima as OI
from tests import golden_util as G

NAME = "reseed_ima_L10_rand3"
FIELDS = ["step_type", "reward", "cumulative", "discount", "term_reason", "frame", "board", "metrics", "pos",
          "action_direction", "observation_direction", "safety", "rng", "rng_has_uint32", "rng_uinteger", "view"]
M64 = (1 << 64) - 1


def numpy_words(seed):
  st = np.random.PCG64(np.random.SeedSequence(int(seed))).state["state"]
  return [st["state"] >> 64, st["state"] & M64, st["inc"] >> 64, st["inc"] & M64]


def layout_crc(original_seed, layout_seed):
  return zlib.crc32(b"".join(int(x).to_bytes(4, byteorder="big") for x in (original_seed, layout_seed, 17122023)))


def segment_seeds(E):
  """[E, 3]: the seed whose generator each segment of env e starts from."""
  return np.array([[2000 + e, layout_crc(2000 + e, 2), (2**32 + 77 + e) & 0xFFFFFFFF] for e in range(E)], dtype=np.int64)


def test_reported_env_seeds():
  fx, meta = G.load(NAME)
  E = int(meta["E"])
  assert fx["seeds"].tolist() == [2000 + e for e in range(E)]
  want = segment_seeds(E)
  assert fx["env_seed"][:, 0].tolist() == want[:, 0].tolist()
  assert fx["env_seed"][:, 1].tolist() == want[:, 1].tolist(), "crc32(2000 + e, 2, 17122023)"
  # reset(seed=s): get_env_seed() is the argument as given; its low 32 bits are the seed of the stream (next test)
  assert fx["env_seed"][:, 2].tolist() == [2**32 + 77 + e for e in range(E)]
  assert (fx["env_seed"][:, 2] & 0xFFFFFFFF).tolist() == want[:, 2].tolist()


def test_every_segment_is_a_fresh_stream_from_its_seed():
  fx, meta = G.load(NAME)
  E, T, SEG = int(meta["E"]), int(meta["T"]), int(meta["segments"])
  assert (E, SEG) == (3, 3) and fx["actions"].shape == (E, SEG, T, 2)
  cfg = OI.make_config(**meta["kwargs"])
  seeds = segment_seeds(E)
  firsts = set()
  for s in range(SEG):
    rng = np.array([numpy_words(seeds[e, s]) for e in range(E)], dtype=np.uint64)
    out = OI.run_streams(cfg, fx["actions"][:, s], rng)
    name = "%s.segment%d" % (NAME, s)
    # slot 0: the constructor's reset / the reseeding reset: the new stream draws the map
    G.assert_same(name + ".rng[0]", out["rng"][:, 0], fx["rng"][:, s, 0])
    G.assert_same(name + ".board[0]", out["board"][:, 0], fx["board"][:, s, 0])
    for f in FIELDS:
      G.assert_same(name + "." + f, out[f][:, 1:], fx[f][:, s, 1:])
      if s > 0 and f not in ("rng_has_uint32", "rng_uinteger"):      # the reseeding reset returns a whole timestep: the oracle's slot 0
        G.assert_same(name + "." + f + "[0]", out[f][:, 0], fx[f][:, s, 0])
    assert (out["reward_none"][:, 1:].astype(bool) == fx["reward_none"][:, s, 1:]).all()
    for e in range(E):
      firsts.add(fx["board"][e, s, 0].tobytes())
      assert (fx["step_type"][e, s, 2:] == 2).any(), "an episode ends inside every segment: the auto-reset draws from the new stream too"
  assert len(firsts) == E * SEG, "every reseeding reset drew a map of its own"
