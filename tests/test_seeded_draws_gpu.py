"""The seeded draws of every stochastic family against the C oracle, away from env id 0 (tests/seeded_draws.py: the tile
family's variant bit, safe_interruptibility's interruption bit, friend_foe's bandit-type and neutral-level draws, whisky_gold's
exploration and replacement draws, tomato_watering's drying draws; most rows straddle env id 2^32).  The host restates every
stream over the global env ids: philox.actions, LP.philox_uniforms, philox.episode_uniform against the spec's probability.

a. The rows and their groups through the launch-path matrix of tests/test_launch_paths_gpu.py (LP.run_path / LP.run_group:
   sgw_step, sgw_step_n direct / captured / replayed on the default and on a side stream, sgw_replay, sgw_rollout,
   sgw_group_step_n, sgw_group_rollout, the final state, read_returns).
b. sgw_fill_actions of an engine at base 2^32 - 500 == philox.actions over the global ids, and the in-kernel rollout stream ==
   that buffer (single-agent and firemaker_ex_ma, every agent).
c. Sharding invariance of every row of launch_paths.ROWS (at base 2^32 - 500) and of every row here: one engine of n envs ==
   two engines of n1 and n - n1 envs (neither a multiple of 64) at bases B and B + n1, array inputs sliced, seeded inputs with
   the same seed: every output, the state, the finished-episode count; the return sums up to the order of the atomic adds.  The
   whole engine also equals the oracle fed the restated streams, so three engines wrong in the same way do not pass."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import seeded_draws as SD
from tests.launch_paths import SEED, T

pytestmark = pytest.mark.gpu
BOUNDARY = SD.B32 - 500


def same_bytes(a, b):
  """Tensors equal byte for byte (NaN == NaN: the discount of a FIRST record)."""
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- a. every launch path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", LP.PATHS)
@pytest.mark.parametrize("row_id", [r["id"] for r in SD.ROWS])
def test_launch_path_matches_oracle(row_id, path):
  LP.run_path(SD.BY_ID[row_id], path)


@pytest.mark.parametrize("gid,members", SD.GROUPS, ids=[g for g, _ in SD.GROUPS])
def test_group_paths_match_oracle(gid, members):
  LP.run_group(gid, [SD.BY_ID[m] for m in members])


# ---- b. actions at the boundary --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ["island_ex_packed", "firemaker_ex_ma"])
def test_action_stream_across_the_id_boundary(row_id):
  row = LP.BY_ID[row_id]
  if row["n"] <= 500:
    row = dict(row, n=701)                            # (firemaker_ex_ma's 401 envs would end below 2^32)
  spec = make_spec(row["name"], **row["kw"])
  inp = LP.inputs(row, spec, 3)
  n, S, step0 = row["n"], 2 * T, 5
  ids = LP.global_ids(n, BOUNDARY)
  assert ids[0] < SD.B32 <= ids[-1]
  a, b = (LP.make_engine(row, spec, inp, base=BOUNDARY) for _ in range(2))
  acts = a.fill_actions(S, SEED, step0=step0)
  got = acts.cpu().numpy()
  for ag in range(spec.A):
    want = philox.actions(SEED, ids, step0 + np.arange(S), spec.action_lo, spec.n_actions, agent=ag)
    assert np.array_equal(got[..., ag] if spec.A > 1 else got, want), "%s: sgw_fill_actions of agent %d differs from philox.actions" % (row_id, ag)
  LP.start(a, row); LP.start(b, row)
  fed = {k: v.clone() for k, v in a.replay(acts, write_every=True).items()}
  own = b.rollout(S, SEED, step0=step0, write_every=True)
  for k in row["outs"]:
    assert same_bytes(fed[k], own[k]), "%s: %s of the rollout's own stream differs from the buffer's" % (row_id, k)
  assert torch.equal(a.get_state()[:, :n], b.get_state()[:, :n])
  a.close(); b.close()


# ---- c. sharding invariance ------------------------------------------------------------------------------------------------------------
ALL_ROWS = LP.ROWS + SD.ROWS


def split_at(n):
  n1 = 357 if n > 421 else n * 3 // 5
  assert n1 % 64 and (n - n1) % 64 and 0 < n1 < n
  return n1


def shard_inputs(inp, lo, hi):
  """Array inputs and generator words sliced to envs lo .. hi - 1; the seeds stay."""
  return {k: (v[lo:hi] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


def run_rollouts(row, spec, inp, base):
  """calls x rollout(T) from a reset: the outputs of every call, read_returns, the state [words, n]."""
  e = LP.make_engine(row, spec, inp, base=base)
  LP.start(e, row)
  calls = []
  for k in range(row["calls"]):
    o = e.rollout(T, SEED, step0=k * T, write_every=True, accumulate=True)
    calls.append({f: v.clone() for f, v in o.items()})
  ret, state = e.read_returns().clone(), e.get_state()[:, :row["n"]].clone()
  torch.cuda.synchronize()
  e.close()
  return calls, ret, state


@pytest.mark.parametrize("row_id", [r["id"] for r in ALL_ROWS])
def test_two_shards_equal_one_engine_and_the_oracle(row_id):
  row = SD.BY_ID[row_id] if row_id in SD.BY_ID else LP.BY_ID[row_id]
  base = row.get("base", BOUNDARY)
  n, S = row["n"], row["calls"] * T
  spec = make_spec(row["name"], **row["kw"])
  inp = LP.inputs(row, spec, row.get("seed", 7), base=base)
  whole, ret, state = run_rollouts(row, spec, inp, base)
  # the whole engine against the oracle, fed the streams restated over the global ids
  want = LP.run_oracle(row, LP.host_actions(spec, LP.global_ids(n, base), np.arange(S), SEED), inp)
  rec = {}
  for k, o in enumerate(whole):
    got = LP.to_np(o, True)
    views = LP.split_views(spec, got["views"]) if "views" in got else None
    bad = LP.oracle_mismatches(row, spec, got, want, 1 + k * T, views=views)
    assert not bad, "%s at base %d, rollout call %d differs from the oracle in %s" % (row_id, base, k, bad)
    for f in ("step_type", "cumulative"):
      rec.setdefault(f, []).append(got[f])
  if row["rng"]:
    assert not LP.rng_mismatch(row, state.cpu().numpy(), want, S), "%s: generator position after %d steps" % (row_id, S)
  if row["oracle"] == "scalar":
    st, cum = want["step_type"][..., None], want["cumulative"]
  else:                                              # (the engine's own arrays, which equal the oracle's: above)
    st, cum = (np.concatenate(rec[f], axis=1).reshape(n, S, -1) for f in ("step_type", "cumulative"))
    st, cum = (np.concatenate([np.zeros_like(x[:, :1]), x], axis=1) for x in (st, cum))      # record 0: the reset
  fin = LP.finished_returns(st, cum)
  assert fin[-1] > 0
  LP.check_returns(dict(row=row, returns={S: fin}), ret, S, "whole engine")
  # two shards
  n1 = split_at(n)
  parts = [run_rollouts(dict(row, n=hi - lo), spec, shard_inputs(inp, lo, hi), base + lo) for lo, hi in ((0, n1), (n1, n))]
  for k in range(row["calls"]):
    for f in row["outs"]:
      both = torch.cat([p[0][k][f] for p in parts], dim=1)
      assert same_bytes(both, whole[k][f]), "%s: %s of rollout call %d differs between one engine and two shards" % (row_id, f, k)
  assert torch.equal(torch.cat([p[2] for p in parts], dim=1), state), "%s: state differs between one engine and two shards" % row_id
  LP.check_returns(dict(row=row, returns={S: ret.cpu().numpy()}), parts[0][1] + parts[1][1], S, "two shards")
