"""sgw_policy_step_n against a host loop of act + step on forked engines: every output of every call, the action tapes and the
final state byte-equal, over the direct, captured and replayed paths (four identical calls; the capture threshold is T = 8), both
values of write_every, accumulate once; the tape against tests/policy_ref.py on the observations the host loop saw (weights are
rewritten in place before the fourth call: a captured graph holds pointers, not values); the tape replayed by step_n; a stale
capture after set_episode_bits; and a hand-written per-cell route on island_navigation_ex level 9 against the C oracle."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd.engine import ALL_OUTPUTS, BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import policy_gpu_util as U
from tests import policy_ref

pytestmark = pytest.mark.gpu

N_ENVS = 65
BASE = (1 << 32) + 11
CALLS = 4


def start(name, kw, source, outs=None):
  spec = make_spec(name, **kw)
  eng = BatchedEngine(spec, N_ENVS, device=U.DEV, env_id_base=BASE, outputs=outs or U.outputs_for(spec, source))
  if name in U.GENERATOR_ENVS:
    eng.seed_rng(base=7)
  eng.reset()
  return spec, eng


def twin_policy(eng, src):
  """A second TablePolicy with the same tables and its own step counter."""
  p = TablePolicy(eng, source=src.source, chars=src.chars, n_policies=src.n_policies, seed=src.seed)
  p.explore_below = src.explore_below
  p.weights.copy_(src.weights); p.bias.copy_(src.bias)
  if src.policy_of_env is not None:
    p.set_policy_of_env(src.policy_of_env.clone())
  return p


def snapshot(res):
  return {k: v.cpu().numpy().copy() for k, v in res.items()}


def host_loop(eng, pol, T, accumulate):
  """T x (act, step) from Python; returns ([T] list of output snapshots, tape [T, N, A], the observations each act read)."""
  outs, tape, seen = [], [], []
  for t in range(T):
    seen.append(eng._bufs[pol.source].cpu().numpy()[:eng.n_envs].copy())
    a = eng.act(pol, t=t)
    tape.append(a.cpu().numpy().copy())
    outs.append(snapshot(eng.step_n(a.reshape((1,) + tuple(a.shape)), accumulate=accumulate)))
  pol.step += T
  return outs, np.stack(tape), seen


def run_twins(name, kw, source, T, write_every, between=None, calls=CALLS, epsilon=0.25):
  spec, eng = start(name, kw, source)
  rng = np.random.default_rng(T * 2 + int(write_every))
  polA = TablePolicy(eng, source=source, chars=list(spec.layer_chars) + [U.WIN], n_policies=3, seed=17, epsilon=epsilon)
  tables = [U.fill_policy(polA, rng, mixed=True)]
  A, B, R = eng.fork(), eng.fork(), eng.fork()
  polB = twin_policy(B, polA)
  record = dict(A=[], B=[], tapeA=[], tapeB=[], seen=[], tables=[])
  for call in range(calls):
    if call == 3:                                      # in place, after the capture: the replay must see the new tables
      w, b, _ = U.fill_policy(polA, rng, mixed=False, with_index=False)
      polB.weights.copy_(polA.weights); polB.bias.copy_(polA.bias)
      tables.append((w, b, tables[0][2]))
    if between is not None:
      between(call, (A, B, R))
    acc = call == 1
    resA = snapshot(A.policy_step_n(polA, T, write_every=write_every, accumulate=acc))
    outsB, tapeB, seen = host_loop(B, polB, T, acc)
    tapeA = resA.pop("actions")
    assert tapeA.shape == (T, N_ENVS, spec.A)
    assert (tapeA == tapeB).all(), "call %d: action tapes differ" % call
    for k in resA:
      wantB = np.stack([o[k] for o in outsB]) if write_every else outsB[-1][k]
      assert LP._same(resA[k].reshape(wantB.shape), wantB), "call %d: output %r differs from the host loop" % (call, k)
    # A's tape through step_n on a third fork reproduces A's outputs
    resR = snapshot(R.step_n(torch.from_numpy(tapeA).to(U.DEV), write_every=True))
    for k, v in resA.items():
      want = resR[k] if (write_every or T == 1) else resR[k][-1]           # (T == 1: plain [N, ...] buffers either way)
      assert LP._same(v.reshape(want.shape), want), "call %d: output %r differs from step_n over the tape" % (call, k)
    record["A"].append(resA); record["tapeA"].append(tapeA); record["seen"].append(seen); record["tables"].append(tables[-1])
  assert int(polA.step.item()) == calls * T == int(polB.step.item())
  assert torch.equal(A.get_state(), B.get_state())
  assert torch.equal(A.read_returns(), B.read_returns())
  assert torch.equal(A.get_state(), R.get_state())
  for e in (eng, A, B, R):
    e.close()
  return polA, record


@pytest.mark.parametrize("write_every", [False, True])
@pytest.mark.parametrize("T", [1, 7, 8, 9])
@pytest.mark.parametrize("geo", sorted(U.GEOMETRIES))
def test_closed_loop_equals_the_host_loop(geo, T, write_every):
  name, kw, source = U.GEOMETRIES[geo]
  polA, rec = run_twins(name, kw, source, T, write_every)
  # the tape is what the numpy statement chooses on the observations each step saw, before and after the tables were rewritten
  changed = 0
  for call in range(CALLS):
    w, b, idx = rec["tables"][call]
    for t in range(T):
      want = U.ref_actions(polA, rec["seen"][call][t], w, b, idx, BASE, call * T + t)
      assert (rec["tapeA"][call][t] == want).all(), "call %d step %d" % (call, t)
      if call == 3:
        w0, b0, _ = rec["tables"][0]
        changed += int((U.ref_actions(polA, rec["seen"][call][t], w0, b0, idx, BASE, call * T + t) != want).sum())
  assert changed > 0, "the rewritten tables choose differently somewhere: the fourth call did not run the old ones"


def test_always_exploring_is_the_philox_stream():
  T = 8
  polA, rec = run_twins("island_navigation_ex", dict(level=9), "board", T, False, epsilon=1.0)
  assert polA.explore_below == 1 << 32
  ids = BASE + np.arange(N_ENVS)
  idx = rec["tables"][0][2]
  for s in range(CALLS * T):
    want = polA.action_lo + policy_ref.explore(np.zeros(N_ENVS, np.int64), polA.n_actions, 1 << 32, polA.seed, ids, s, 0)
    want = np.where((idx >= 0) & (idx < polA.n_policies), want, 0)
    assert (rec["tapeA"][s // T][s % T][:, 0] == want).all(), "step %d" % s


def test_a_setter_between_calls_makes_the_capture_stale():
  """safe_interruptibility draws should_interrupt per episode from (seed, env id): set_episode_bits bumps the engine's argument
  epoch, so the captured chain (which holds the old seed in its step launches) must not be replayed."""
  def between(call, engines):
    if call == 3:
      for e in engines:
        e.set_episode_bits(None, seed=5)
  run_twins("safe_interruptibility", dict(max_iterations=6), "board", 8, True, between=between, calls=6)


def test_per_cell_route_against_the_oracle():
  """island_navigation_ex level 9: up from the start, along the top row over the drink tile, down to the gold G, and one step
  further into the water, which ends the episode with TERMINATED (checked on the oracle alone: the gold tile itself does not).
  The closed loop must produce that route in every env and the oracle's outputs for it."""
  from oracle import oracle as O
  name, kw, T = "island_navigation_ex", dict(level=9), 24
  spec = make_spec(name, **kw)
  W = spec.W
  table = np.zeros(spec.H * W, np.int64)                       # 0 noop, 1 left, 2 right, 3 up, 4 down
  for (r, c), a in {(2, 2): 3, (1, 2): 2, (1, 3): 2, (1, 4): 2, (1, 5): 4, (2, 5): 4, (3, 5): 2, (3, 6): 2}.items():
    table[r * W + c] = a
  route = [3, 2, 2, 2, 4, 4, 2, 2]
  alone = O.run_streams(O.make_config(name, **kw), np.array([route], np.int8))
  assert alone["step_type"][0, len(route)] == 2 and alone["term_reason"][0, len(route)] == 0, "the route ends TERMINATED on the oracle"
  eng = BatchedEngine(spec, N_ENVS, device=U.DEV, env_id_base=BASE, outputs=ALL_OUTPUTS)
  pol = TablePolicy.from_cell_actions(eng, table)
  first = snapshot(eng.reset())
  res = snapshot(eng.policy_step_n(pol, T, write_every=True))
  tape = res.pop("actions")
  assert (tape[:len(route), :, 0] == np.array(route)[:, None]).all()
  assert (tape[len(route) + 1:2 * len(route) + 1, :, 0] == np.array(route)[:, None]).all(), "after the auto-reset the route starts over"
  row = dict(oracle="scalar", name=name)
  want = O.run_streams(O.make_config(name, **kw), np.ascontiguousarray(np.moveaxis(tape[:, :, 0], 0, 1)), nthreads=16)
  got = {k: np.moveaxis(v, 0, 1) for k, v in res.items()}
  assert LP.oracle_mismatches(row, spec, got, want, 1) == []
  assert LP.oracle_mismatches(row, spec, {k: v[:, None] for k, v in first.items()}, want, 0) == []
  tr = res["term_reason"]
  assert (tr[len(route) - 1] == 0).all() and (res["step_type"][len(route) - 1] == 2).all(), "TERMINATED inside T steps"
  eng.close()
