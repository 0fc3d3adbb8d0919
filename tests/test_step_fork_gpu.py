"""The forked headline step kernel (k_step_fork: a state wave and an output wave per env-wave, csrc/sgw_kernels.hpp) against the C
oracle and against the one-wave kernel it replaces (SGW_NO_FORK set at sgw_create), bit for bit.

Sizes: N = 1 (one ragged wave), 65 (a second wave), 129 and 257 (a last workgroup with live and dead env-waves when a workgroup
holds two / four env-waves).  Tapes and oracle are those of tests/test_headline_prologue_gpu.py: the scripted tape holds the step
where drink and food regrow together.  Paths: sgw_step per step; three identical sgw_step_n calls (direct, capture, replay) with
write_every and accumulate.  Every output of FIELDS, metrics included, is compared with the oracle, the returns exactly; outputs,
exported state and returns are the same bytes on both kernels.

Output subsets at N = 129, each buffer inside guard bytes (tests/output_subsets.py): the bench set, each field alone (`metrics`
alone makes the output wave run the regrowth, `cumulative` alone is the one reader of the running sums), and none at all (state and
returns only).

The selection by size: an engine of 4 x CUs x 64 envs forks, one of 4 x CUs x 64 + 64 does not and still equals SGW_NO_FORK; both
default-selected engines are compared with the oracle over 8 steps of the bench output set.

The features (masked resets, QUIT, the packed state at its limit, ragged returns, the closed loop, copy / fork / lookahead, the
facades) on this kernel and on the other three: tests/test_headline_kernels_gpu.py."""
import numpy as np
import pytest

from tests.test_headline_prologue_gpu import FIELDS, _returns, _same, oracle, regrowth_events

pytestmark = pytest.mark.gpu

NS = (1, 65, 129, 257)
BENCH_OUTPUTS = ("board", "reward", "step_type", "term_reason", "safety", "frame")    # bench.py's headline output set
SUBSETS = [("bench", BENCH_OUTPUTS)] + [(f, (f,)) for f in FIELDS] + [("none", ())]
KERNELS = ((None, 1), ("SGW_NO_FORK", 0))                                              # env at sgw_create, sgw_step_fork


def _engine(cls, n, env, outputs, monkeypatch):
  from ai_safety_gridworlds_amd import _native as N
  from ai_safety_gridworlds_amd.specs import make_spec
  if env:
    monkeypatch.setenv(env, "1")
  try:
    eng = cls(make_spec("island_navigation_ex"), n, device="cuda:0", outputs=tuple(outputs))
  finally:
    if env:
      monkeypatch.delenv(env, raising=False)
  assert (N.lib().sgw_step_rules(eng._h), N.lib().sgw_step_shape(eng._h)) == (1, 1)
  return eng


def _compare(got, want, s0, n, fields, label):
  """got {field: [S, n_pad, ...]} device tensors = steps s0 .. s0 + S - 1 of the oracle's record"""
  for k in fields:
    g = np.moveaxis(got[k].cpu().numpy()[:, :n], 0, 1)
    w = want[k][:, s0:s0 + g.shape[1]]
    if k == "term_reason":
      g = g.astype(np.int16); g[g == 255] = -1
    if k == "metrics":
      g = g[..., :w.shape[-1]]
    assert _same(g.reshape(w.shape), w), "%s: %s differs from the oracle in steps %d..%d" % (label, k, s0, s0 + g.shape[1] - 1)


def _step_n_run(cls, n, env, fork, outputs, acts, want, T, calls, monkeypatch):
  """-> ([per call {field: tensor}], returns, state[:, :n]) of `calls` identical sgw_step_n calls, each checked against the oracle"""
  import torch
  from ai_safety_gridworlds_amd import _native as N
  label = "sgw_step_n" + (" with " + env if env else "")
  eng = _engine(cls, n, env, outputs, monkeypatch)
  assert N.lib().sgw_step_fork(eng._h) == fork, label
  eng.reset()
  buf = torch.from_numpy(acts[:T]).to("cuda:0")
  recs = []
  for call in range(calls):
    got = {k: v.clone() for k, v in eng.step_n(buf, write_every=True, accumulate=True).items()}
    _compare(got, want, 1 + call * T, n, outputs, "%s call %d" % (label, call))
    recs.append({k: v[:, :n] for k, v in got.items()})
  r, w = eng.read_returns().cpu().numpy(), _returns(want, calls * T)
  assert np.array_equal(r, w), "%s: returns %s, the oracle's %s" % (label, r, w)
  state = eng.get_state()[:, :n].clone()
  if hasattr(eng, "guards_intact"):
    assert eng.guards_intact() == [], label
  eng.close()
  return recs, r, state


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["philox", "script"])
def test_fork_matches_the_oracle_and_the_one_wave_kernel(kind, n, monkeypatch):
  import torch
  from ai_safety_gridworlds_amd import _native as N
  from ai_safety_gridworlds_amd.engine import BatchedEngine
  acts, want = oracle(kind, n)
  T = (len(acts) - 16) // 3
  if kind == "script":
    both, limit, one = regrowth_events(want)
    assert both[:, :T].any() and limit[:, :T].any() and one[:, :T].any()
  dev = torch.from_numpy(acts).to("cuda:0")
  per_kernel = []
  for env, fork in KERNELS:
    # sgw_step, one call per step
    eng = _engine(BatchedEngine, n, env, FIELDS, monkeypatch)
    assert N.lib().sgw_step_fork(eng._h) == fork
    rec = {k: [v.clone()] for k, v in eng.reset().items()}
    for t in range(3 * T):
      for k, v in eng.step(dev[t]).items():
        rec[k].append(v.clone())
    rec = {k: torch.stack(v) for k, v in rec.items()}
    _compare(rec, want, 0, n, FIELDS, "sgw_step" + (" with " + env if env else ""))
    state = eng.get_state()[:, :n].clone()
    eng.close()
    # three identical sgw_step_n calls: direct launches, capture, replay
    recs, r, state_n = _step_n_run(BatchedEngine, n, env, fork, FIELDS, acts, want, T, 3, monkeypatch)
    assert w_any(r) or n == 1, "no episode ends inside the run"
    assert torch.equal(state, state_n), "the exported state differs between sgw_step and sgw_step_n"
    per_kernel.append(({k: v[:, :n] for k, v in rec.items()}, recs, r, state))
  (rec_f, recs_f, r_f, st_f), (rec_o, recs_o, r_o, st_o) = per_kernel
  for k in FIELDS:
    assert _same_bytes(rec_f[k], rec_o[k]), "sgw_step: %s differs between the two kernels" % k
    for call, (a, b) in enumerate(zip(recs_f, recs_o)):
      assert _same_bytes(a[k], b[k]), "sgw_step_n call %d: %s differs between the two kernels" % (call, k)
  assert np.array_equal(r_f, r_o) and torch.equal(st_f, st_o)


def _same_bytes(a, b):
  import torch
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def w_any(r):
  return r[-1] > 0          # the episode count of the returns row


@pytest.mark.parametrize("name,outputs", SUBSETS, ids=[s[0] for s in SUBSETS])
def test_output_subsets_inside_guard_bytes(name, outputs, monkeypatch):
  import torch
  from tests.output_subsets import GuardedEngine
  n = 129
  acts, want = oracle("script", n)
  T = (len(acts) - 16) // 3
  runs = [_step_n_run(GuardedEngine, n, env, fork, outputs, acts, want, T, 3, monkeypatch) for env, fork in KERNELS]
  (recs_f, r_f, st_f), (recs_o, r_o, st_o) = runs
  for call, (a, b) in enumerate(zip(recs_f, recs_o)):
    assert sorted(a) == sorted(outputs)
    for k in outputs:
      assert _same_bytes(a[k], b[k]), "call %d: %s differs between the two kernels" % (call, k)
  assert np.array_equal(r_f, r_o) and torch.equal(st_f, st_o)
  assert r_f[-1] > 0


def test_the_selection_by_size(monkeypatch):
  """At most one env-wave per SIMD forks; one env-wave more keeps the one-wave kernel, which SGW_NO_FORK also selects.  On both
  sides of the edge the default-selected engine's 8 recorded steps of the bench output set equal the C oracle's on the same
  Philox tape: 4 x CUs x 64 envs is the largest forked grid (its last workgroup runs nowhere else), 64 envs more the one size
  at which the default selection launches the one-wave kernel with its real grid.  66 067 episodes end inside the 8 steps.
  The oracle takes 0.4 s for the 65 600 envs x 8 steps of a 256-CU part (16 threads on 8 cores; 0.5 s with one thread), the
  whole test 0.7 s on the MI355X's host."""
  import torch
  from ai_safety_gridworlds_amd import _native as N, philox
  from ai_safety_gridworlds_amd.engine import BatchedEngine
  from oracle import oracle as O
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  edge = 4 * cus * 64
  n, steps = edge + 64, 8
  host = philox.actions(0xF02C, np.arange(n, dtype=np.uint64), np.arange(steps, dtype=np.uint64), 0, 5).astype(np.int8)
  want = O.run_streams(O.make_config("island_navigation_ex"), host.T.copy(), fields=list(BENCH_OUTPUTS), nthreads=16)
  acts = torch.from_numpy(host).to("cuda:0")

  def play(eng):
    eng.reset()
    return [{k: v.clone() for k, v in eng.step(acts[t, :eng.n_envs].contiguous()).items()} for t in range(steps)]

  def against_the_oracle(rec, m, label):
    _compare({k: torch.stack([r[k] for r in rec]) for k in BENCH_OUTPUTS}, {k: want[k][:m] for k in BENCH_OUTPUTS}, 1, m, BENCH_OUTPUTS, label)

  eng = _engine(BatchedEngine, edge, None, BENCH_OUTPUTS, monkeypatch)
  assert N.lib().sgw_step_fork(eng._h) == 1
  against_the_oracle(play(eng), edge, "the fork at %d envs" % edge)          # (env e's tape does not depend on the batch size)
  eng.close()
  got = []
  for env in (None, "SGW_NO_FORK"):
    eng = _engine(BatchedEngine, n, env, BENCH_OUTPUTS, monkeypatch)
    assert N.lib().sgw_step_fork(eng._h) == 0
    rec = play(eng)
    if env is None:
      against_the_oracle(rec, n, "the default selection at %d envs" % n)
    got.append((rec, eng.get_state().clone()))
    eng.close()
  (rec_a, st_a), (rec_b, st_b) = got
  assert torch.equal(st_a, st_b)
  for t in range(steps):
    for k in BENCH_OUTPUTS:
      assert _same_bytes(rec_a[t][k], rec_b[t][k]), (t, k)
