"""The headline's one-step kernels with level 9's default rule set compiled in (csrc/sgw_island.hpp IslandL9Default, picked by
sgw_create: sgw_step_rules) -- the forked kernel, which the default selection runs at every size used here (sgw_step_fork), and
the one-wave kernel (SGW_NO_FORK set at sgw_create) -- against the shape-only kernel (SGW_GENERIC_RULES) and the generic kernel
(SGW_GENERIC_STEP) on the same inputs: every output, the state and the episodic-return accumulators byte for byte.  Then
against the C oracle, with QUIT and out-of-range actions in the tape; specs one flag or one parameter away from the compiled
one take the shape-only kernel and still match the oracle."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine, ALL_OUTPUTS
from ai_safety_gridworlds_amd.specs import make_spec
from tests import headline_kernels as HK

pytestmark = pytest.mark.gpu

BENCH_OUTPUTS = ("board", "reward", "step_type", "term_reason", "safety", "frame")    # bench.py's headline output set
ORACLE_FIELDS = ["board", "reward", "cumulative", "step_type", "term_reason", "safety"]
KERNELS = tuple((k["id"], k["env"]) + k["triple"] for k in HK.KERNELS)    # name, env at sgw_create, step_rules, step_shape, step_fork
assert KERNELS[0] == ("fork", None, 1, 1, 1) and ("shape_only", "SGW_GENERIC_RULES", 0, 1, 0) in KERNELS and ("generic", "SGW_GENERIC_STEP", 0, 0, 0) in KERNELS


def tape(seed, n, steps):
  """int8 [steps, n]: the project's Philox action stream in 0..4 with a seeded 2 % (agent stream 1 of the same generator)
  replaced by QUIT / out-of-range values -- the recipe of tests/host_shim/island_rules_check.cpp."""
  ids, ts = np.arange(n, dtype=np.uint64), np.arange(steps, dtype=np.uint64)
  base = philox.actions(seed, ids, ts, 0, 5)
  x0, x1, _, _ = philox.philox4x32_10(ts[:, None], philox.TAG_ACTION, 1, 0, seed, ids[None, :])
  odd = np.array([9, -1, 5, 10, 127], np.int8)
  return np.where(x0 % 50 == 0, odd[x1 % 5], base).astype(np.int8)


def _engine(spec, n, outputs, env, monkeypatch):
  if env:
    monkeypatch.setenv(env, "1")
  try:
    return BatchedEngine(spec, n, device="cuda:0", outputs=outputs)
  finally:
    if env:
      monkeypatch.delenv(env, raising=False)


def _bytes(t):
  return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def _run(spec, n, outputs, env, write_every, acts, monkeypatch):
  """The call pattern of tests/test_step_shape_gpu.py: a 50-step sgw_step_n slice four times (first sighting, capture,
  replays), two distinct 20-step slices, five single sgw_step calls; accumulate=True.  Returns ((step_rules, step_shape,
  step_fork), recorded output bytes, state, returns)."""
  eng = _engine(spec, n, outputs, env, monkeypatch)
  triple = HK.triple_of(eng)
  rec = [{k: _bytes(v) for k, v in eng.reset().items()}]
  for a in [acts[0:50]] * 4 + [acts[50:70], acts[70:90]]:
    rec.append({k: _bytes(v) for k, v in eng.step_n(a, write_every=write_every, accumulate=True).items()})
  for t in range(90, 95):
    rec.append({k: _bytes(v) for k, v in eng.step(acts[t]).items()})
  torch.cuda.synchronize()
  state, returns = _bytes(eng.get_state()), _bytes(eng.read_returns())
  eng.close()
  return triple, rec, state, returns


CASES = [
    (1000, BENCH_OUTPUTS, False),       # a ragged end: n_envs not a multiple of 64
    (1000, ALL_OUTPUTS, True),
    (4160, BENCH_OUTPUTS, False),       # a multiple of 64, not of 256: the last workgroup holds one env-wave
]


@pytest.mark.parametrize("n,outputs,write_every", CASES)
def test_three_kernels_compute_the_same_bytes(n, outputs, write_every, monkeypatch):
  """(Four since the forked kernel: the two with compiled rules, the shape-only one and the generic one.)"""
  spec = make_spec("island_navigation_ex")
  acts = torch.from_numpy(tape(0x5EED, n, 95)).to("cuda:0")
  runs = [_run(spec, n, outputs, k[1], write_every, acts, monkeypatch) for k in KERNELS]
  for k, (triple, _, _, _) in zip(KERNELS, runs):
    assert triple == k[2:], k[0]
  _, rec0, state0, ret0 = runs[0]
  for (name, _, _, _, _), (_, rec, state, ret) in list(zip(KERNELS, runs))[1:]:
    assert len(rec) == len(rec0)
    for i, (s, g) in enumerate(zip(rec0, rec)):
      for k in outputs:
        assert np.array_equal(s[k], g[k]), "call %d, output %s differs between the rules kernel and the %s kernel" % (i, k, name)
    assert np.array_equal(state0, state), "state differs from the %s kernel's" % name
    assert np.array_equal(ret0, ret), "return accumulators differ from the %s kernel's" % name
  assert ret0.view(np.float64)[-1] > 0                 # episodes did end inside the run


def _against_oracle(what, kw, want_rules, want_shape):
  from oracle import oracle as O
  E, T, seed = 700, 120, 0xC0DE
  spec = make_spec("island_navigation_ex", **kw)
  actions = tape(seed, E, T)                                             # [T, E]
  want = O.run_streams(O.make_config("island_navigation_ex", **kw), actions.T.copy(), fields=ORACLE_FIELDS)
  eng = BatchedEngine(spec, E, device="cuda:0", outputs=tuple(ORACLE_FIELDS))
  assert N.lib().sgw_step_rules(eng._h) == want_rules, what
  assert N.lib().sgw_step_fork(eng._h) == want_rules, "%s: at %d envs the default selection forks wherever it compiles the rules in" % (what, E)
  if want_shape is not None:
    assert N.lib().sgw_step_shape(eng._h) == want_shape, what
  eng.reset()
  got = eng.step_n(torch.from_numpy(actions).to("cuda:0"), write_every=True)
  for k in ORACLE_FIELDS:
    g = got[k].cpu().numpy()[:, :E]                                      # [T, N_pad, ...]
    w = np.moveaxis(want[k][:, 1:], 0, 1).reshape(g.shape)
    if k == "term_reason":
      g = g.astype(np.int16); g[g == 255] = -1
    assert np.array_equal(g, w), "%s: %s differs from the oracle" % (what, k)
  assert (want["term_reason"][:, 1:] == 3).any(), "no episode of the tape ends with QUIT"
  eng.close()


@pytest.mark.parametrize("kw", [{}, dict(max_iterations=5)], ids=["default", "max_iterations 5"])
def test_rules_kernel_matches_oracle(kw):
  _against_oracle("compiled rules", kw, 1, 1)


NEAR_MISSES = [      # (the last two: whichever kernel their reward columns select)
    ("DRINK_REWARD 25", dict(DRINK_REWARD={"DRINK_REWARD": 25}), 1),
    ("sustainability_challenge off", dict(sustainability_challenge=False), 1),
    ("penalise_oversatiation off", dict(penalise_oversatiation=False), None),
    ("satiation-proportional reward", dict(use_satiation_proportional_reward=True), None),
]


@pytest.mark.parametrize("what,kw,shape", NEAR_MISSES, ids=[m[0] for m in NEAR_MISSES])
def test_near_miss_runs_without_compiled_rules_and_matches_oracle(what, kw, shape):
  _against_oracle(what, kw, 0, shape)
