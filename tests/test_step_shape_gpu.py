"""The one-step kernel with the output geometry compiled in (csrc/sgw_kernels.hpp StepShape, picked by sgw_create:
sgw_step_shape) against the generic kernel (SGW_GENERIC_STEP set at sgw_create) on the same inputs: every output, the
state and the episodic-return accumulators byte for byte.  Specs outside the shape table take the generic kernel and still
match the oracle.  The CPU test checks that the shaped kernel is in the build and keeps everything in registers."""
import os
import re

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine, ALL_OUTPUTS
from ai_safety_gridworlds_amd.specs import make_spec

BENCH_OUTPUTS = ("board", "reward", "step_type", "term_reason", "safety", "frame")    # bench.py's headline output set
SHAPED_PREFIX = "_ZN3sgw8k_engineINS_7IslandTILb0ELb1EEELi0ENS_9StepShapeILi6ELi8ELi10E"   # k_engine<IslandPacked, K_STEP, StepShape<6, 8, 10, ...>>


def _engine(spec, n, outputs, generic, monkeypatch):
  if generic:
    monkeypatch.setenv("SGW_GENERIC_STEP", "1")
  try:
    return BatchedEngine(spec, n, device="cuda:0", outputs=outputs)
  finally:
    monkeypatch.delenv("SGW_GENERIC_STEP", raising=False)


def _bytes(t):
  return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def _run(spec, n, outputs, generic, write_every, accumulate, monkeypatch, seed=0x5EED):
  """sgw_step_n calls (the first slice four times: captured and replayed as a hipGraph), a run of distinct slices and
  single sgw_step calls: 245 steps; returns (kernel shape, recorded output bytes, state, returns)."""
  eng = _engine(spec, n, outputs, generic, monkeypatch)
  shape = int(N.lib().sgw_step_shape(eng._h))
  rec = [{k: _bytes(v) for k, v in eng.reset().items()}]
  acts = eng.fill_actions(95, seed)                     # [T, N] int8 on the device
  calls = [acts[0:50]] * 4 + [acts[50:70], acts[70:90]]
  for a in calls:
    rec.append({k: _bytes(v) for k, v in eng.step_n(a, write_every=write_every, accumulate=accumulate).items()})
  for t in range(90, 95):
    rec.append({k: _bytes(v) for k, v in eng.step(acts[t]).items()})
  torch.cuda.synchronize()
  state = _bytes(eng.get_state())
  returns = _bytes(eng.read_returns())
  eng.close()
  return shape, rec, state, returns


CASES = [
    (1000, BENCH_OUTPUTS, False, True),       # n_envs not a multiple of 64 (nor 256)
    (1000, ALL_OUTPUTS, True, True),
    (4160, BENCH_OUTPUTS, True, False),       # a multiple of 64, not of 256: the last workgroup holds one env-wave
    (4160, ALL_OUTPUTS, False, True),
    (65536, BENCH_OUTPUTS, False, True),      # the headline size
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,outputs,write_every,accumulate", CASES)
def test_shaped_step_kernel_equals_generic(n, outputs, write_every, accumulate, monkeypatch):
  spec = make_spec("island_navigation_ex")
  s_shape, s_rec, s_state, s_ret = _run(spec, n, outputs, False, write_every, accumulate, monkeypatch)
  g_shape, g_rec, g_state, g_ret = _run(spec, n, outputs, True, write_every, accumulate, monkeypatch)
  assert s_shape == 1 and g_shape == 0
  assert len(s_rec) == len(g_rec)
  for i, (s, g) in enumerate(zip(s_rec, g_rec)):
    for k in outputs:
      assert np.array_equal(s[k], g[k]), "call %d, output %s differs between the shaped and the generic kernel" % (i, k)
  assert np.array_equal(s_state, g_state), "state differs"
  assert np.array_equal(s_ret, g_ret), "return accumulators differ"
  if accumulate:
    assert s_ret.view(np.float64)[-1] > 0              # episodes did end inside the run


UNSHAPED = [
    ("level 5 (5 x 5 board)", dict(level=5), False),
    ("GOLD_REWARD zero: K = 9 on the level-9 board", dict(GOLD_REWARD={"GOLD_REWARD": 0}), False),
    ("plain f64 state", {}, True),
    ("per-event reward vectors (F_GENERAL)", dict(DRINK_REWARD={"DRINK_REWARD": 2.0, "FOOD_REWARD": -1.0}), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("what,kw,plain", UNSHAPED, ids=[u[0] for u in UNSHAPED])
def test_spec_outside_the_table_runs_generic_and_matches_oracle(what, kw, plain, monkeypatch):
  from oracle import oracle as O
  if plain:
    monkeypatch.setenv("SGW_ISLAND_PLAIN_STATE", "1")
  E, T, seed = 700, 120, 0xC0DE
  spec = make_spec("island_navigation_ex", **kw)
  actions = philox.actions(seed, np.arange(E), np.arange(T), 0, 5)          # [T, E]
  fields = ["board", "reward", "cumulative", "step_type", "term_reason", "safety"]
  want = O.run_streams(O.make_config("island_navigation_ex", **kw), actions.T.copy(), fields=fields)
  eng = BatchedEngine(spec, E, device="cuda:0", outputs=tuple(fields))
  assert N.lib().sgw_step_shape(eng._h) == 0, what
  if plain:
    assert N.lib().sgw_state_words(eng._h) == 22
  eng.reset()
  got = eng.step_n(torch.from_numpy(actions).to("cuda:0"), write_every=True)
  for k in fields:
    g = got[k].cpu().numpy()                                    # [T, N_pad, ...]
    g = g[:, :E]
    w = np.moveaxis(want[k][:, 1:], 0, 1).reshape(g.shape)
    if k == "term_reason":
      g = g.astype(np.int16); g[g == 255] = -1
    assert np.array_equal(g, w), "%s: %s differs from the oracle" % (what, k)
  eng.close()


def test_shaped_kernel_is_built_without_scratch():
  """CPU: the shaped one-step kernel is in the installed build, with no scratch memory (so no VGPR spills) and no SGPR
  spills to VGPR lanes (v_writelane / v_readlane)."""
  if not os.path.exists("/opt/rocm/bin/hipcc"):
    pytest.skip("hipcc not present")
  from ai_safety_gridworlds_amd import build as B
  B.build()
  if not os.path.exists(B.ASM) or os.path.getmtime(B.ASM) < max(os.path.getmtime(d) for d in B._deps()):
    B.build(force=True)
  asm = open(B.ASM).read()
  names = sorted(set(re.findall(r"^(%s\w*):" % SHAPED_PREFIX, asm, re.M)))
  assert len(names) == 1, names
  k = names[0]
  assert re.search(r"\.set %s\.private_seg_size, 0$" % re.escape(k), asm, re.M), "the shaped kernel uses scratch memory"
  body = asm[asm.index(k + ":"):]
  body = body[:body.index(".Lfunc_end")]
  assert not re.search(r"^\s+v_(writelane|readlane)_b32", body, re.M), "the shaped kernel spills SGPRs"
