"""read_returns() at ragged batch sizes against the C oracle's finished-episode sums and count.

The returns transpose (csrc/sgw_kernels.hpp accumulate_returns) reads all 64 staged rows of an env-wave without a per-row
guard: a lane that is not a real env (the padding up to the next multiple of 64; it steps with action 0 and ends episodes at
max_iterations like any other) stages exact zeros.  A padded lane that leaked into the sums would show in the episode count
first, so every case ends episodes in every env (max_iterations = 5 over 24 steps) and asserts the count exactly.

Cases: 1, 63, 65 and 129 envs (a lone lane, a ragged only wave, a ragged wave behind one and behind two full ones) of
island_navigation_ex level 9 (the shaped one-step kernel, and the generic one: SGW_GENERIC_STEP at sgw_create), boat_race_ex
level 3, island_navigation_ex_ma (2K + 1 = 17 columns: the second pass of the transpose) and firemaker_ex_ma (the cooperative
leader wave), each through one-step launches, sgw_step_n three times over one buffer (direct launches, capture, replay) and the
fused sgw_rollout.  These rewards are integers, so the sums are exact in any order: equality is asserted.

The fractional case (MOVEMENT_REWARD = -0.3: the plain island state) pins the ASSOCIATION of the device's sums bit for bit:
per launch a tree over each 16-row part -- pairs (j, j + 8), (j, j + 4), (j, j + 2), (j, j + 1) -- one add per launch into the
part's accumulator row, then k_read_returns: thread t adds rows t, t + 256, ... in order and a halving tree over the 256 threads.

The expectations need no GPU (the action stream is Philox on the host): the unmarked tests check them on the oracle alone."""
import numpy as np
import pytest

from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP

SEED, T, CALLS = 0x7A66ED, 8, 3          # T >= 8: the second sgw_step_n call over a buffer is captured, the third replayed
STEPS = T * CALLS
NS = (1, 63, 65, 129)
OUTS = ("step_type", "cumulative")
# id: env name, make_spec / oracle kwargs, oracle, SGW_GENERIC_STEP, expected sgw_step_shape (None: not an island spec)
FAMILIES = {
    "island_shaped": ("island_navigation_ex", dict(level=9, max_iterations=5), "scalar", False, 1),
    "island_generic": ("island_navigation_ex", dict(level=9, max_iterations=5), "scalar", True, 0),
    "boat_race_ex": ("boat_race_ex", dict(level=3, max_iterations=5), "scalar", False, None),
    "island_ex_ma": ("island_navigation_ex_ma", dict(max_iterations=5), "ima", False, None),
    "firemaker_ex_ma": ("firemaker_ex_ma", dict(amount_agents=3, max_iterations=5), "ma", False, None),
}
FRACTIONAL = ("island_navigation_ex", dict(level=9, max_iterations=5, MOVEMENT_REWARD={"MOVEMENT_REWARD": -0.3}), "scalar", False, 0)
PATHS = ("step", "step_n", "rollout")


def device_order_returns(last, cum, n_pad):
  """last bool [E, S], cum float64 [E, S, A*K]: the episodes that end at each step and their return vectors -> what the
  accumulators hold after S launches and k_read_returns makes of them, in the device's order of additions."""
  E, S, AK = cum.shape
  C, rows = AK + 1, n_pad // 64 * 4                          # SGW_ACC_PARTS = 4 accumulator rows per env-wave
  acc = np.zeros((rows, C))
  for t in range(S):
    staged = np.zeros((n_pad, C))                            # a padded lane's row and an unfinished env's row: zeros
    staged[:E, :AK] = np.where(last[:, t, None], cum[:, t], 0.0)
    staged[:E, AK] = last[:, t]
    v = staged.reshape(rows, 16, C)
    for w in (8, 4, 2, 1):
      v = v[:, :w] + v[:, w:2 * w]
    wave_adds = np.repeat(staged[:, AK].reshape(-1, 64).any(axis=1), 4)      # a wave with no finished episode adds nothing
    acc[wave_adds] = acc[wave_adds] + v[wave_adds, 0]
  part = np.zeros((256, C))
  for w in range(rows):
    part[w % 256] = part[w % 256] + acc[w]
  for s2 in (128, 64, 32, 16, 8, 4, 2, 1):
    part[:s2] = part[:s2] + part[s2:2 * s2]
  return part[0]


_CASES = {}


def case(fam, n, family=None):
  """Per (family, env count), cached and left unchanged: row, spec, inputs, the host action stream int8 [STEPS, n(, A)], and
  from the oracle the finished-episode mask [n, STEPS], the return vectors [n, STEPS, A*K] and the expected read_returns."""
  if (fam, n) in _CASES:
    return _CASES[(fam, n)]
  name, kw, orc, generic, shape = family or FAMILIES[fam]
  row = LP._row(fam, name, kw, n, None, oracle=orc, outs=OUTS, rng=orc != "scalar")
  spec = make_spec(name, **kw)
  inp = LP.inputs(row, spec, 5)
  acts = np.stack([philox.actions(SEED, np.arange(n), np.arange(STEPS), spec.action_lo, spec.n_actions, agent=a)
                   for a in range(spec.A)], axis=-1).astype(np.int8)
  if spec.A == 1:
    acts = acts[..., 0]
  want = LP.run_oracle(row, acts, inp, nthreads=4)
  s0 = LP.resets(row) - 1                                    # the two-reset oracles record both resets
  st = want["step_type"][:, s0:].reshape(n, STEPS + 1, -1)
  cum = want["cumulative"][:, s0:].reshape(n, STEPS + 1, -1)
  assert cum.shape[2] == spec.A * spec.K
  done = (st >= 2).all(axis=2)
  last = done[:, 1:] & ~done[:, :-1]
  c = dict(row=row, spec=spec, inp=inp, acts=acts, generic=generic, shape=shape, last=last, cum=cum[:, 1:],
           returns=LP.finished_returns(st, cum))
  _CASES[(fam, n)] = c
  return c


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_oracle_expectation_is_exact_and_every_env_finishes(fam, n):
  c = case(fam, n)
  last, cum, r = c["last"], c["cum"], c["returns"]
  assert last.any(axis=1).all(), "every env ends an episode inside the run"
  assert r[-1] == last.sum() and r[-1] >= 2 * n
  ended = cum[last]
  assert np.array_equal(ended, np.round(ended)) and np.abs(ended).max() < 2.0 ** 40, "integer returns: sums exact in any order"
  assert np.array_equal(r[:-1], ended.sum(axis=0))
  n_pad = -(-n // 64) * 64
  assert np.array_equal(device_order_returns(last, cum, n_pad), r), "the device's order of additions gives the same sums"
  if fam == "island_ex_ma":
    assert c["spec"].A * c["spec"].K + 1 > 16                # the transpose needs a second pass of 16 columns


def test_fractional_expectation_depends_on_the_order():
  """The fractional sums do round: a plain sum over the run differs from the device's order somewhere in the last bits, or at
  least the returns are not integers (so the bit-equality test below is not vacuous)."""
  c = case("island_fractional", 65, FRACTIONAL)
  ended = c["cum"][c["last"]]
  assert not np.array_equal(ended, np.round(ended))
  r = device_order_returns(c["last"], c["cum"], 128)
  assert r[-1] == c["last"].sum() and np.allclose(r, c["returns"], rtol=1e-12, atol=0)


def _play(eng, c, path):
  """The case through one of PATHS on an engine that was just made -> (read_returns, n_pad); closes the engine."""
  import torch
  LP.start(eng, c["row"])
  acts = torch.from_numpy(c["acts"]).to(LP.DEV)
  if path == "step":                                         # one direct launch of the one-step kernel per call
    for t in range(STEPS):
      eng.step_n(acts[t:t + 1], accumulate=True)
  elif path == "step_n":                                     # direct launches, capture + replay, replay
    buf = torch.empty_like(acts[:T])
    for k in range(CALLS):
      buf.copy_(acts[k * T:(k + 1) * T])
      eng.step_n(buf, accumulate=True)
  else:                                                      # the in-kernel Philox stream is the same stream
    eng.rollout(STEPS, SEED, step0=0, accumulate=True)
  r = eng.read_returns().cpu().numpy()
  n_pad = eng.n_pad
  eng.close()
  return r, n_pad


def _run(c, path, monkeypatch):
  from ai_safety_gridworlds_amd import _native as N
  if c["generic"]:
    monkeypatch.setenv("SGW_GENERIC_STEP", "1")
  try:
    eng = LP.make_engine(c["row"], c["spec"], c["inp"])
  finally:
    monkeypatch.delenv("SGW_GENERIC_STEP", raising=False)
  if c["shape"] is not None:
    assert int(N.lib().sgw_step_shape(eng._h)) == c["shape"]
  if c["row"]["id"] == "island_fractional":
    assert int(N.lib().sgw_state_words(eng._h)) == 22, "a reward that does not pack selects the plain f64 state"
  return _play(eng, c, path)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_ragged_returns_equal_oracle(fam, n, path, monkeypatch):
  c = case(fam, n)
  r, _ = _run(c, path, monkeypatch)
  w = c["returns"]
  assert r[-1] == w[-1], "%s n=%d %s: %d finished episodes, the oracle has %d" % (fam, n, path, r[-1], w[-1])
  assert np.array_equal(r, w), "%s n=%d %s: returns %s, the oracle's %s" % (fam, n, path, r, w)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_fractional_returns_keep_the_device_order(path, monkeypatch):
  c = case("island_fractional", 65, FRACTIONAL)
  r, n_pad = _run(c, path, monkeypatch)
  w = device_order_returns(c["last"], c["cum"], n_pad)
  assert r[-1] == w[-1]
  assert r.tobytes() == w.tobytes(), "%s: returns %s, expected in the device's order %s" % (path, r, w)
