"""The headline's one-step kernel against the C oracle, bit for bit, at the sizes where its prologue can go wrong (the loads'
order, the staging of the pow pieces, the kernarg touch settled at the one workgroup barrier): N = 1, 65 (a
second, ragged wave) and 257 (a ragged wave alone in a last workgroup whose other three env-waves are dead and must still reach the
barrier).

Two action sets per size, repeated three times (sgw_step_n is called three times with the SAME buffer: direct launches, capture,
replay):
* 64 steps of the project's Philox stream;
* a scripted tape per env group (env e plays tape e % 4: that many leading no-ops, the script, then Philox actions up to 32
  steps).  The script is checked on the oracle before anything runs on the GPU -- see test_scripted_tape_* (CPU tier): it holds
  a step where drink AND food regrow (the pass runs twice), a regrowth that lands on the growth limit and one from avail 1.

Paths: sgw_step per step; three identical sgw_step_n calls; the same with SGW_GENERIC_RULES (shape-only kernel) and with
SGW_GENERIC_STEP (generic kernel).  Every output of every step is compared with the oracle.  The returns (step_n paths: sgw_step
does not accumulate) are compared exactly: the default rewards are integers, so the sums do not depend on the order of the
device's atomic adds.  The oracle has no packed state, so the exported state is pinned in two steps: it is the same bytes on all
four paths, and imported into a fresh engine it continues for 16 more steps exactly as the oracle does (which needs the
regrowth fractions, the one part of the state that no output shows).

island_navigation_ex_ma (the same engine prologue, pow tables read from global memory): N = 65 through the launch-path matrix
of tests/launch_paths.py (96 sgw_step rounds and three sgw_step_n calls of 16 against its oracle, generator position
included)."""
import numpy as np
import pytest

from ai_safety_gridworlds_amd import philox

LEFT, RIGHT, UP, DOWN, NOOP = 1, 2, 3, 4, 0
# level 9, start (2, 2): up and right twice onto D (drink: 20 -> 10); off (regrows to 13.98), on (3.98), off and two no-ops
# (5.8, 8.3, 11.6), on (1.6), off (regrowth from avail 1); round the wall to F (eat: 20 -> 10, drink at 17.8 by then); off F: the
# food regrows and the drink regrows onto the limit in the same step
SCRIPT = [UP, RIGHT, RIGHT, LEFT, RIGHT, LEFT, NOOP, NOOP, RIGHT, LEFT, DOWN, LEFT, DOWN, DOWN, RIGHT, LEFT]
NS = (1, 65, 257)
GROUPS, T_SCRIPT, T_PHILOX, MORE, SEED = 4, 32, 64, 16, 0x5AFE
FIELDS = ("step_type", "reward", "cumulative", "discount", "term_reason", "actual_action", "frame", "hidden", "board", "metrics", "safety")
KERNELS = ((None, 1, 1), ("SGW_GENERIC_RULES", 0, 1), ("SGW_GENERIC_STEP", 0, 0))     # env at sgw_create, step_rules, step_shape


def tape(kind, n):
  """int8 [T, n]"""
  ids = np.arange(n, dtype=np.uint64)
  if kind == "philox":
    return philox.actions(SEED, ids, np.arange(T_PHILOX, dtype=np.uint64), 0, 5).astype(np.int8)
  a = philox.actions(SEED + 1, ids, np.arange(T_SCRIPT, dtype=np.uint64), 0, 5).astype(np.int8)
  for e in range(n):
    g = e % GROUPS
    a[:g, e] = NOOP
    a[g:g + len(SCRIPT), e] = SCRIPT
  return a


_ORACLE = {}


def oracle(kind, n):
  """(actions [3 T + MORE, n], the oracle's arrays [n, 3 T + MORE + 1, ...]): the tape three times over, then MORE Philox steps"""
  if (kind, n) not in _ORACLE:
    from oracle import oracle as O
    t = tape(kind, n)
    more = philox.actions(SEED + 2, np.arange(n, dtype=np.uint64), np.arange(MORE, dtype=np.uint64), 0, 5).astype(np.int8)
    acts = np.concatenate([t, t, t, more])
    want = O.run_streams(O.make_config("island_navigation_ex"), acts.T.copy(), fields=list(FIELDS))
    _ORACLE[(kind, n)] = (acts, want)
  return _ORACLE[(kind, n)]


def regrowth_events(want):
  """bool [E, S] each: drink and food regrow in the same step; a drink regrowth lands on the limit; a drink regrowth from avail 1"""
  d, f = want["metrics"][..., 1], want["metrics"][..., 3]                  # DrinkAvailability, FoodAvailability: the integer parts
  same_episode = want["step_type"][:, 1:] != 0
  d_up, f_up = (d[:, 1:] > d[:, :-1]) & same_episode, (f[:, 1:] > f[:, :-1]) & same_episode
  return d_up & f_up, d_up & (d[:, 1:] == 20.0), d_up & (d[:, :-1] == 1.0)


@pytest.mark.parametrize("n", NS)
def test_scripted_tape_regrows_both_lands_on_the_limit_and_starts_from_one(n):
  _, want = oracle("script", n)
  both, limit, one = regrowth_events(want)
  for g in range(min(GROUPS, n)):                                          # every env group's tape, inside its first pass
    for what, ev in (("drink and food regrow in one step", both), ("a regrowth lands on the limit", limit), ("a regrowth from avail 1", one)):
      assert ev[g, :T_SCRIPT].any(), "tape %d: no step where %s" % (g, what)


def _same(g, w):
  return bool(((g == w) | ((g != g) & (w != w))).all())


def _compare(got, want, s0, n, label):
  """got {field: [S, n_pad, ...]} device tensors = steps s0 .. s0 + S - 1 of the oracle's record"""
  for k in FIELDS:
    g = np.moveaxis(got[k].cpu().numpy()[:, :n], 0, 1)
    w = want[k][:, s0:s0 + g.shape[1]]
    if k == "term_reason":
      g = g.astype(np.int16); g[g == 255] = -1
    if k == "metrics":
      g = g[..., :w.shape[-1]]
    assert _same(g.reshape(w.shape), w), "%s: %s differs from the oracle in steps %d..%d" % (label, k, s0, s0 + g.shape[1] - 1)


def _returns(want, steps):
  from tests.launch_paths import finished_returns
  return finished_returns(want["step_type"][:, :steps + 1, None], want["cumulative"][:, :steps + 1])


def _engine(n, env, monkeypatch):
  from ai_safety_gridworlds_amd.engine import BatchedEngine
  from ai_safety_gridworlds_amd.specs import make_spec
  if env:
    monkeypatch.setenv(env, "1")
  try:
    return BatchedEngine(make_spec("island_navigation_ex"), n, device="cuda:0", outputs=FIELDS)
  finally:
    if env:
      monkeypatch.delenv(env, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", ["philox", "script"])
def test_every_path_matches_the_oracle(kind, n, monkeypatch):
  import torch
  from ai_safety_gridworlds_amd import _native as N
  acts, want = oracle(kind, n)
  both, limit, one = regrowth_events(want)
  T = (len(acts) - MORE) // 3
  if kind == "script":
    assert both[:, :T].any() and limit[:, :T].any() and one[:, :T].any()
  dev = torch.from_numpy(acts).to("cuda:0")
  states = []

  # sgw_step, one call per step
  eng = _engine(n, None, monkeypatch)
  assert (N.lib().sgw_step_rules(eng._h), N.lib().sgw_step_shape(eng._h)) == (1, 1)
  rec = {k: [v.clone()] for k, v in eng.reset().items()}
  for t in range(3 * T):
    for k, v in eng.step(dev[t]).items():
      rec[k].append(v.clone())
  _compare({k: torch.stack(v) for k, v in rec.items()}, want, 0, n, "sgw_step")
  states.append(eng.get_state()[:, :n].clone())
  eng.close()

  # three identical sgw_step_n calls: compiled rules, shape only, generic
  for env, rules, shape in KERNELS:
    label = "sgw_step_n" + (" with " + env if env else "")
    eng = _engine(n, env, monkeypatch)
    assert (N.lib().sgw_step_rules(eng._h), N.lib().sgw_step_shape(eng._h)) == (rules, shape), label
    eng.reset()
    buf = dev[:T].clone()
    for call in range(3):
      got = {k: v.clone() for k, v in eng.step_n(buf, write_every=True, accumulate=True).items()}
      _compare(got, want, 1 + call * T, n, "%s call %d" % (label, call))
    r, w = eng.read_returns().cpu().numpy(), _returns(want, 3 * T)
    assert w[-1] > 0 or n == 1, "no episode ends inside the run"
    assert np.array_equal(r, w), "%s: returns %s, the oracle's %s" % (label, r, w)
    states.append(eng.get_state()[:, :n].clone())
    eng.close()
  for s in states[1:]:
    assert torch.equal(s, states[0]), "the exported state differs between the paths"

  # the exported state carries what the oracle's env carries: a fresh generic engine continues from it as the oracle does
  eng = _engine(n, "SGW_GENERIC_STEP", monkeypatch)
  eng.reset()
  full = eng.get_state()
  full[:, :n] = states[0]
  eng.set_state(full.contiguous())
  got = {k: v.clone() for k, v in eng.step_n(dev[3 * T:].clone(), write_every=True).items()}
  _compare(got, want, 1 + 3 * T, n, "continued from the exported state")
  eng.close()


@pytest.mark.gpu
def test_island_navigation_ex_ma_at_65_envs_matches_its_oracle():
  from tests import launch_paths as LP
  row = dict(LP.BY_ID["island_ex_ma"], id="island_ex_ma_n65", n=65, seed=8)
  LP.run_path(row, "step_n")
