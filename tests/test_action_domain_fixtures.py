"""The `_quit` / `_quitlate` fixtures (tests/golden/make_fixtures.py ACTION_DOMAIN) carry what they were recorded for: QUIT
(9), NOOP where the family's own range starts at 1, and the turn actions 5..8, often enough and in the places where a QUIT
frame meets state outside the agent.  These are conditions on the committed files -- the generator asserts the same when it
records them -- so a regenerated tape that no longer exercises a case fails here, not silently."""
import numpy as np
import pytest

from ai_safety_gridworlds_amd.specs import make_spec
from tests import action_domain as AD
from tests import golden_util as G
from tests import launch_paths as LP

NAMES = [n for n in G.fixture_names(G.SCALAR_PREFIXES) if n.endswith(("_quit", "_quitlate"))]
QUIT = 3                                  # term_reason of Actions.QUIT
DENSE = ["island_L9", "boat_ex_L3", "boat_race_L0", "safe_int_L1", "safeintex_L1", "islnav_L0", "dshift_test", "absent_random",
         "sokoban_L1", "conveyor_sushi_goal", "conveyorex_vase", "tomato_watering", "tomato_crmdp", "friendfoe_random",
         "whisky_human", "rocks_L1"]
SPARSE_ONLY = ["absent_present", "safe_int_L1_p1", "conveyor_sushi_goal2", "rocks_L0"]


def test_every_action_domain_fixture_is_committed():
  assert sorted(NAMES) == sorted([n + "_quit" for n in DENSE] + [n + "_quitlate" for n in DENSE + SPARSE_ONLY])


def test_fixture_replays_enrol_the_action_domain_fixtures():
  """The oracle test, the host build of the kernel sources and the GPU fixture replay pick their cases up by prefix: every
  action-domain fixture is a case of each."""
  from tests import test_host_families as H, test_oracle_golden as OG, test_parity_gpu as P
  def cases(*fns):
    return [n for f in fns for m in f.pytestmark if m.name == "parametrize" for n in m.args[1]]
  assert sorted(n for n in cases(OG.test_oracle_matches_reference_fixture) if n in NAMES) == sorted(NAMES)
  assert sorted(n for n in cases(P.test_hip_matches_reference_fixture) if n in NAMES) == sorted(NAMES)
  host = cases(H.test_island_source_on_the_host_matches_reference, H.test_deterministic_scalar_family_source_on_the_host_matches_reference,
               H.test_externally_randomised_scalar_family_source_on_the_host_matches_reference)
  assert sorted(n for n in host if n in NAMES) == sorted(NAMES)


def quit_last(fx):
  return (fx["step_type"] == 2) & (fx["term_reason"] == QUIT)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_submits_quit_and_out_of_range_actions(name):
  fx, meta = G.load(name)
  spec = make_spec(meta["family_name"], **meta["kwargs"])
  acts = fx["actions"]
  assert acts.min() >= 0 and acts.max() == 9
  assert quit_last(fx).sum() >= 100
  assert ((acts >= 5) & (acts <= 8)).sum() >= 100
  if spec.action_lo == 1:
    assert (acts == 0).sum() >= 20
  for f in ("obs_board", "rgb", "hidden", "cumulative", "actual_action", "discount", "last_performance"):
    assert f in fx.files, "every field is kept"
  assert (meta["action_lo"], meta["n_actions"]) == (spec.action_lo, spec.n_actions)
  if name.endswith("_quitlate"):
    assert (meta["tape_lo"], meta["tape_n_actions"]) == (spec.action_lo, spec.n_actions)
    assert ((fx["step_type"] == 2) & (fx["term_reason"] != QUIT)).sum() >= 1, "an episode ends for another reason as well"
  else:
    assert (meta["tape_lo"], meta["tape_n_actions"]) == (0, 10)


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("absent_")])
def test_absent_supervisor_fixture_punishes_on_quit_frames(name):
  fx, _ = G.load(name)
  assert (quit_last(fx) & (fx["reward"][:, :, 0] == -30.0)).sum() >= 4


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("tomato_")])
def test_tomato_fixture_draws_on_quit_frames(name):
  fx, _ = G.load(name)
  d = fx["draws_at"]
  drew = np.zeros(d.shape, bool)
  drew[:, 1:] = d[:, 1:] > d[:, :-1]
  assert (quit_last(fx) & drew).sum() >= 1
  assert np.array_equal(d[:, -1], fx["rand_count"])


# ---- the launch-path tapes of tests/test_action_domain_gpu.py, with the oracle alone ----


def test_rows_are_the_scalar_launch_path_rows_at_ragged_sizes():
  assert [r["id"] for r in AD.ROWS] == [r["id"] for r in LP.ROWS if r["oracle"] == "scalar"] and len(AD.ROWS) == 18
  assert {r["n"] for r in AD.ROWS} == {1, 63, 65, 193}
  assert all(r["n"] <= 193 and AD.steps_of(r) <= 112 for r in AD.ROWS)
  assert set(AD.FOLLOW) <= set(AD.BY_ID) and all(m in AD.BY_ID for _, ms in AD.GROUPS for m in ms)


@pytest.mark.parametrize("row_id", [r["id"] for r in AD.ROWS])
def test_row_tape_ends_an_episode_with_quit_inside_its_calls(row_id):
  row = AD.BY_ID[row_id]
  spec = make_spec(row["name"], **row["kw"])
  tape = AD.host_tape(row, spec)
  assert (tape == 9).any() and (row["n"] == 1 or ((tape >= 5) & (tape <= 8)).any())
  want = LP.run_oracle(row, tape, AD.inputs(row, spec), nthreads=4)
  assert AD.quit_lasts(want, row["calls"] * AD.T) >= 1
  assert AD.quit_lasts(want, AD.CALLS * AD.T) >= 1, "the group paths run CALLS calls"


def test_overlay_is_the_fixture_rule():
  """The `_quitlate` fixtures were drawn by the rule the launch-path tapes use (another seed)."""
  from ai_safety_gridworlds_amd import philox
  fx, meta = G.load("tomato_watering_quitlate")
  E, Tn = fx["actions"].shape
  seed, ids, steps = int(meta["seed"]), np.arange(E), np.arange(Tn)
  base = philox.actions(seed, ids, steps, int(meta["tape_lo"]), int(meta["tape_n_actions"]))
  old = AD.SEED
  try:
    AD.SEED = seed
    assert np.array_equal(AD.overlay(base, ids).T, fx["actions"])
  finally:
    AD.SEED = old


@pytest.mark.parametrize("name", [n for n in NAMES if n.startswith("tomato_")])
def test_oracle_draw_count_matches_the_reference(name):
  """or_env_random_draws (what the GPU test compares the engine's stream position with) against the reference's own count of
  np.random.random() calls, at every step of four streams."""
  from oracle import oracle as O
  fx, meta = G.load(name)
  cfg = O.make_config(meta["family_name"], **meta["kwargs"])
  for e in range(4):
    env = O.Env(cfg)
    env.set_random_stream(fx["rand_stream"][e])
    env.reset()
    got = [env.random_draws()]
    for a in fx["actions"][e]:
      env.step(int(a))
      got.append(env.random_draws())
    assert got == list(fx["draws_at"][e])
