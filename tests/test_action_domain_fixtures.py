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


# ---- the multi-agent families: firemaker_ex_ma, island_navigation_ex_ma, aintelope_savanna ----

MA_NAMES = [n for n in G.fixture_names(["firemaker_", "ima_", "sav_"]) if n.endswith(("_quit", "_quitlate"))]
MA_WANTED = ["firemaker_L0_quitlate", "firemaker_L0_a1_quit", "firemaker_L0_a2_turn_quitlate",
             "ima_L9_quit", "ima_L10_rand3_quitlate", "ima_L9_rand3_quitlate", "ima_L9_turn_quitlate", "ima_L9_aec_quitlate",
             "sav_rich2_quitlate", "sav_rich1_quit", "sav_rich2_turn_quitlate"]
# level 10 of the island has no water and no goal: no agent is done before the other, so that one file cannot hold a QUIT next
# to a LAST / DEAD agent (ima_L9_rand3_quitlate is the same map randomisation on a level that can)
ALONE_NEVER_DONE = ("ima_L10_rand3_quitlate",)


def test_every_multi_agent_action_domain_fixture_is_committed():
  assert sorted(MA_NAMES) == sorted(MA_WANTED)


def test_fixture_replays_enrol_the_multi_agent_action_domain_fixtures():
  from tests import test_firemaker_gpu as FG, test_host_families as H, test_island_ma_gpu as IG, test_savanna_gpu as SG
  from tests import test_oracle_ima_golden as OI, test_oracle_ma_golden as OM, test_oracle_sav_golden as OS
  def cases(*fns):
    return [n for f in fns for m in f.pytestmark if m.name == "parametrize" and m.args[0] == "name" for n in m.args[1]]
  oracle = cases(OM.test_ma_oracle_matches_reference_fixture, OI.test_ima_oracle_matches_reference_fixture,
                 OS.test_sav_oracle_matches_reference_fixture)
  assert sorted(n for n in oracle if n in MA_NAMES) == sorted(MA_NAMES)
  gpu = cases(FG.test_firemaker_hip_matches_reference_fixture, IG.test_island_ma_hip_matches_reference_fixture,
              SG.test_savanna_hip_matches_reference_fixture)
  assert sorted(n for n in gpu if n in MA_NAMES) == sorted(MA_NAMES)
  host = cases(H.test_multi_agent_family_source_on_the_host_matches_reference)
  assert sorted(n for n in host if n in MA_NAMES) == sorted(n for n in MA_NAMES if not n.startswith("firemaker_"))   # (no host build)


def _ma_layout(name, fx, meta):
  """(present agent columns, record slots before the first tick's) of a multi-agent fixture."""
  if name.startswith("firemaker_"):
    return {1: [0], 2: [0, 2], 3: [0, 1, 2]}[meta["kwargs"]["amount_agents"]], 1
  return list(range(fx["step_type"].shape[2])), 2


@pytest.mark.parametrize("name", MA_NAMES)
def test_multi_agent_fixture_holds_its_quit_rounds(name):
  """From the recorded arrays alone: a QUIT-ended episode for every agent index as the quitter, a whole (multi-submitter) and a
  solo QUIT round, 20 ticks after the first QUIT, a QUIT next to a LAST / DEAD agent (island; no savanna or firemaker agent is
  ever done alone), a QUIT on a tick on which the fire spreads (firemaker); and the counts the generator wrote into the meta."""
  fx, meta = G.load(name)
  slots, resets = _ma_layout(name, fx, meta)
  rec = {k: fx[k] for k in ("actions", "submitted", "step_type", "term_reason", "board")}
  got = AD.quit_fixture_counts(name, rec, slots, resets=resets)          # (asserts the per-agent, whole / solo and tail conditions)
  for k, v in got.items():
    assert np.array_equal(np.asarray(v), meta[k]), k
  acts = fx["actions"][:, :, slots]
  assert acts.max() == 9 and (meta["tape_turns"] == 1) == bool(((acts >= 5) & (acts <= 8)).any())
  if name.startswith("ima_") and name not in ALONE_NEVER_DONE:
    assert got["quit_others_done"] >= 1
  if name.startswith("firemaker_"):
    assert got["quit_fire_spread"] >= 1
  # a round with a 9 is one the reference defines: the quitter submits alone, or nobody plays after it (one frame per submitter)
  live = ~(fx["step_type"][:, resets - 1:-1][:, :, slots] >= 2).all(axis=2)
  nine = (fx["submitted"][:, :, slots] & (acts == 9)).sum(axis=2) * live
  assert (nine <= 1).all()
  plays = fx["frame"][:, resets:] - fx["frame"][:, resets - 1:-1]
  assert (plays[nine == 1] == fx["submitted"][:, :, slots].sum(axis=2)[nine == 1]).all()


def test_multi_agent_rows_are_the_launch_path_rows_and_one_turn_row():
  assert [r["id"] for r in AD.MA_ROWS] == ["firemaker_ex_ma", "island_ex_ma", "aintelope_savanna", "island_ex_ma_turn"]
  assert {r["n"] for r in AD.MA_ROWS} == {1, 63, 65, 193} and all(r["tag"] is None for r in AD.MA_ROWS)
  assert all(48 <= AD.ma_steps_of(r) <= 112 for r in AD.MA_ROWS)
  turn = make_spec(AD.MA_TURN_ROW["name"], **AD.MA_TURN_ROW["kw"])
  assert turn.A == 2 and turn.n_actions == 9 and AD.turns_survive(turn)


@pytest.mark.parametrize("row_id", [r["id"] for r in AD.MA_ROWS])
def test_multi_agent_row_tape_holds_quit_rounds_inside_its_calls(row_id):
  """With the oracle alone: a QUIT-ended episode per agent index, a round in which a play is dropped behind a QUIT, and a whole
  QUIT round, inside the row's calls."""
  row = AD.MA_BY_ID[row_id]
  spec = make_spec(row["name"], **row["kw"])
  tape = AD.ma_host_tape(row, spec)
  assert (tape == 9).any() and AD.turns_survive(spec) == bool(((tape >= 5) & (tape <= 8) & (spec.n_actions == 5)).any() or spec.n_actions == 9)
  want = LP.run_oracle(row, tape, AD.ma_inputs(row, spec), nthreads=4)
  got = AD.ma_quit_rounds(row, spec, tape, want, AD.ma_steps_of(row))
  assert (got["per_agent"] >= 1).all() and got["dropped"] >= 1 and got["whole"] >= 1, got
