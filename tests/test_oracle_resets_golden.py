"""Pin every oracle's explicit reset to the reference: fixtures whose action tapes carry RESET (-128) at ticks that differ per
stream (tests/golden/resets_*.npz; the generators called the reference's own reset() there) -- immediately after a reset,
mid-episode, on the tick after LAST in place of the auto-reset, and on the tick after an auto-reset.  Every recorded field
must be equal bit for bit, the generator position included."""
import numpy as np
import pytest

from oracle import oracle as O, oracle_ima as OI, oracle_ma as OM, oracle_sav as OS
from tests import golden_util as G
from tests import reset_schedules as RS
from tests import test_oracle_golden as TG, test_oracle_ima_golden as TI, test_oracle_ma_golden as TM, test_oracle_sav_golden as TS

NAMES = G.fixture_names(["resets_"])
CLASSES = {"after_reset", "mid", "after_last", "after_auto"}


def _multi(name):
  fam = G.load(name)[1]["family"]
  return {"firemaker_ex_ma": "ma", "island_navigation_ex_ma": "ima", "aintelope_savanna": "sav"}.get(fam, "scalar")


def test_every_listed_family_has_a_reset_fixture():
  fams = sorted((G.load(n)[1]["family"], str(sorted(G.load(n)[1]["kwargs"].items()))) for n in NAMES)
  assert [f for f, _ in fams] == ["absent_supervisor", "aintelope_savanna", "distributional_shift", "firemaker_ex_ma", "friend_foe",
                                  "island_ex", "island_navigation_ex_ma", "island_navigation_ex_ma", "safe_interruptibility",
                                  "side_effects_sokoban", "tomato_watering", "whisky_gold"]
  freq = sorted(G.load(n)[1]["kwargs"]["map_randomization_frequency"] for n in NAMES if _multi(n) == "ima")
  assert freq == [2, 3]
  for n in NAMES:                                               # the kwargs that make each family's reset worth pinning
    fam, kw = G.load(n)[1]["family"], G.load(n)[1]["kwargs"]
    for k, v in PINNED_KWARGS[fam].items():
      assert kw.get(k) == v, "%s: %s = %r, not %r" % (n, k, kw.get(k), v)
    assert fam != "whisky_gold" or not kw.get("human_player", False)       # (the agent itself explores)


PINNED_KWARGS = {
    "safe_interruptibility": dict(level=1), "distributional_shift": dict(is_testing=True), "absent_supervisor": {},
    "friend_foe": dict(bandit_type="adversary"), "tomato_watering": {}, "whisky_gold": dict(whisky_exploration=0.7),
    "island_ex": dict(level=9, max_iterations=20), "side_effects_sokoban": dict(level=0),
    "firemaker_ex_ma": dict(amount_agents=3, max_iterations=20), "island_navigation_ex_ma": {},
    "aintelope_savanna": dict(amount_agents=2, map_randomization_frequency=3),
}


@pytest.mark.parametrize("name", NAMES)
def test_tape_holds_every_kind_of_reset_at_ragged_ticks(name):
  fx, meta = G.load(name)
  off = 0 if _multi(name) in ("scalar", "ma") else 1            # (records of the two-reset families start one slot earlier)
  acts = fx["actions"].reshape(fx["actions"].shape[0], fx["actions"].shape[1], -1)[:, :, 0]
  E, T = acts.shape
  assert E <= 32 and T <= 120
  seen = set()
  for e in range(E):
    seen |= RS.tape_classes(fx["step_type"][e, off:], acts[e])
  assert seen == CLASSES, "%s: the tapes hold %s" % (name, sorted(seen))
  ticks = [tuple(np.nonzero(acts[e] == RS.RESET)[0]) for e in range(E)]
  assert len(set(ticks)) > E // 2, "the reset ticks differ per stream"


@pytest.mark.parametrize("name", [n for n in NAMES if _multi(n) == "scalar"])
def test_oracle_matches_reference_resets(name):
  fx, meta = G.load(name)
  cfg = O.make_config(meta["family_name"], **meta["kwargs"])
  bits = G.interrupt_bits(fx) if "should_interrupt" in fx.files else None
  rand = fx["rand_stream"] if "rand_stream" in fx.files and fx["rand_stream"].shape[1] else None
  out = O.run_streams(cfg, fx["actions"], interrupt_bits=bits, rand_stream=rand)
  for f in TG.FIELDS + [f for f in ("metrics", "safety", "should_interrupt") if f in fx.files]:
    G.assert_same(name + "." + f, out[f], fx[f])
  m = G.performance_mask(fx)
  G.assert_same(name + ".last_performance", out["last_performance"][m], fx["last_performance"][m])


@pytest.mark.parametrize("name", [n for n in NAMES if _multi(n) == "ma"])
def test_ma_oracle_matches_reference_resets(name):
  fx, meta = G.load(name)
  out = OM.run_streams(OM.make_config(**meta["kwargs"]), fx["actions"], fx["rng_init"])
  for f in TM.FIELDS + ["action_direction", "observation_direction"]:
    G.assert_same(name + "." + f, out[f], fx[f])
  assert (out["reward_none"].astype(bool) == fx["reward_none"]).all()


@pytest.mark.parametrize("name", [n for n in NAMES if _multi(n) in ("ima", "sav")])
def test_ima_sav_oracles_match_reference_resets(name):
  fx, meta = G.load(name)
  Or, fields = (OI, TI.FIELDS) if _multi(name) == "ima" else (OS, TS.FIELDS)
  out = Or.run_streams(Or.make_config(**meta["kwargs"]), fx["actions"], fx["rng_seeded"])
  G.assert_same(name + ".rng[0]", out["rng"][:, 0], fx["rng"][:, 0])
  for f in fields:
    w = fx["drape_layers" if f == "layers" else f]             # (stored under another key: see make_fixtures_sav.py)
    G.assert_same(name + "." + f, out[f][:, 1:], w[:, 1:])
  assert (out["reward_none"][:, 1:].astype(bool) == fx["reward_none"][:, 1:]).all()
