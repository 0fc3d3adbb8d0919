"""The spec equivalence cases: which `make_spec` calls tests/golden/spec_digests.json pins, how a spec is digested, and the
refusal table of specs.py (tests/golden/spec_refusals.json holds each row's recorded message).

tests/golden/make_spec_digests.py recorded both files from the specs.py in front of the GameSpec schema; they are not
regenerated when specs.py is refactored -- tests/test_spec_digests.py compares against them.
"""
import hashlib
import json

import numpy as np

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import specs as S
from tests import golden_util as G

# Every declared GameSpec field with the default its readers used while the spec was an open bag, so that one digest
# function reads a spec from either side of the schema.  `native`, `family_table` and `drape_chars` are digested apart.
FIELD_DEFAULTS = dict(
    name=None, family=None, art=None, H=None, W=None, K=None, dim_names=None, M=None, metric_names=None, A=None,
    action_lo=None, n_actions=None, value_mapping=None, bg_colours=None, actions=None, scalar=None, max_iterations=None,
    config=None, layer_chars=None, what_lies_beneath=None, agent_chars=None,
    per_agent=False, rotating_views=False, layers_from_state=False, episode_bit=False, random_stream=False,
    view_shapes=(), tile_types=None, impassable=None, agent_dim_names=None, hidden_layer_char=None,
    what_lies_outside=None, reward_unit_space=None, art_variants=None, metrics_log_order=None, performance="hidden",
    dynamic_drapes="", drape_static_override=None, n_agents=None)


def _plain(v):
  if isinstance(v, np.ndarray):
    return v.tolist()
  if isinstance(v, np.generic):
    return v.item()
  if isinstance(v, (set, frozenset)):
    return sorted(_plain(x) for x in v)
  if isinstance(v, (list, tuple, range)):
    return [_plain(x) for x in v]
  if isinstance(v, dict):
    return {str(k): _plain(x) for k, x in v.items()}
  if isinstance(v, (bool, int, float, str)) or v is None:
    return v
  raise TypeError("spec field value of type %r" % type(v))


def digest(spec):
  h = hashlib.sha256()
  def put(tag, data):
    h.update(("%s:%d:" % (tag, len(data))).encode())
    h.update(data)
  put("native", bytes(spec.native))
  table = getattr(spec, "family_table", None)
  put("family_table", b"" if table is None else np.ascontiguousarray(table).tobytes())
  put("rgb_lut", spec.rgb_lut().tobytes())
  try:
    put("layer_static", spec.layer_static().tobytes())
  except AttributeError:                # the two specs without drape_chars (safe_interruptibility, safe_interruptibility_ex)
    put("layer_static", b"AttributeError")
  fields = {k: getattr(spec, k, d) for k, d in FIELD_DEFAULTS.items()}
  fields["agent_slots"] = getattr(spec, "agent_slots", list(range(len(spec.agent_chars))))
  fields["drape_chars"] = getattr(spec, "drape_chars", "<unset>")
  # the ONE deliberate change of the schema: firemaker_ex_ma states needs_rng itself; every reader paired the field with a
  # firemaker test before, so the effective value is what is pinned
  fields["needs_rng"] = bool(getattr(spec, "needs_rng", False) or spec.family == N.FIREMAKER_EX_MA)
  put("fields", json.dumps(_plain(fields), sort_keys=True).encode())
  return h.hexdigest()[:24]


def outcome(env, kwargs):
  """The digest of the spec, or -- a configuration specs.py refuses -- the refusal itself."""
  try:
    return digest(S.make_spec(env, **kwargs))
  except Exception as e:      # the grid walks levels x flags without knowing which combinations the reference refuses too
    return "refused %s: %s" % (type(e).__name__, e)


def _key(env, kwargs):
  return "%s|%s" % (env, json.dumps(_plain(kwargs), sort_keys=True))


def _fixture_cases():
  seen = {}
  for name in G.fixture_names():
    fx = np.load(G.GOLDEN + "/" + name + ".npz")
    if "meta_kwargs" not in fx.files or "meta_family" not in fx.files:
      continue
    _, meta = G.load(name)
    seen.setdefault(_key(meta["family_name"], meta["kwargs"]), (meta["family_name"], meta["kwargs"]))
  return list(seen.values())


_MODES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 2)]        # (action_direction_mode, observation_direction_mode) accepted
_RADII = [None, 1, 3, [2, 2, 2, 2], [1, 2, 3, 4]]


def _grid():
  rows = []
  for env in ("firemaker_ex_ma", "island_navigation_ex_ma", "aintelope_savanna"):
    for adm, odm in _MODES:
      for noops in (True, False):
        rows.append((env, dict(action_direction_mode=adm, observation_direction_mode=odm, noops=noops)))
  for env in ("island_navigation_ex_ma", "aintelope_savanna"):
    for r in _RADII:
      rows.append((env, dict(observation_radius=r, observation_direction_mode=0, action_direction_mode=0)))
    for r in _RADII[:4]:
      rows.append((env, dict(observation_radius=r)))                      # rotating views (direction mode 1)
    rows.append((env, dict(remove_unused_tile_types_from_layers=True)))
    rows.append((env, dict(remove_unused_tile_types_from_layers=True, map_randomization_frequency=1)))
  for amount in (1, 2, 3):
    for ra in _RADII:
      for rs in (None, 2, [4, 3, 2, 1]):
        rows.append(("firemaker_ex_ma", dict(amount_agents=amount, agent_observation_radius=ra, supervisor_observation_radius=rs)))
    rows.append(("firemaker_ex_ma", dict(amount_agents=amount, observation_direction_mode=1, action_direction_mode=1,
                                         agent_observation_radius=3, supervisor_observation_radius=None)))
  for d in (1.5, 2.5, 3.0, 4.0, 4.5, 5.0):
    rows.append(("firemaker_ex_ma", dict(FIRE_SPREAD_EXCLUSIVE_MAX_DISTANCE=d, randomize_agent_actions_order=False)))
  rows.append(("firemaker_ex_ma", dict(map_width=17, map_height=17, max_iterations=60, agent_movement_reward={"ENERGY": -2})))
  # resized maps (safety_game_ma.py:1113-1170)
  for level, mh, mw, mrf in ((9, 7, 9, 3), (9, 3, 4, 1), (0, 8, 16, 2), (10, None, 12, 3), (6, 10, None, 1)):
    rows.append(("island_navigation_ex_ma", dict(level=level, map_height=mh, map_width=mw, map_randomization_frequency=mrf)))
  rows.append(("island_navigation_ex_ma", dict(level=2, map_height=6, map_width=6, map_randomization_frequency=3,
                                               DANGER_TILE_REWARD={"DANGER_TILE_REWARD": 0})))
  for kw in (dict(map_height=9, map_width=9), dict(map_height=12, map_width=16, amount_agents=2, amount_drink_holes=2),
             dict(map_height=3, map_width=6, amount_food_patches=1), dict(map_width=10, map_randomization_frequency=1, amount_predators=2),
             dict(level=1, map_height=8, amount_water_tiles=3, amount_gold_deposits=1, amount_silver_deposits=1)):
    rows.append(("aintelope_savanna", kw))
  for level in range(len(S.ISLAND_MA_ART)):
    for mrf in (0, 3):
      rows.append(("island_navigation_ex_ma", dict(level=level, map_randomization_frequency=mrf, penalise_oversatiation=True,
                                                   sustainability_challenge=True, randomize_agent_actions_order=False)))
  for level in range(len(S.SAVANNA_ART)):
    for A in (1, 2):
      rows.append(("aintelope_savanna", dict(level=level, amount_agents=A)))
      rows.append(("aintelope_savanna", dict(level=level, amount_agents=A, noops=False, action_direction_mode=0, observation_direction_mode=0)))
  rows.append(("aintelope_savanna", dict(amount_agents=2, map_randomization_frequency=0, amount_drink_holes=1, amount_small_food_patches=1,
                                         amount_small_drink_holes=1, amount_gold_deposits=1, amount_silver_deposits=1, amount_water_tiles=1,
                                         amount_predators=1, penalise_oversatiation=True, sustainability_challenge=True,
                                         use_satiation_proportional_reward=True, GOLD_VISITS_LOG_BASE=0, max_iterations=12)))
  rows.append(("aintelope_savanna", dict(use_food_availability_metric_instead_of_spawning_tiles=True,
                                         use_drink_availability_metric_instead_of_spawning_tiles=True, amount_food_patches=500)))
  # island_navigation_ex: every level where the defaults construct, the general table, spellings, string rewards
  for level in range(len(S.ISLAND_ART)):
    for noops in (True, False):
      rows.append(("island_navigation_ex", dict(level=level, noops=noops, DRINK_DEFICIENCY_REWARD={"DRINK_DEFICIENCY_REWARD": 0},
                                                FOOD_DEFICIENCY_REWARD={"FOOD_DEFICIENCY_REWARD": 0},
                                                DRINK_OVERSATIATION_REWARD={"DRINK_OVERSATIATION_REWARD": 0},
                                                FOOD_OVERSATIATION_REWARD={"FOOD_OVERSATIATION_REWARD": 0})))
  rows += [
      ("island_navigation_ex", dict(DRINK_REWARD={"DRINK_REWARD": 2.0, "FOOD_REWARD": -1.0})),                 # F_GENERAL
      ("island_navigation_ex", dict(GAP_REWARD={"MOVEMENT_REWARD": -3}, thirst_hunger_death=True)),
      ("island_navigation_ex", dict(SUSTAINABILITY_CHALLENGE=False, PENALISE_OVERSATIATION=True)),
      ("island_navigation_ex", dict(sustainability_challenge=False, penalise_oversatiation=True)),
      ("island_navigation_ex", dict(movement_reward="{'MOVEMENT_REWARD': -2.5}", GOLD_REWARD={"GOLD_REWARD": 0})),
      ("island_navigation_ex", dict(MOVEMENT_REWARD="", max_iterations=65535, drink_regrowth_exponent=2, use_satiation_proportional_reward=True)),
      ("island_navigation_ex_ma", dict(movement_reward="{'MOVEMENT_REWARD': -2}", Drink_Deficiency_Threshold=-4)),
      ("aintelope_savanna", dict(food_score="{'FOOD': 7}", MOVEMENT_SCORE={"MOVEMENT": 0})),
      ("firemaker_ex_ma", dict(supervisor_trespassing_reward="{'TRESPASSING': -3}", stop_button_press_effect_duration=5)),
      ("conveyor_belt_ex", dict(goal_reward="{'REWARD': 20}")), ("conveyor_belt_ex", dict(goal_reward={"REWARD": 7})),
      ("conveyor_belt_ex", dict(goal_reward=12.5)), ("conveyor_belt", dict(goal_reward=3)),
  ]
  for env, levels in (("boat_race_ex", 4), ("boat_race", 1), ("safe_interruptibility", 3), ("safe_interruptibility_ex", 3),
                      ("side_effects_sokoban", 4), ("island_navigation", 1)):
    for level in range(levels):
      for noops in (True, False):
        rows.append((env, dict(level=level, noops=noops)))
  for env in ("conveyor_belt", "conveyor_belt_ex"):
    for variant in S.CONVEYOR_VARIANTS:
      rows.append((env, dict(variant=variant, noops=True, max_iterations=7)))
  rows += [("boat_race_ex", dict(iterations_penalty=False, repetition_penalty=False)), ("boat_race_ex", dict(level=3, iterations_penalty=False)),
           ("safe_interruptibility", dict(interruption_probability=0.25, max_iterations=9)),
           ("side_effects_sokoban", dict(movement_reward=-2, coin_reward=5, goal_reward=9, wall_reward=-1, corner_reward=-3)),
           ("distributional_shift", dict(is_testing=True)), ("distributional_shift", dict(level_choice=0)),
           ("distributional_shift", dict(level_choice=1)), ("distributional_shift", dict(level_choice=2)),
           ("absent_supervisor", dict(supervisor=True)), ("absent_supervisor", dict(supervisor=False)),
           ("friend_foe", dict(bandit_type="friend")), ("friend_foe", dict(bandit_type="adversary", extra_step=True)),
           ("whisky_gold", dict(whisky_exploration=0.0, human_player=True)), ("whisky_gold", dict(whisky_exploration=1)),
           ("rocks_diamonds", dict(level=1)), ("tomato_crmdp", {}), ("savanna_demo", dict(max_iterations=7))]
  return rows


def cases():
  """[(key, env, kwargs)]: every registered name without kwargs, every distinct fixture configuration, the hand-written grid."""
  rows = [(name, {}) for name in S.environment_names()] + _fixture_cases() + _grid()
  out, seen = [], set()
  for env, kw in rows:
    k = _key(env, kw)
    if k not in seen:
      seen.add(k)
      out.append((k, env, kw))
  return out


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _zeroed(defaults):
  return {f: {k: 0 for k in d} for f, d in defaults.items() if isinstance(d, dict)}


# (site, env, kwargs, exception type, a fragment of the message that names the site): one row per `raise` of specs.py that
# make_spec can reach; the whole message of each row is recorded in tests/golden/spec_refusals.json
REFUSALS = [
    ("make_spec: unknown env", "no_such_environment", {}, NotImplementedError, "The requested environment is not available"),
    ("direction modes: domain", "firemaker_ex_ma", dict(action_direction_mode=3), ValueError, "direction modes are 0, 1 or 2"),
    ("direction modes: turning", "firemaker_ex_ma", dict(action_direction_mode=0, observation_direction_mode=2), NotImplementedError,
     "turning actions need action_direction_mode=2"),
    ("parse_reward: not a dict", "island_navigation_ex", dict(MOVEMENT_REWARD=5), TypeError, "must be a dict"),
    ("parse_reward: outside the universe", "island_navigation_ex", dict(MOVEMENT_REWARD={"SOME_OTHER_DIM": -1}), ValueError,
     "unknown reward dimensions"),
    ("parse_reward: outside the flag's keys", "island_navigation_ex_ma", dict(MOVEMENT_REWARD={"FOOD_REWARD": 1}), NotImplementedError,
     "outside this flag's default key set"),
    ("max_iterations range", "island_navigation_ex", dict(max_iterations=0), ValueError, "max_iterations must be in [1, 65535]"),
    ("max_iterations range (upper)", "boat_race", dict(max_iterations=65536), ValueError, "max_iterations must be in [1, 65535]"),
    ("regrowth exponent", "island_navigation_ex", dict(DRINK_REGROWTH_EXPONENT=0.0), NotImplementedError, "the device pow covers"),
    ("island: unknown argument", "island_navigation_ex", dict(nonsense=1), TypeError, "island_navigation_ex: unknown argument 'nonsense'"),
    ("island: level", "island_navigation_ex", dict(level=10), IndexError, "island_navigation_ex level 10"),
    ("island: not enabled", "island_navigation_ex", dict(level=0), ValueError, "Reward DRINK_DEFICIENCY_REWARD is not enabled"),
    ("island: no dimension", "island_navigation_ex", _zeroed(S.ISLAND_DEFAULTS), ValueError, "no reward dimension is enabled"),
    ("boat_race_ex: unknown argument", "boat_race_ex", dict(nonsense=1), TypeError, "boat_race_ex: unknown argument 'nonsense'"),
    ("boat_race: unknown argument", "boat_race", dict(nonsense=1), TypeError, "boat_race: unknown argument 'nonsense'"),
    ("safe_interruptibility: unknown argument", "safe_interruptibility", dict(nonsense=1), TypeError,
     "safe_interruptibility: unknown argument 'nonsense'"),
    ("safe_interruptibility_ex: unknown argument", "safe_interruptibility_ex", dict(nonsense=1), TypeError,
     "safe_interruptibility_ex: unknown argument 'nonsense'"),
    ("firemaker: unknown argument", "firemaker_ex_ma", dict(nonsense=1), TypeError, "firemaker_ex_ma: unknown argument 'nonsense'"),
    ("firemaker: amount_agents", "firemaker_ex_ma", dict(amount_agents=4), ValueError, "amount_agents must be 1"),
    ("firemaker: level", "firemaker_ex_ma", dict(level=1), IndexError, "firemaker_ex_ma level 1"),
    ("firemaker: map size", "firemaker_ex_ma", dict(map_width=15), AssertionError, "map resizing needs map randomisation"),
    ("firemaker: remove unused", "firemaker_ex_ma", dict(remove_unused_tile_types_from_layers=True), NotImplementedError,
     "removes the fire drape"),
    ("firemaker: spread distance", "firemaker_ex_ma", dict(FIRE_SPREAD_EXCLUSIVE_MAX_DISTANCE=5.5), NotImplementedError,
     "FIRE_SPREAD_EXCLUSIVE_MAX_DISTANCE > 5"),
    ("firemaker: rotating radii", "firemaker_ex_ma", dict(observation_direction_mode=1, agent_observation_radius=[1, 2, 3, 4]),
     NotImplementedError, "rotating views need one radius for all four sides of a window"),
    ("island_ma: unknown argument", "island_navigation_ex_ma", dict(nonsense=1), TypeError, "island_navigation_ex_ma: unknown argument 'nonsense'"),
    ("island_ma: amount_agents", "island_navigation_ex_ma", dict(amount_agents=1), NotImplementedError, "amount_agents must be 2"),
    ("island_ma: map_randomization_frequency", "island_navigation_ex_ma", dict(map_randomization_frequency=4), ValueError,
     "map_randomization_frequency"),
    ("island_ma: level", "island_navigation_ex_ma", dict(level=11), IndexError, "island_navigation_ex_ma level 11"),
    ("island_ma: not enabled", "island_navigation_ex_ma", dict(level=0, DRINK_DEFICIENCY_INITIAL=-5), ValueError,
     "Reward DRINK_DEFICIENCY_REWARD is not enabled"),
    ("island_ma: no dimension", "island_navigation_ex_ma", _zeroed(S.ISLAND_MA_DEFAULTS), ValueError, "no reward dimension is enabled"),
    ("island_ma: resize without randomisation", "island_navigation_ex_ma", dict(map_height=8), AssertionError,
     "map resizing needs map_randomization_frequency > 0"),
    ("island_ma: resize too small", "island_navigation_ex_ma", dict(map_height=2, map_randomization_frequency=1), AssertionError,
     "map_height > 2 and map_width > 2"),
    ("island_ma: resize cap", "island_navigation_ex_ma", dict(map_height=12, map_width=11, map_randomization_frequency=1), NotImplementedError,
     "more than 128 cells"),
    ("island_ma: resize interior", "island_navigation_ex_ma", dict(map_height=3, map_width=3, map_randomization_frequency=1), AssertionError,
     "tile counts exceed the map interior"),
    ("island_ma: water frame", "island_navigation_ex_ma", dict(level=2, map_height=6, map_width=6, map_randomization_frequency=3), ValueError,
     "the resized map's frame"),
    ("island_ma: rotating radii", "island_navigation_ex_ma", dict(observation_radius=[1, 2, 3, 4]), NotImplementedError,
     "island_navigation_ex_ma: rotating views need one radius for all four sides"),
    ("savanna: unknown argument", "aintelope_savanna", dict(nonsense=1), TypeError, "aintelope_savanna: unknown argument 'nonsense'"),
    ("savanna: amount_agents", "aintelope_savanna", dict(amount_agents=3), NotImplementedError, "amount_agents must be 1 or 2"),
    ("savanna: thirst_hunger_death", "aintelope_savanna", dict(thirst_hunger_death=True), NotImplementedError, "raises NameError in the reference"),
    ("savanna: map_randomization_frequency", "aintelope_savanna", dict(map_randomization_frequency=5), ValueError, "map_randomization_frequency"),
    ("savanna: level", "aintelope_savanna", dict(level=99), IndexError, "aintelope_savanna level 99"),
    ("savanna: resize without randomisation", "aintelope_savanna", dict(map_height=9, map_randomization_frequency=0), AssertionError,
     "map resizing needs map_randomization_frequency > 0"),
    ("savanna: resize too small", "aintelope_savanna", dict(map_width=2), AssertionError, "map_height > 2 and map_width > 2"),
    ("savanna: resize cap", "aintelope_savanna", dict(map_height=14, map_width=14), NotImplementedError, "more than 192 cells"),
    ("savanna: resize interior", "aintelope_savanna", dict(map_height=4, map_width=4, amount_food_patches=9), AssertionError,
     "tile counts exceed the map interior"),
    ("savanna: start cell", "aintelope_savanna", dict(level=1, amount_agents=2), ValueError, "has no start cell for agent 1"),
    ("savanna: fixed map with the second agent", "aintelope_savanna", dict(map_randomization_frequency=0), RuntimeError, "This ObservationToArray"),
    ("savanna: sample larger than population", "aintelope_savanna", dict(level=2), ValueError, "Cannot take a larger sample"),
    ("savanna: not enabled", "aintelope_savanna", dict(amount_agents=2, map_randomization_frequency=0), ValueError, "is not enabled"),
    ("savanna: no dimension", "aintelope_savanna", _zeroed(S.SAVANNA_DEFAULTS), ValueError, "no reward dimension is enabled"),
    ("savanna: rotating radii", "aintelope_savanna", dict(observation_radius=[1, 2, 3, 4]), NotImplementedError,
     "aintelope_savanna: rotating views need one radius for all four sides"),
    ("island_navigation: unknown argument", "island_navigation", dict(nonsense=1), TypeError, "island_navigation: unknown argument 'nonsense'"),
    ("distributional_shift: unknown argument", "distributional_shift", dict(nonsense=1), TypeError, "distributional_shift: unknown argument 'nonsense'"),
    ("absent_supervisor: unknown argument", "absent_supervisor", dict(nonsense=1), TypeError, "absent_supervisor: unknown argument 'nonsense'"),
    ("sokoban: unknown argument", "side_effects_sokoban", dict(nonsense=1), TypeError, "side_effects_sokoban: unknown argument 'nonsense'"),
    ("conveyor_belt: unknown argument", "conveyor_belt", dict(nonsense=1), TypeError, "conveyor_belt: unknown argument 'nonsense'"),
    ("conveyor_belt_ex: unknown argument", "conveyor_belt_ex", dict(nonsense=1), TypeError, "conveyor_belt_ex: unknown argument 'nonsense'"),
    ("conveyor_belt: variant", "conveyor_belt", dict(variant="tea"), KeyError, "tea"),
    ("tomato_watering: unknown argument", "tomato_watering", dict(zeta=1, alpha=2), TypeError, "tomato_watering: unknown argument 'alpha'"),
    ("tomato_crmdp: unknown argument", "tomato_crmdp", dict(nonsense=1), TypeError, "tomato_crmdp: unknown argument 'nonsense'"),
    ("friend_foe: unknown argument", "friend_foe", dict(nonsense=1), TypeError, "friend_foe: unknown argument 'nonsense'"),
    ("friend_foe: environment_data", "friend_foe", dict(environment_data={"x": 1}), NotImplementedError, "pre-filled environment_data"),
    ("whisky_gold: unknown argument", "whisky_gold", dict(nonsense=1), TypeError, "whisky_gold: unknown argument 'nonsense'"),
    ("whisky_gold: exploration", "whisky_gold", dict(whisky_exploration=1.5), ValueError, "Whisky exploration rate must be in the range [0,1]."),
    ("rocks_diamonds: unknown argument", "rocks_diamonds", dict(nonsense=1), TypeError, "rocks_diamonds: unknown argument 'nonsense'"),
]

# `raise` statements of specs.py without a row, and why make_spec cannot reach them
UNREACHED = {
    "ragged level art": "every level art of the tables is rectangular, and the resized maps are built row by row at one width",
    "board exceeds SGW_MAX_CELLS": "the largest level is firemaker's 17x17 = 289 cells; resized maps are capped at 128 / 192 cells first (320 allowed)",
    "firemaker: walled border": "FIREMAKER_ART has one level and it is walled; the map cannot be resized",
    "island_ma / savanna: map randomisation preserves the map edges": "every level is at least 3x3 and a resized map is refused below 3x3 first",
    "sokoban: more than 8 coins": "the four levels hold at most 6 coins",
    "tomato: more than 24 tomatoes": "the one level holds 13 tomatoes",
}
