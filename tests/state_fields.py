"""The packed per-env state: every field narrower than 32 bits of every family's load / store (csrc/sgw_<family>.hpp), what keeps
its value inside the field, and the run that drives it to that limit.  No GPU here.

FIELDS: one row per (layout file, field): bits; `bound`, one of
  "max_iterations"  the field counts plays or visits, at most one per play: <= max_iterations <= 65535 (make_spec, sgw_create)
  "spec"            a refusal of make_spec / sgw_create keeps it in range: `refusal` names the test that pins the refusal
  "board"           a cell index, a row, a column or a distance on a board of at most SGW_MAX_CELLS cells with H, W <= 255
  "enum"            a handful of values of the family's own
  "wraps"           an episode counter that is only incremented and compared with its own kind: it wraps consistently
  "i16"             island_navigation_ex's packed satiations, availabilities and cumulative rewards: packable() proves the range
and `cases`, the ids of the CASES that drive it there (empty for the kinds nothing can drive).

CASES: one row per run.  name, kw (make_spec); oracle ("scalar", "ma", "ima", "sav"); n (envs: ragged, never a multiple of 64), T
(steps), tape (a TAPES builder); plays (plays of one step: frame advances by this much); crossings: the frame values whose
neighbourhood is compared step by step (255 / 256, 32767 / 32768 where the run gets there), next to the episode's end and 8
steps into the next episode; expect: end_frame (the frame every env's first episode ends on, after the full max_iterations)
and reach: (what, column, value, quantifier) conditions the oracle's run must show, so that the GPU comparison of
tests/test_state_fields_gpu.py cannot pass without having been at the limit; state_words where the case pins sgw_state_words.

oracle_case() runs a case through the C oracle in batches of envs and keeps only the compared steps (a whole savanna run of
65 543 steps x 67 envs would hold 16 GB): {(a, b): the oracle's arrays of steps a .. b}, and per env the step and frame of
the first episode's end, the metrics' maxima over it and the cumulative rewards and metrics at its end."""
import numpy as np

from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import ALL_OUTPUTS
from tests import launch_paths as LP

MAX_IT = 65535
WINDOW = 24                    # steps compared on either side of a crossing: windows of 49 steps
TAIL = 8                       # steps compared into the next episode
BULK = 4096                    # steps of one call between windows: its last row is compared
FM_SEED = 0xF1E                # the uniform Philox tape of tests/test_firemaker_gpu.py

# island_navigation_ex level 9 from the start cell (2, 2): stay on the gap; LEFT onto S; UP RIGHT RIGHT onto D; DOWN DOWN RIGHT
# onto F; UP RIGHT RIGHT RIGHT DOWN DOWN RIGHT (over D) onto G -- then NOOP.  MO actions: LEFT 1 RIGHT 2 UP 3 DOWN 4.
ISLAND_L9_PARKING = ((), (1,), (3, 2, 2), (4, 4, 2), (3, 2, 2, 2, 4, 4, 2))

SATURATING = dict(MOVEMENT_REWARD={"MOVEMENT_REWARD": -50},
                  GAP_REWARD={"FOOD_REWARD": 50, "DRINK_REWARD": -50, "GOLD_REWARD": 50, "SILVER_REWARD": -50},
                  DRINK_DEFICIENCY_REWARD={"DRINK_DEFICIENCY_REWARD": -50}, FOOD_DEFICIENCY_REWARD={"FOOD_DEFICIENCY_REWARD": 50})
# packable() bounds a dimension's step by |tile reward| + |gap reward| (20 + 50, 40 + 50, 30 + 50 with the default tile rewards:
# 70 * 655 > 32767; a tile reward of 0 would disable its dimension and make_spec refuse the gap reward on it), so the
# saturating flags run the plain state at 655 already.  Without GAP_REWARD the three remaining dimensions (movement and the two
# deficiencies: 50 * 655 = 32750 < 32767) pack.
SATURATING_PACKED = {k: v for k, v in SATURATING.items() if k != "GAP_REWARD"}
SATURATED_DIMS = ("DRINK_DEFICIENCY_REWARD", "DRINK_REWARD", "FOOD_DEFICIENCY_REWARD", "FOOD_REWARD", "GOLD_REWARD", "MOVEMENT_REWARD",
                  "SILVER_REWARD")
SATURATED_SIGNS = (-1, -1, 1, 1, 1, -1, -1)
SATURATED_WITHOUT_GAP = ("DRINK_DEFICIENCY_REWARD", "FOOD_DEFICIENCY_REWARD", "MOVEMENT_REWARD")


# ---- tapes: int8 [E, T(, A)] ------------------------------------------------------------------------------------------------------
def _tape_noop(case, spec):
  """NOOP.  odd: agent 1 submits nothing in the first round, so a two-agent frame runs over the odd numbers and ends on
  max_iterations + 1; idle: that many rounds after the episode's end in which nobody submits anything (no play, no reset: the
  frame stands), before the round that starts the next episode."""
  acts = np.zeros((case["n"], case["T"]) + ((spec.A,) if spec.A > 1 else ()), np.int8)
  if case.get("odd"):
    acts[:, 0, 1] = -1
  end = end_step(case)
  acts[:, end:end + case.get("idle", 0)] = -1
  return acts


def _tape_island_parking(case, spec):
  acts = np.zeros((case["n"], case["T"]), np.int8)
  for e in range(case["n"]):
    p = ISLAND_L9_PARKING[e % 5]
    acts[e, :len(p)] = p
  return acts


def _tape_cycle(case, spec):
  return np.tile(np.resize(np.array(case["cycle"], np.int8), case["T"]), (case["n"], 1))


def _tape_philox(case, spec):
  per = [philox.actions(FM_SEED, np.arange(case["n"]), np.arange(case["T"]), spec.action_lo, spec.n_actions, agent=a) for a in range(spec.A)]
  acts = per[0] if spec.A == 1 else np.stack(per, axis=-1)                  # [T, E(, A)]
  acts = np.ascontiguousarray(np.moveaxis(acts, 0, 1))
  for a in case.get("withheld", ()):
    acts[:, :, a] = -1                                                      # the agent submits nothing: the round plays the others
  return acts


TAPES = dict(noop=_tape_noop, island_parking=_tape_island_parking, cycle=_tape_cycle, philox=_tape_philox)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _case(id, name, kw, oracle, n, T, tape, end_frame, reach, plays=1, crossings=(255, 32767), outs=ALL_OUTPUTS, rng=False,
          bits=None, rand=None, state_words=None, plain_too=False, countdown=False, **more):
  return dict(id=id, name=name, kw=kw, oracle=oracle, n=n, T=T, tape=tape, plays=plays, crossings=crossings, outs=outs, rng=rng,
              bits=bits, rand=rand, state_words=state_words, plain_too=plain_too, countdown=countdown,
              expect=dict(end_frame=end_frame, reach=reach), **more)


def _island_cases():
  out = [_case("island_l9_65535", "island_navigation_ex", dict(level=9, max_iterations=MAX_IT), "scalar", 131, MAX_IT + TAIL,
               "island_parking", MAX_IT,
               [("metric_max", v, 65500, "some>=") for v in ("GapVisits", "DrinkVisits", "FoodVisits", "GoldVisits", "SilverVisits")] +
               [("metric_end", "GapVisits", MAX_IT, "some=="), ("metric_min", "DrinkSatiation", -MAX_IT, "some=="),
                ("metric_min", "FoodSatiation", -MAX_IT, "some==")], state_words=22)]
  for tag, kw, words in (("default", {}, (10, 22)), ("saturating", SATURATING, (22, 22)), ("saturating_packed", SATURATING_PACKED, (10, 22))):
    for mi, w in zip((655, 656), words):
      sat = tag != "default"
      reach = [("cum_end", d, s * 50.0 * mi, "all==") for d, s in zip(SATURATED_DIMS, SATURATED_SIGNS)
               if "GAP_REWARD" in kw or d in SATURATED_WITHOUT_GAP] if sat else \
          [("cum_end", "MOVEMENT_REWARD", -1.0 * mi, "all=="), ("metric_end", "DrinkSatiation", -1.0 * mi, "all==")]
      out.append(_case("island_%s_%d" % (tag, mi), "island_navigation_ex", dict(level=9, max_iterations=mi, **kw), "scalar", 131,
                       mi + TAIL, "cycle", mi, reach, crossings=(255,), state_words=w, plain_too=(w == 10), cycle=(3, 4)))
  return out


def _firemaker_cases():
  out = []
  for d in (3, 254, 255, 300, 1000):       # 700 rounds of three plays: the first episode ends after round 234 on frame 702
    out.append(_case("firemaker_duration_%d" % d, "firemaker_ex_ma",
                     dict(amount_agents=3, max_iterations=700, STOP_BUTTON_PRESS_EFFECT_DURATION=d), "ma", 131, 700, "philox", 702,
                     [("metric_max", "StopButtonPressCountdown", d + 1.0, "all==")],       # reload - 1, in every env
                     plays=3, crossings=(), outs=LP.WIN, rng=True, countdown=True, every_step=True,
                     checkpoint=237))      # 3 rounds into the second episode: with a duration of 255, 17 envs' countdowns are at 256
  # a whole run at max_iterations = 65535 takes the oracle 15 s for 65 envs: 32769, so that frame and visits still cross 32767 / 32768
  out.append(_case("firemaker_32769", "firemaker_ex_ma", dict(amount_agents=3, max_iterations=32769), "ma", 65, 10923 + TAIL, "philox",
                   32769, [("metric_max", "ExternalVisits_1", 1000, "some>=")], plays=3, outs=LP.WIN, rng=True))
  out.append(_case("firemaker_32769_withheld", "firemaker_ex_ma", dict(amount_agents=3, max_iterations=32769), "ma", 65, 16385 + TAIL,
                   "philox", 32770, [("metric_max", "ExternalVisits_1", 1000, "some>=")], plays=2, outs=LP.WIN, rng=True, withheld=(1,)))
  return out


def _multi_agent_cases():
  """A round of A plays ends the episode on up to max_iterations + A - 1, so make_spec and sgw_create take max_iterations <= 65535
  - (A - 1): at 65535 a two-agent episode ended on frame 65536, stored as 0, and the idle rounds after the end (nobody submits:
  no play, no reset, the frame stands) reported frame 0 from the step path against 65536 from the oracle and the fused path.
  The two-agent cases run max_iterations = 65534 over the odd frames (agent 1 sits out the first round): the episode ends on
  65535, the largest frame the field holds, and three idle rounds read it back."""
  two = dict(plays=2, rng=True, idle=3, odd=True)
  return [
      _case("island_ma_65534_odd", "island_navigation_ex_ma", dict(level=9, max_iterations=MAX_IT - 1), "ima", 67, 32768 + TAIL, "noop", MAX_IT,
            [("metric_max", "GapVisits_1", 32768, "all=="), ("metric_max", "GapVisits_2", 32767, "all==")], outs=LP.WIN, **two),
      _case("savanna_1_65535", "aintelope_savanna", dict(amount_agents=1, max_iterations=MAX_IT), "sav", 67, MAX_IT + TAIL, "noop", MAX_IT,
            [("metric_max", 0, MAX_IT, "all==")], outs=LP.SAV, rng=True, idle=3),
      _case("savanna_2_65534_odd", "aintelope_savanna", dict(amount_agents=2, amount_predators=0, max_iterations=MAX_IT - 1), "sav", 67,
            32768 + TAIL, "noop", MAX_IT, [("metric_max", 0, 32768, "all==")], outs=LP.SAV, **two),
  ]


def _scalar_cases():
  """One family per remaining layout file.  The reference's boat_race(_ex), safe_interruptibility(_ex), conveyor_belt(_ex) and
  island_navigation take max_iterations: NOOP, or bumping the wall next to the start cell where the action range starts at 1.
  side_effects_sokoban, tomato_*, rocks_diamonds, whisky_gold and friend_foe take none: their episodes end at the
  reference's own 100 plays."""
  rows = [("boat_race_ex", dict(level=1), (0,), None), ("island_navigation", dict(level=0), (0,), None),
          ("safe_interruptibility", dict(level=0), (1,), "array"), ("conveyor_belt", dict(variant="sushi"), (1,), None)]
  out = [_case(name + "_65535", name, dict(max_iterations=MAX_IT, **kw), "scalar", 131, MAX_IT + TAIL, "cycle", MAX_IT, [], bits=bits,
               cycle=cycle) for name, kw, cycle, bits in rows]
  # the families without max_iterations: kept alive to the reference's frame 100, the longest reachable (action 1 bumps a wall
  # or walks into one and stays; tomato_watering and rocks_diamonds end nowhere else, so a uniform tape does)
  fixed = [("side_effects_sokoban", dict(level=0), "cycle", None), ("tomato_watering", dict(), "philox", "array"),
           ("rocks_diamonds", dict(level=1), "philox", None), ("whisky_gold", dict(human_player=False), "cycle", "array"),
           ("friend_foe", dict(bandit_type="friend"), "cycle", "array")]
  out += [_case(name + "_100", name, kw, "scalar", 131, 100 + TAIL, tape, 100, [], crossings=(), rand=rand, cycle=(1,))
          for name, kw, tape, rand in fixed]
  return out


CASES = _island_cases() + _firemaker_cases() + _multi_agent_cases() + _scalar_cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- the fields -------------------------------------------------------------------------------------------------------------------
def _field(layout, field, bits, bound, why, cases=(), refusal=None):
  return dict(layout=layout, field=field, bits=bits, bound=bound, why=why, cases=tuple(cases), refusal=refusal)


LONG = dict(sgw_island=("island_l9_65535",), sgw_boat=("boat_race_ex_65535",), sgw_tile=("island_navigation_65535",),
            sgw_safeint=("safe_interruptibility_65535",), sgw_conveyor=("conveyor_belt_65535",),
            sgw_firemaker=("firemaker_32769", "firemaker_32769_withheld"), sgw_island_ma=("island_ma_65534_odd",),
            sgw_savanna=("savanna_1_65535", "savanna_2_65534_odd"))
FIXED = dict(sgw_sokoban=("side_effects_sokoban_100",), sgw_tomato=("tomato_watering_100",), sgw_rocks=("rocks_diamonds_100",),
             sgw_whisky=("whisky_gold_100",), sgw_friendfoe=("friend_foe_100",))
NO_MAX_IT = "the reference's env takes no max_iterations: its episodes end after its own 100 plays, the longest frame reachable"
SCALAR_LAYOUTS = ("sgw_island", "sgw_boat", "sgw_tile", "sgw_safeint", "sgw_sokoban", "sgw_conveyor", "sgw_tomato", "sgw_rocks", "sgw_whisky",
                  "sgw_friendfoe")
LAYOUTS = SCALAR_LAYOUTS + ("sgw_firemaker", "sgw_island_ma", "sgw_savanna")


def _fields():
  out = []
  for lay in LAYOUTS:
    multi = lay in ("sgw_firemaker", "sgw_island_ma", "sgw_savanna")
    if lay in LONG:
      why = "frame counts plays; the episode ends once frame >= max_iterations <= 65535"
      if multi:
        why += ("; a round of A plays ends on up to max_iterations + A - 1, and the idle rounds after the end read the stored frame: "
                "max_iterations <= 65535 - (A - 1)")
      out.append(_field(lay, "frame", 16, "max_iterations", why, LONG[lay], refusal="test_max_iterations_above_the_frame_field_is_refused"))
    else:
      out.append(_field(lay, "frame", 16, "max_iterations", NO_MAX_IT, FIXED[lay],
                        refusal="test_max_iterations_above_the_frame_field_is_refused"))
    out.append(_field(lay, "step_type", 4, "enum", "FIRST / MID / LAST and the per-agent variants: < 16"))
    out.append(_field(lay, "term_reason", 4, "enum", "SGW_* termination reasons, 15 = none"))
    if not multi:
      out.append(_field(lay, "row, col", 8, "board", "H, W <= 255 (sgw_create)", refusal="test_board_over_the_cell_limit_is_refused"))
      out.append(_field(lay, "actual_action + 1", 8, "enum", "the action range and QUIT (9): < 255"))
  out += [
      _field("sgw_island", "safety", 8, "board", "Manhattan distance to water, 99 without water: < H + W"),
      _field("sgw_island", "gap_v, drink_v, food_v, gold_v, silver_v", 16, "max_iterations", "one visit per play at most", LONG["sgw_island"]),
      _field("sgw_island", "episode", 32, "wraps", "only incremented and compared"),
      _field("sgw_island", "drink_sat, food_sat, d_avail, f_avail (packed)", 16, "i16",
             "packable(): |initial| + max_iterations * (|rate| + |extraction|) < 32767, growth limit < 32767",
             ("island_default_655", "island_default_656")),
      _field("sgw_island", "cumulative[12] (packed)", 16, "i16", "packable(): max_iterations * the largest step of the dimension < 32767",
             ("island_saturating_packed_655", "island_saturating_packed_656", "island_saturating_655", "island_saturating_656",
              "island_default_655", "island_default_656")),
      _field("sgw_boat", "episode", 16, "wraps", "only incremented and compared with itself"),
      _field("sgw_tile", "safety", 8, "board", "distance on the board"),
      _field("sgw_sokoban", "coins", 8, "spec", "one bit per coin", refusal="test_sokoban_over_its_coin_and_box_fields_is_refused"),
      _field("sgw_sokoban", "pen", 6, "spec", "two bits per box, three boxes", refusal="test_sokoban_over_its_coin_and_box_fields_is_refused"),
      _field("sgw_sokoban", "brow[3], bcol[3]", 8, "board", "H, W <= 255", refusal="test_board_over_the_cell_limit_is_refused"),
      _field("sgw_tomato", "tomato mask", 24, "spec", "one bit per tomato", refusal="test_tomato_over_its_mask_is_refused"),
      _field("sgw_conveyor", "orow, ocol, old_r, old_c", 8, "board", "H, W <= 255"),
      _field("sgw_rocks", "lr[], lc[]", 8, "board", "rows and columns of the rocks and diamonds: H, W <= 255"),
      _field("sgw_firemaker", "countdown", 16, "spec", "reload - 1 at most; reload = 1 + 1 + STOP_BUTTON_PRESS_EFFECT_DURATION <= 65535",
             ["firemaker_duration_%d" % d for d in (3, 254, 255, 300, 1000)], refusal="test_firemaker_countdown_over_its_field_is_refused"),
      _field("sgw_firemaker", "n_ext", 16, "board", "burning cells outside the territory: <= 289"),
      _field("sgw_firemaker", "visits[15]", 16, "max_iterations", "one visit per play at most", LONG["sgw_firemaker"]),
      _field("sgw_firemaker", "row[3], col[3]", 8, "board", "17 x 17"),
      _field("sgw_firemaker", "dirs", 12, "enum", "six directions of 2 bits"),
      _field("sgw_firemaker", "episode", 32, "wraps", "only incremented"),
      _field("sgw_island_ma", "gap_v, drink_v, food_v, gold_v, silver_v [2]", 16, "max_iterations", "one visit per play of the agent", LONG["sgw_island_ma"]),
      _field("sgw_island_ma", "row[2], col[2]", 8, "board", "H * W <= 128"),
      _field("sgw_island_ma", "episode_no, map_episode", 16, "wraps", "incremented and compared with each other only"),
      _field("sgw_savanna", "vis, stepc", 16, "max_iterations", "one per play of the agent", LONG["sgw_savanna"]),
      _field("sgw_savanna", "row[2], col[2], saf, saf2", 8, "board", "H * W <= 192"),
      _field("sgw_savanna", "episode_no, map_episode", 16, "wraps", "incremented and compared with each other only"),
  ]
  return out


FIELDS = _fields()


# ---- the plan of a run ------------------------------------------------------------------------------------------------------------
def end_step(case):
  """The step after which every env's first episode has ended."""
  return -(-case["expect"]["end_frame"] // case["plays"])


def windows(case):
  """Sorted, disjoint (a, b) step ranges (1-based, inclusive) compared row by row."""
  T = case["T"]
  if case.get("every_step"):
    return [(a, min(a + 63, T)) for a in range(1, T + 1, 64)]
  end = end_step(case)
  spans = [(max(1, -(-f // case["plays"]) - WINDOW), -(-f // case["plays"]) + WINDOW) for f in case["crossings"] if f + 64 < case["expect"]["end_frame"]]
  spans.append((max(1, end - 40), min(T, end + TAIL)))
  out = []
  for a, b in sorted(spans):
    if out and a <= out[-1][1]:
      out[-1] = (out[-1][0], max(b, out[-1][1]))
    else:
      out.append((a, b))
  assert all(b - a < 64 for a, b in out) and out[-1][1] == T
  return out


def segments(case):
  """[(a, b, every)] covering steps 1 .. T in order: the windows (every step written) and calls of at most BULK steps between
  them (the last row written)."""
  out, t = [], 1
  for a, b in windows(case):
    while t < a:
      out.append((t, min(t + BULK - 1, a - 1), False))
      t = out[-1][1] + 1
    out.append((a, b, True))
    t = b + 1
  cp = checkpoint_step(case)              # a call ends on the checkpoint step
  return [p for a, b, every in out for p in (((a, cp, every), (cp + 1, b, every)) if a <= cp < b else ((a, b, every),))]


def checkpoint_step(case):
  """The step after which the state is snapshotted: one step before the end of the first episode, or the case's own."""
  return case.get("checkpoint", end_step(case) - 1)


def compared(case):
  """The (a, b) step ranges of segments() that are compared with the oracle."""
  return [(a, b) if every else (b, b) for a, b, every in segments(case)]


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
_BATCH = dict(scalar=33, ma=17, ima=34, sav=9)
_ORACLE = {}


def spec_of(case):
  from ai_safety_gridworlds_amd.specs import make_spec
  return make_spec(case["name"], **case["kw"])


def inputs(case, spec):
  """LP.inputs() of the case; the firemaker cases take the generators of tests/test_firemaker_gpu.py (5000 + env)."""
  inp = LP.inputs(case, spec, list(BY_ID).index(case["id"]))
  if case["oracle"] == "ma":
    from oracle import oracle_ma as OM
    inp["rng"] = np.stack([OM.rng_state_words(5000 + e) for e in range(case["n"])])
  return inp


def actions(case, spec):
  return TAPES[case["tape"]](case, spec)


def _column(names, key):
  return key if isinstance(key, int) else list(names).index(key)


def oracle_case(case, nthreads=8):
  """dict(want={(a, b): arrays}, end_step=[E], end_frame=[E], metric_max / metric_min / metric_end=[E, M], cum_end=[E, A*K],
  metric_names, dim_names, countdown=[E, T + 1] for the countdown cases, seconds)."""
  import time
  if case["id"] in _ORACLE:
    return _ORACLE[case["id"]]
  spec = spec_of(case)
  inp, acts = inputs(case, spec), actions(case, spec)
  E, off = case["n"], LP.resets(case) - 1
  spans = compared(case)
  parts = {k: [] for k in ("end_step", "end_frame", "metric_max", "metric_min", "metric_end", "cum_end", "countdown")}
  want = {s: [] for s in spans}
  t0 = time.time()
  for e0 in range(0, E, _BATCH[case["oracle"]]):
    e1 = min(E, e0 + _BATCH[case["oracle"]])
    sub = dict(inp)
    for k in ("bits_oracle", "rand_oracle", "rng"):
      sub[k] = None if inp[k] is None else inp[k][e0:e1]
    w = LP.run_oracle(case, np.moveaxis(acts[e0:e1], 0, 1), sub, nthreads=nthreads)
    arrays = {k: v for k, v in w.items() if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == e1 - e0}
    st = arrays["step_type"][:, off:]
    st = st.reshape(st.shape[0], st.shape[1], -1)
    if case.get("withheld"):
      st = np.delete(st, list(case["withheld"]), axis=2)
    done = (st == 2).all(axis=2)
    assert done.any(axis=1).all(), "%s: an env's first episode never ends" % case["id"]
    end = done.argmax(axis=1)
    rows = np.arange(e1 - e0)
    met, cum = arrays["metrics"][:, off:], arrays["cumulative"][:, off:]
    last = np.full_like(end, met.shape[1]) if case["countdown"] else end        # the countdown cases: maxima over the whole run
    alive = np.arange(met.shape[1])[None, :, None] <= last[:, None, None]
    parts["end_step"].append(end)
    parts["end_frame"].append(arrays["frame"][:, off:][rows, end])
    parts["metric_max"].append(np.nanmax(np.where(alive, met, -np.inf), axis=1) if met.shape[2] else met[:, 0])
    parts["metric_min"].append(np.nanmin(np.where(alive, met, np.inf), axis=1) if met.shape[2] else met[:, 0])
    parts["metric_end"].append(met[rows, end])
    parts["cum_end"].append(cum[rows, end].reshape(e1 - e0, -1))
    if case["countdown"]:
      parts["countdown"].append(met[..., 15].copy())
    for (a, b) in spans:            # scalar / ma: index = step; ima / sav: LP.oracle_mismatches reads [s0 + 1, s0 + 1 + S) with s0 = 0
      want[(a, b)].append({k: v[:, a:b + 1].copy() if not off else v[:, a:b + 2].copy() for k, v in arrays.items()})
    meta = {k: v for k, v in w.items() if k not in arrays}
  out = {k: np.concatenate(v) for k, v in parts.items() if v}
  out["want"] = {s: dict(meta, **{k: np.concatenate([p[k] for p in ps]) for k in ps[0]}) for s, ps in want.items()}
  out["metric_names"], out["dim_names"] = list(spec.metric_names), list(spec.dim_names)
  out["seconds"] = time.time() - t0
  _ORACLE[case["id"]] = out
  return out


def reached(case, o):
  """The failed conditions of case["expect"] on an oracle_case() result (empty: the tape does what the row claims)."""
  bad = []
  E = case["n"]
  if not (o["end_step"] == end_step(case)).all():
    bad.append("%d envs end their first episode before step %d" % ((o["end_step"] != end_step(case)).sum(), end_step(case)))
  if not (o["end_frame"] == case["expect"]["end_frame"]).all():
    bad.append("end frames %s, not %d" % (sorted(set(o["end_frame"].tolist()))[:5], case["expect"]["end_frame"]))
  for what, key, value, quant in case["expect"]["reach"]:
    names = o["dim_names"] if what == "cum_end" else o["metric_names"]
    v = o[what][:, _column(names, key)]
    if what == "cum_end" and case["oracle"] != "scalar":
      raise NotImplementedError("cum_end conditions are stated for the single-agent oracle")
    ok = dict([("all==", (v == value).all()), ("some==", (v == value).any()), ("some>=", (v >= value).any())])[quant]
    if not ok:
      bad.append("%s[%s] %s %r fails: %s .. %s over %d envs" % (what, key, quant, value, v.min(), v.max(), E))
  return bad
