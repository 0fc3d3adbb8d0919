"""The rows of tests/seeded_draws.py can fail (CPU, the C oracle alone): a row whose run draws nothing, or whose drawn numbers
never reach an output, would pass tests/test_seeded_draws_gpu.py whatever the kernel keyed its Philox draws by.  For every row,
at the run length of the GPU path test (calls x 16 steps), the oracle is fed the correct restated streams and the streams a
wrong kernel would draw, and enough envs must differ: at least one finished episode; for the rand rows, at least half of the
envs under the two uniforms of every Philox block swapped; for the seeded rows, at least half of the envs keyed from base 0,
and where the row straddles env id 2^32 at least half of the envs at or past 2^32 with the high id word dropped (and none below).
whisky_human takes each of the four replacement directions, and friendfoe_random each bandit type, at least 100 times.
"Half" and "100" are conditions on the rows, not measurements: a row that misses one gets other kwargs, another seed or size.

Observed (finished episodes; envs differing of n):
  dshift_seeded      777 x 64    1810 finished   base 0: 663   high word dropped: 240 of 277 past 2^32, 0 below
  absent_seeded      1011 x 64   1243 finished   base 0: 730
  safeint_seeded     1013 x 48   3039 finished   base 0: 946   high word dropped: 677 of 713, 0 below
  friendfoe_random   1023 x 48   1660 finished   base 0: 929   high word dropped: 484 of 523, 0 below   swap: 844
                                 bandit types drawn (friend / neutral / adversary): 888 / 896 / 864
  friendfoe_neutral  1029 x 64   2301 finished   base 0: 710   swap: 561   (at 48 steps the swap reaches only 477 envs: one draw
                                 per episode, a swapped pair changes the rewarding box with probability 2 x 0.6 x 0.4, and it shows
                                 only when a box is opened -- hence the fourth call)
  whisky_human       1025 x 48   479 finished    base 0: 924   high word dropped: 474 of 525, 0 below   swap: 919
                                 replaced steps by direction: 5219 / 5241 / 5239 / 5290
  tomato_seeded      1019 x 112  1019 finished   base 0: 1019  high word dropped: 519 of 519, 0 below   swap: 1019
  whisky_human_array 333 x 48    140 finished    swap: 297     replaced steps by direction: 1862 / 1788 / 1880 / 1740
"""
import numpy as np
import pytest

from tests import launch_paths as LP
from tests import seeded_draws as SD

IDS = [r["id"] for r in SD.ROWS]
_V = {}


def variants(row_id):
  if row_id not in _V:
    _V[row_id] = SD.variants(SD.BY_ID[row_id])
  return _V[row_id]


def test_the_table_holds_the_required_rows_and_groups():
  want = dict(dshift_seeded=("distributional_shift", "bits", SD.B32 - 500), absent_seeded=("absent_supervisor", "bits", 777777),
              safeint_seeded=("safe_interruptibility", "bits", SD.B32 - 300), friendfoe_random=("friend_foe", "rand", SD.B32 - 500),
              friendfoe_neutral=("friend_foe", "rand", 123457), whisky_human=("whisky_gold", "rand", SD.B32 - 500),
              tomato_seeded=("tomato_watering", "rand", SD.B32 - 500))
  for rid, (name, kind, base) in want.items():
    r = SD.BY_ID[rid]
    assert (r["name"], r[kind], r["base"]) == (name, "philox", base), rid
  assert SD.BY_ID["tomato_seeded"]["calls"] == 7
  assert len(SD.BY_ID) == len(SD.ROWS) and not set(SD.BY_ID) & set(LP.BY_ID), "row ids are unique across both tables"
  assert all(r["n"] % 64 for r in SD.ROWS), "every n is ragged"
  members = [m for _, ms in SD.GROUPS for m in ms]
  assert sorted(members) == sorted(r["id"] for r in SD.ROWS if r["tag"]), "every member row is in exactly one group"
  for gid, ms in SD.GROUPS:
    assert 2 <= len(ms) <= 4 and len({SD.BY_ID[m]["base"] for m in ms}) > 1, "%s: members at different bases" % gid
  assert any(sum(SD.straddles(SD.BY_ID[m]) for m in ms) >= 2 for _, ms in SD.GROUPS), "one group has two members straddling 2^32"


def test_the_rows_that_draw_nothing_have_a_drawing_complement():
  """launch_paths' friend_foe row fixes the bandit (P_FIXED >= 0: no type draw, argmax) and its whisky_gold row has no human
  player (the replacement block is dead): seeded_draws must hold rows of the same env names that draw."""
  ff, wg = LP.BY_ID["friend_foe"], LP.BY_ID["whisky_gold"]
  assert ff["kw"].get("bandit_type") == "friend" and not wg["kw"].get("human_player"), "the rows draw now: update this test"
  assert any(r["name"] == "friend_foe" and not r["kw"].get("bandit_type") for r in SD.ROWS), "no friend_foe row draws the bandit type"
  assert any(r["name"] == "friend_foe" and r["kw"].get("bandit_type") == "neutral" for r in SD.ROWS), "no neutral friend_foe row"
  assert any(r["name"] == "whisky_gold" and r["kw"].get("human_player") and r["kw"].get("whisky_exploration", 0.9) > 0
             and r["rand"] == "philox" for r in SD.ROWS), "no whisky_gold row with a human player"


@pytest.mark.parametrize("row_id", IDS)
def test_an_episode_ends_inside_the_run(row_id):
  c = variants(row_id)["correct"]
  assert LP.finished_returns(c["step_type"][..., None], c["cumulative"])[-1] > 0


@pytest.mark.parametrize("row_id", [r["id"] for r in SD.ROWS if r["rand"]])
def test_outputs_depend_on_the_order_of_a_philox_pair(row_id):
  v = variants(row_id)
  n = int(SD.envs_differing(v["correct"], v["swap"]).sum())
  print("%s: %d of %d envs differ with the pair swapped" % (row_id, n, SD.BY_ID[row_id]["n"]))
  assert 2 * n >= SD.BY_ID[row_id]["n"]


@pytest.mark.parametrize("row_id", [r["id"] for r in SD.ROWS if SD.seeded(r)])
def test_outputs_depend_on_the_global_env_id(row_id):
  row, v = SD.BY_ID[row_id], variants(row_id)
  n = int(SD.envs_differing(v["correct"], v["base0"]).sum())
  print("%s: %d of %d envs differ keyed from base 0" % (row_id, n, row["n"]))
  assert 2 * n >= row["n"]
  assert SD.straddles(row) == ("nohigh" in v)
  if SD.straddles(row):
    d = SD.envs_differing(v["correct"], v["nohigh"])
    hi = LP.global_ids(row["n"], row["base"]) >= np.uint64(SD.B32)
    print("%s: %d of %d envs past 2^32 differ with the high id word dropped" % (row_id, d[hi].sum(), hi.sum()))
    assert 2 * int(d[hi].sum()) >= int(hi.sum())
    assert not d[~hi].any(), "an env below 2^32 depends on the high id word"


@pytest.mark.parametrize("row_id", ["whisky_human", "whisky_human_array"])
def test_whisky_takes_every_replacement_direction(row_id):
  row, v = SD.BY_ID[row_id], variants(row_id)
  count, actual = SD.whisky_replacements(v["correct"], v["actions"], v["rand"], row["kw"]["whisky_exploration"])
  played = actual >= 0
  assert np.array_equal(v["correct"]["actual_action"][:, 1:][played], actual[played]), "the restated draws are not the oracle's"
  print("%s: replaced steps by direction %s" % (row_id, count.tolist()))
  assert count.min() >= 100


def test_friend_foe_draws_every_bandit_type():
  v = variants("friendfoe_random")
  count, builds = SD.friendfoe_builds(v["correct"], v["rand"])
  assert all(v["correct"]["safety"][e, t] == bt for e, t, bt in builds), "the restated draws are not the oracle's"
  print("friendfoe_random: bandit types drawn %s" % count.tolist())
  assert count.min() >= 100


def test_a_base_of_zero_leaves_the_inputs_as_they_were():
  """LP.inputs' default base: the seeded streams of the two seeded rows of launch_paths.ROWS, restated as before the base
  existed (local ids, <= interruption_probability)."""
  from ai_safety_gridworlds_amd import philox
  from ai_safety_gridworlds_amd.specs import make_spec
  for rid in ("safe_interruptibility_ex", "tomato_crmdp"):
    row = LP.BY_ID[rid]
    spec = make_spec(row["name"], **row["kw"])
    d = LP.inputs(row, spec, 5)
    ids = np.arange(row["n"])
    if row["bits"]:
      w = (philox.episode_uniform(1005, ids[:, None], np.arange(LP.N_BITS)[None, :]) <= spec.config["interruption_probability"])
      assert d["bits_seed"] == 1005 and d["bits_oracle"].dtype == np.uint8 and np.array_equal(d["bits_oracle"], w.astype(np.uint8))
    else:
      assert d["rand_seed"] == 2005 and np.array_equal(d["rand_oracle"], LP.philox_uniforms(2005, ids, LP.N_RAND))
