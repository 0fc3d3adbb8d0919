"""Rows for the families that draw random numbers, in seeded mode (the kernel's own Philox, keyed by seed, GLOBAL env id and the
episode / draw counter) and away from env id 0: every row has a `base` (the engine's env_id_base), most of them so that the
envs straddle id 2^32 -- the high id word goes into Philox counter word 3 in synth_action, episode_uniform, philox_pair and
tomato_watering's own two-per-call path.  tests/launch_paths.py's `friend_foe` and `whisky_gold` rows draw nothing (a fixed
friend bandit; human_player=False); friendfoe_random / friendfoe_neutral / whisky_human(_array) here do.

ROWS are launch_paths rows (LP._row) with two more keys: `base`, and `seed` (LP.inputs' seed: bit seed 1000 + seed, stream seed
2000 + seed).  tests/test_seeded_draws_gpu.py runs them through the whole launch-path matrix, and every row of both tables
through the sharding test; tests/test_seeded_draws.py (CPU, the oracle alone) asserts that each row CAN fail:

variants(row): the oracle's records of the row's run under the correct restated streams and under the streams a wrong kernel
would draw -- "base0" (keyed by the local env), "nohigh" (the high id word dropped), "swap" (the two uniforms of every Philox
block exchanged).  Only the drawn streams change; the actions stay those of the global ids."""
import numpy as np

from tests import launch_paths as LP

B32 = 1 << 32
ROWS = [
    dict(LP._row("dshift_seeded", "distributional_shift", dict(is_testing=True), 777, "TAG_TILE", bits="philox", calls=4),
         base=B32 - 500, seed=1),
    dict(LP._row("absent_seeded", "absent_supervisor", dict(), 1011, "TAG_TILE", bits="philox", calls=4), base=777777, seed=1),
    dict(LP._row("safeint_seeded", "safe_interruptibility", dict(level=1, max_iterations=12), 1013, "TAG_SAFEINT", bits="philox"),
         base=B32 - 300, seed=1),
    dict(LP._row("friendfoe_random", "friend_foe", dict(), 1023, "TAG_FRIEND_FOE", rand="philox"), base=B32 - 500, seed=1),
    dict(LP._row("friendfoe_neutral", "friend_foe", dict(bandit_type="neutral"), 1029, "TAG_FRIEND_FOE", rand="philox", calls=4),
         base=123457, seed=1),
    dict(LP._row("whisky_human", "whisky_gold", dict(human_player=True, whisky_exploration=0.7), 1025, "TAG_WHISKY", rand="philox"),
         base=B32 - 500, seed=1),
    dict(LP._row("tomato_seeded", "tomato_watering", dict(), 1019, "TAG_TOMATO", rand="philox", calls=7), base=B32 - 500, seed=1),
    dict(LP._row("whisky_human_array", "whisky_gold", dict(human_player=True, whisky_exploration=0.7), 333, "TAG_WHISKY", rand="array"),
         base=65, seed=1),
]
BY_ID = {r["id"]: r for r in ROWS}

# every row once; g4_bases: four different bases, two members (distributional_shift, safe_interruptibility) straddle 2^32 at
# different offsets; g4_rand: the rand-stream families next to a bit family, three members straddling 2^32
GROUPS = [
    ("g4_bases", ["dshift_seeded", "safeint_seeded", "friendfoe_neutral", "whisky_human_array"]),
    ("g4_rand", ["absent_seeded", "friendfoe_random", "whisky_human", "tomato_seeded"]),
]

FIELDS = LP.SCALAR_FIELDS


def seeded(row):
  return "philox" in (row["bits"], row["rand"])


def straddles(row):
  return row["base"] < B32 < row["base"] + row["n"]


def run_steps(row):
  """The run length of the GPU path test: the row's calls of T steps."""
  return row["calls"] * LP.T


def variants(row, which=("correct", "base0", "nohigh", "swap")):
  """{variant: the oracle's arrays [E, run_steps + 1, ...]} for the variants that apply to the row, + "actions" [T, E] and
  "rand" (the correct uniforms the oracle read, or None)."""
  from ai_safety_gridworlds_amd.specs import make_spec
  spec = make_spec(row["name"], **row["kw"])
  ids = LP.global_ids(row["n"], row["base"])
  acts = LP.host_actions(spec, ids, np.arange(run_steps(row)), LP.SEED)
  inp = LP.inputs(row, spec, row["seed"], base=row["base"])
  out = dict(actions=acts, rand=inp["rand_oracle"], spec=spec)
  for v in which:
    d = dict(inp)
    if v == "base0" and seeded(row):
      LP.restate_seeded(row, spec, d, LP.global_ids(row["n"], 0))
    elif v == "nohigh" and seeded(row) and straddles(row):
      LP.restate_seeded(row, spec, d, ids & np.uint64(0xFFFFFFFF))
    elif v == "swap" and row["rand"]:
      u = inp["rand_oracle"]
      d["rand_oracle"] = np.ascontiguousarray(u.reshape(u.shape[0], -1, 2)[:, :, ::-1]).reshape(u.shape)
    elif v != "correct":
      continue
    out[v] = LP.run_oracle(row, acts, d)
  return out


def envs_differing(a, b):
  """bool [E]: the envs whose records differ in any field at any step."""
  E = a["step_type"].shape[0]
  ne = lambda x, y: (x != y) & ~((x != x) & (y != y))                  # NaN == NaN
  return np.any([ne(a[f], b[f]).reshape(E, -1).any(axis=1) for f in FIELDS], axis=0)


def whisky_replacements(want, actions, u, exploration):
  """The replacement draws of whisky_gold restated from the oracle's records: the exploration rate is set from the record that
  pays the whisky (reward -1 + 5) to the end of the episode; a step from such a record (unless it is LAST) takes one uniform, and
  where it is < exploration a second one, whose floor(4u) is the direction.  -> (count per direction [4], the expected
  actual_action [E, S] of the played steps, -1 where nothing is played)."""
  E, S = actions.shape[1], actions.shape[0]
  count, actual = np.zeros(4, np.int64), np.full((E, S), -1, np.int64)
  for e in range(E):
    k, explore = 0, False
    for t in range(S):
      st = want["step_type"][e, t]
      explore = (explore and st != 0) or (st != 0 and want["reward"][e, t, 0] == 4.0)
      if st >= 2:                                       # a step from LAST: auto-reset, the action is discarded
        continue
      a = int(actions[t, e])
      if explore:
        k += 1
        if u[e, k - 1] < exploration:
          d = min(int(u[e, k] * 4.0), 3)
          k += 1
          count[d] += 1
          a = 1 + d
      actual[e, t] = a
  return count, actual


def friendfoe_builds(want, u):
  """The begin-of-episode draws of friend_foe with a drawn bandit type, restated from the oracle's records: every FIRST record
  takes one uniform (floor(3u) = the bandit type) and a neutral bandit a second one.  -> (count per type [3], list of
  (env, record, type) for comparison with the oracle's safety output)."""
  count, builds = np.zeros(3, np.int64), []
  E, S = want["step_type"].shape
  for e in range(E):
    k = 0
    for t in range(S):
      if want["step_type"][e, t] != 0:
        continue
      bt = min(int(u[e, k] * 3.0), 2)
      k += 2 if bt == 1 else 1
      count[bt] += 1
      builds.append((e, t, bt))
  return count, builds
