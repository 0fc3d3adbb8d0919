"""A deterministic schedule of step and masked-reset calls for the masked-reset GPU tests (engine == oracle after every call), and the per-stream reset rule of
the reset fixtures (tests/golden/resets_*.npz).

schedule(row, seed) -> list of calls, each ("step",) or ("reset", mask uint8 [n]), n = env_count(row).  About one random call
in four is a masked reset whose density is drawn per call from DENSITIES; forced calls (forced(row, seed): name -> call index)
are spliced in at fixed places:
  zero      an all-zero mask (nothing may change)              ones      an all-ones mask (== the unmasked reset)
  lone      exactly env n - 1 (a lone lane of the partial last wave)
  wave      exactly envs 64..127 (one whole wave on, its neighbours off; empty where the row has no such envs)
  overlap   two consecutive reset calls of density 1/2 (overlap + 1 is the second)
Rows whose episodes only end after 100 steps (LONG: no max_iterations to shorten them) start with 100 step calls, then reset
half of the envs on their LAST record ("at_last"), step, and reset half of them again ("after_auto").

Each env's stream is the subsequence of the calls that touch it (every step call, the reset calls whose mask holds it), so the
streams of one schedule have unequal lengths: per_env_tapes() writes them as the oracle's action tapes, cursor() gives the index
of every env's latest oracle record after every call.  coverage() counts, from the oracle's records alone, the explicit
resets by what the env's latest record was; tests/test_reset_schedules.py asserts MIN_COVER of each class for every row."""
import numpy as np

from ai_safety_gridworlds_amd import philox
from tests import launch_paths as LP

RESET = -128
N_MAX = 333                      # five full waves plus 13 lanes
RANDOM_CALLS = 88
DENSITIES = (1.0 / 64, 1.0 / 8, 1.0 / 2)
LONG = ("tomato_watering", "tomato_crmdp", "rocks_diamonds")
LONG_STEPS = 100
TAG_MASK, TAG_KIND = 0x5EED, 0x5EEE
MIN_COVER, MIN_PARTIAL = 8, 3
FORCED_AT = dict(zero=9, ones=22, lone=37, wave=50, overlap=66)      # positions among the random calls

# rows of the masked-reset tests only (launch_paths.ROWS keeps one row per env name): the step kernel with the island level 9 output geometry
# compiled in, aintelope_savanna with agent windows larger than the board (the chunked masked window path), and
# island_navigation_ex_ma with map_randomization_frequency=3, where an explicit reset's bump of the episode number decides whether
# the map is drawn again (at frequency 2, the launch_paths row, the number is never read)
LOCAL_ROWS = [
    LP._row("island_ex_L9_shaped", "island_navigation_ex", dict(level=9, max_iterations=15), 333, None),
    LP._row("aintelope_savanna_r10", "aintelope_savanna",
            dict(LP.BY_ID["aintelope_savanna"]["kw"], observation_radius=[10, 10, 10, 10]), 333, None, oracle="sav", outs=LP.SAV,
            rng=True),
    LP._row("island_ex_ma_rand3", "island_navigation_ex_ma", dict(LP.BY_ID["island_ex_ma"]["kw"], map_randomization_frequency=3), 333, None,
            oracle="ima", outs=LP.WIN, rng=True),
]
ALL_ROWS = LP.ROWS + LOCAL_ROWS
BY_ID = {r["id"]: r for r in ALL_ROWS}


def env_count(row):
  return min(row["n"], N_MAX)


def _mask(seed, c, n, density):
  x0 = philox.philox4x32_10(np.uint64(c), TAG_MASK, 0, 0, seed, np.arange(n, dtype=np.uint64))[0]
  return (x0.astype(np.float64) < density * 2.0 ** 32).astype(np.uint8)


def _build(row, seed):
  n = env_count(row)
  kinds = philox.philox4x32_10(np.arange(RANDOM_CALLS, dtype=np.uint64), TAG_KIND, 0, 0, seed, 0)
  calls, named = [], {}
  if row["name"] in LONG:
    calls += [("step",)] * LONG_STEPS
    named["at_last"] = len(calls); calls.append(("reset", _mask(seed, 1000, n, 0.5)))
    calls.append(("step",))
    named["after_auto"] = len(calls); calls.append(("reset", _mask(seed, 1001, n, 0.5)))
  ids = np.arange(n)
  for c in range(RANDOM_CALLS):
    for name, at in FORCED_AT.items():
      if at != c:
        continue
      named[name] = len(calls)
      if name == "zero":
        calls.append(("reset", np.zeros(n, np.uint8)))
      elif name == "ones":
        calls.append(("reset", np.ones(n, np.uint8)))
      elif name == "lone":
        calls.append(("reset", (ids == n - 1).astype(np.uint8)))
      elif name == "wave":
        calls.append(("reset", ((ids >= 64) & (ids < 128)).astype(np.uint8)))
      else:
        calls += [("reset", _mask(seed, 2000, n, 0.5)), ("reset", _mask(seed, 2001, n, 0.5))]
    if int(kinds[0][c]) % 4 == 0:
      calls.append(("reset", _mask(seed, c, n, DENSITIES[int(kinds[1][c]) % 3])))
    else:
      calls.append(("step",))
  return calls, named


def schedule(row, seed):
  return _build(row, seed)[0]


def forced(row, seed):
  return _build(row, seed)[1]


def touched(sched):
  """bool [C, n]: the calls that touch each env."""
  n = _n(sched)
  return np.stack([np.ones(n, bool) if c[0] == "step" else c[1].astype(bool) for c in sched])


def _n(sched):
  return next(len(c[1]) for c in sched if c[0] == "reset")


def cursor(sched):
  """int64 [C, n]: after call c, the index of env e's latest record (record 0 = the reset before the schedule)."""
  return np.cumsum(touched(sched), axis=0)


def per_env_tapes(sched, actions):
  """actions int8 [C, n(, A)] (the action of every call; ignored at reset calls) -> the oracle's tapes int8 [n, L(, A)]: RESET
  where the env was masked, the calls that skipped the env compacted away, the tail padded with steps of action 0."""
  actions = np.asarray(actions, dtype=np.int8)
  tch = touched(sched)
  C, n = tch.shape
  is_reset = np.array([c[0] == "reset" for c in sched])
  L = int(tch.sum(axis=0).max())
  tapes = np.zeros((n, L) + actions.shape[2:], np.int8)
  for e in range(n):
    cs = np.nonzero(tch[:, e])[0]
    t = actions[cs, e].copy()
    t[is_reset[cs]] = RESET
    tapes[e, :len(cs)] = t
  return tapes


def step_types(row, want):
  """The oracle's step_type as [E, S, A], S counted from the reset before the schedule."""
  st = want["step_type"]
  if row["oracle"] in ("ima", "sav"):
    st = st[:, 1:]                                      # (its record starts with two resets)
  return st.reshape(st.shape[0], st.shape[1], -1)


def coverage(row, sched, tapes, want):
  """Explicit resets by the class of the env's latest record, from the oracle's records alone: first (a reset's record), mid
  (every agent MID), last (every agent LAST or DEAD), auto (the FIRST record an auto-reset step produced), partial (an agent
  LAST or DEAD next to one that is not)."""
  st = step_types(row, want)
  slot0 = tapes.reshape(tapes.shape[0], tapes.shape[1], -1)[:, :, 0]
  idx = cursor(sched)
  n = idx.shape[1]
  count = dict(first=0, mid=0, last=0, auto=0, partial=0)
  for c, call in enumerate(sched):
    if call[0] != "reset":
      continue
    prev = idx[c - 1] if c else np.zeros(n, np.int64)
    for e in np.nonzero(call[1])[0]:
      r = int(prev[e])
      s = st[e, r]
      done = s >= 2
      if (s == 0).all():
        by_reset = r == 0 or slot0[e, r - 1] == RESET
        count["first" if by_reset else "auto"] += 1
      elif done.all():
        count["last"] += 1
      elif done.any():
        count["partial"] += 1
      elif (s == 1).all():
        count["mid"] += 1
  return count


class TapeResets(object):
  """Where stream e of a reset fixture calls the reference's reset() (tests/golden/make_fixtures*.py), decided from what the
  stream has shown so far, so that the ticks differ per stream: in place of the auto-reset after every third finished episode,
  on the tick after the auto-reset of another third; on the odd streams also twice in a row early in the stream and once
  more later (mid-episode); on streams 2 and 3 of every four at every second tick on which one agent is done and another is not.
  The committed tests/golden/resets_*.npz were recorded under this rule: regenerate them (every make_fixtures*.py) when it changes."""

  def __init__(self, e):
    self.e, self.lasts, self.partials = e, 0, 0
    self.t_mid = 4 + e % 5
    self.t_late = self.t_mid + 17 + 3 * (e % 4)

  def want(self, t, done, after_auto, partial=False):
    if done:
      self.lasts += 1
      return (self.lasts + self.e) % 3 == 0
    if after_auto and (self.lasts + self.e) % 3 == 1:
      return True
    if partial and self.e % 4 >= 2:
      self.partials += 1
      return self.partials % 2 == 0
    return self.e % 2 == 1 and t in (self.t_mid, self.t_mid + 1, self.t_late)


def tape_classes(step_type, slot0):
  """What a recorded tape holds, per stream: the four kinds of explicit reset the fixtures must contain.  step_type [S(, A)]
  and slot0 [S - 1] (the stream's actions, agent 0's slot) aligned so that slot0[t] produced record t + 1."""
  st = step_type.reshape(step_type.shape[0], -1)
  got = set()
  for t in np.nonzero(slot0 == RESET)[0]:
    s = st[t]
    if t > 0 and slot0[t - 1] == RESET:
      got.add("after_reset")
    elif (s >= 2).all():
      got.add("after_last")
    elif (s == 0).all() and t > 0:
      got.add("after_auto")
    elif (s == 1).all():
      got.add("mid")
  return got


DEFAULT_SEED = 0x2E5E7
# row id -> schedule seed, where DEFAULT_SEED misses a class of coverage() (found by running the oracle on the host)
SEEDS = {"island_ex_plain": DEFAULT_SEED + 1, "safe_interruptibility_ex": DEFAULT_SEED + 4, "side_effects_sokoban": DEFAULT_SEED + 1,
         "conveyor_belt_ex": DEFAULT_SEED + 5}


def seed_of(row):
  return SEEDS.get(row["id"], DEFAULT_SEED)


def host_actions(spec, n, C, seed):
  """int8 [C, n(, A)]: the action of every call of a schedule (the package's synthetic Philox stream, per agent)."""
  per = [philox.actions(seed, np.arange(n), np.arange(C), spec.action_lo, spec.n_actions, agent=a).astype(np.int8)
         for a in range(spec.A)]
  return per[0] if spec.A == 1 else np.stack(per, axis=-1)


def oracle_case(row, spec, extra=()):
  """The row cut to env_count(row) envs, its schedule (+ `extra` calls appended), the actions of every call, the inputs, the
  per-env tapes, the oracle's records of them and the cursor."""
  row = dict(row, n=env_count(row))
  seed = seed_of(row)
  sched = schedule(row, seed) + list(extra)
  acts = host_actions(spec, row["n"], len(sched), seed)
  inp = LP.inputs(row, spec, seed & 0xFF)
  tapes = per_env_tapes(sched, acts)
  want = LP.run_oracle(row, np.moveaxis(tapes, 0, 1), inp)
  return dict(row=row, spec=spec, sched=sched, named=forced(row, seed), acts=acts, inp=inp, tapes=tapes, want=want, idx=cursor(sched))
