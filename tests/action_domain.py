"""Caller actions outside a family's own sampling range -- QUIT (9), NOOP (0) where the range starts at 1, the turn actions
5..8 -- on every launch path that takes caller actions (tests/test_action_domain_gpu.py).  The C ABI takes a raw int8 per env
and validates nothing, and neither does the reference's step(), so all of these reach play() of every single-agent family.

Rows: the scalar rows of tests/launch_paths.py at ragged sizes, cycled over the rows: a lone env, one short of a wave, one
over, three waves and one env.  Tape: the row's own Philox stream (sgw_fill_actions) with the `_quitlate` rule of
tests/golden/make_fixtures.py laid over it.  tests/test_action_domain_fixtures.py checks on the CPU, with the oracle, that
every row's tape ends at least one episode with QUIT inside the row's calls."""
import numpy as np

from ai_safety_gridworlds_amd import philox
from tests import launch_paths as LP

T, CALLS, SEED = 16, 3, 0x1A7C          # as tests/test_launch_paths_gpu.py: the second call of a buffer is captured
SIZES = (65, 193, 1, 63)                # cycled over the rows; this order gives the three FOLLOW rows more than a lone env
QUIT = 3                                # term_reason of Actions.QUIT
# the three rows of launch_paths.py that take no max_iterations keep their seven calls: the later calls run long episodes that a
# QUIT cuts short; every row's tape, the lone-env ones included, ends an episode with QUIT inside its first three calls
MORE_CALLS = {"tomato_watering": 7, "tomato_crmdp": 7, "rocks_diamonds": 7}

ROWS = [dict(r, n=SIZES[i % len(SIZES)], calls=MORE_CALLS.get(r["id"], CALLS))
        for i, r in enumerate(r for r in LP.ROWS if r["oracle"] == "scalar")]
BY_ID = {r["id"]: r for r in ROWS}
GROUPS = LP.GROUPS
FOLLOW = ("island_ex_packed", "tomato_watering", "safe_interruptibility")      # what follows a QUIT: returns, episode log, draws


def steps_of(row):
  return max(row["calls"], CALLS) * T


def inputs(row, spec):
  return LP.inputs(row, spec, ROWS.index(row))


def overlay(base, env_ids, step0=0):
  """base int8 [S, E]: the `_quitlate` rule -- 9 with probability 1/24, one of {0, 5, 6, 7, 8} with probability 1/24."""
  steps = step0 + np.arange(base.shape[0])
  gate = philox.actions(SEED ^ 0x9, env_ids, steps, 0, 24)
  odd = np.array([0, 5, 6, 7, 8])[philox.actions(SEED ^ 0x58, env_ids, steps, 0, 5)]
  return np.where(gate == 0, 9, np.where(gate == 1, odd, base)).astype(np.int8)


def host_tape(row, spec):
  """The row's tape restated on the host (sgw_fill_actions == philox.actions): int8 [steps_of(row), n]."""
  ids = np.arange(row["n"])
  base = philox.actions(SEED, ids, np.arange(steps_of(row)), spec.action_lo, spec.n_actions)
  return overlay(base, ids)


def quit_lasts(want, steps):
  """LAST steps with term_reason QUIT among steps 1..steps of the oracle's arrays [E, S, ...]."""
  return int(((want["step_type"][:, 1:steps + 1] == 2) & (want["term_reason"][:, 1:steps + 1] == QUIT)).sum())


def oracle_draws(row, tape, inp, steps):
  """tomato_*: numbers each env has taken from its external stream after `steps` steps, from the oracle stepped one env at a
  time.  int64 [E]."""
  from oracle import oracle as O
  cfg = O.make_config(row["name"], **row["kw"])
  out = np.zeros(row["n"], np.int64)
  for e in range(row["n"]):
    env = O.Env(cfg)
    env.set_random_stream(inp["rand_oracle"][e])
    env.reset()
    for t in range(steps):
      env.step(int(tape[t, e]))
    out[e] = env.random_draws()
  return out
