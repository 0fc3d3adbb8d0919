"""Caller actions outside a family's own sampling range -- QUIT (9), NOOP (0) where the range starts at 1, the turn actions
5..8 -- on every launch path that takes caller actions (tests/test_action_domain_gpu.py).  The C ABI takes a raw int8 per env
and validates nothing, and neither does the reference's step(), so all of these reach play() of every single-agent family.

Rows: the scalar rows of tests/launch_paths.py at ragged sizes, cycled over the rows: a lone env, one short of a wave, one
over, three waves and one env.  Tape: the row's own Philox stream (sgw_fill_actions) with the `_quitlate` rule of
tests/golden/make_fixtures.py laid over it.  tests/test_action_domain_fixtures.py checks on the CPU, with the oracle, that
every row's tape ends at least one episode with QUIT inside the row's calls."""
import copy

import numpy as np

from ai_safety_gridworlds_amd import philox
from tests import launch_paths as LP

T, CALLS, SEED = 16, 3, 0x1A7C          # as tests/test_launch_paths_gpu.py: the second call of a buffer is captured
SIZES = (65, 193, 1, 63)                # cycled over the rows; this order gives the three FOLLOW rows more than a lone env
QUIT = 3                                # term_reason of Actions.QUIT
QUIT_ACTION = 9
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


def overlay(base, env_ids, step0=0, agent=0, seed=None, turns=True):
  """base int8 [S, E]: the `_quitlate` rule -- 9 with probability 1/24, one of {0, 5, 6, 7, 8} with probability 1/24.  agent:
  every agent of a multi-agent tape has its own gate stream.  turns=False: the "odd" value is 0 (configurations in which the
  reference does not survive 5..8)."""
  seed = SEED if seed is None else seed
  steps = step0 + np.arange(base.shape[0])
  gate = philox.actions(seed ^ 0x9, env_ids, steps, 0, 24, agent=agent)
  odd = np.array([0, 5, 6, 7, 8])[philox.actions(seed ^ 0x58, env_ids, steps, 0, 5, agent=agent)] if turns else 0
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


# ---- multi-agent tapes: the fixtures of tests/golden/make_fixtures_{ma,ima,sav}.py ----


def legal_quit_round(np_random, row, sub):
  """row: the int8 actions of one round (edited in place), sub: who would be submitted.  A round with a submitted 9 stays whole
  when the order the reference is going to draw plays the first quitter last; otherwise everybody but the first quitter (in
  agent order) is withdrawn (-1): a lone submitter, no shuffle, no draw.  Returns the new `sub`."""
  who = [i for i in range(len(sub)) if sub[i]]
  quitters = [i for i in who if row[i] == QUIT_ACTION]
  if not quitters or len(who) == 1:
    return sub
  items = [(i, int(row[i])) for i in who]                     # what EnvironmentMa.step shuffles: one item per submitted agent
  copy.deepcopy(np_random).shuffle(items)
  order = [i for i, _ in items]
  if order[-1] in quitters and not any(i in quitters for i in order[:-1]):
    return sub
  for i in range(len(sub)):
    if i != quitters[0]:
      row[i] = -1
  return [i == quitters[0] for i in range(len(sub))]


def quit_fixture_counts(name, rec, slots, resets=2):
  """The conditions of a multi-agent `_quit` / `_quitlate` fixture, from its arrays alone (the generator asserts them when it
  records, tests/test_action_domain_fixtures.py on the committed file).  slots: the agent columns that are present; resets: the
  record's slots before the first tick's (two resets for island_navigation_ex_ma / aintelope_savanna, one for firemaker).
  Returns them as counts for the meta."""
  acts, sub, st, tr = rec["actions"][:, :, slots], rec["submitted"][:, :, slots], rec["step_type"][:, :, slots], rec["term_reason"][:, :, slots]
  before, after = st[:, resets - 1:-1], st[:, resets:]        # tick t plays on slot t + resets - 1 and is recorded in the next
  live = ~((before >= 2).all(axis=2))                         # (an all-done round auto-resets and discards its actions)
  played = sub & (acts == QUIT_ACTION) & live[..., None]      # [E, T, A]
  assert (after[played.any(axis=2)] >= 2).all(), "%s: a played 9 that did not end the episode for every agent" % name
  # (a drape that runs on the QUIT frame may terminate an agent again and rewrite its reason: count the quitters that keep QUIT)
  per_agent = (played & (tr[:, resets:] == QUIT)).sum(axis=(0, 1))
  assert (per_agent >= 1).all(), "%s: QUIT-ended episodes per quitter %s" % (name, per_agent)
  n_sub = sub.sum(axis=2)
  whole, solo = int((played.any(axis=2) & (n_sub > 1)).sum()), int((played.any(axis=2) & (n_sub == 1)).sum())
  assert (whole >= 1 or len(slots) == 1) and solo >= 1, "%s: %d whole and %d solo QUIT rounds" % (name, whole, solo)
  first = np.where(played.any(axis=2).any(axis=1), played.any(axis=2).argmax(axis=1), acts.shape[1])
  tail = int(acts.shape[1] - 1 - first.min())
  assert tail >= 20, "%s: %d ticks after the first QUIT" % (name, tail)
  done = before >= 2
  others_done = int((played & ((done.sum(axis=2, keepdims=True) - done) > 0)).sum())      # a QUIT next to an agent that is LAST / DEAD
  fires = (rec["board"] == ord("F")).sum(axis=(2, 3))         # firemaker: QUIT frames on which the fire spread (other boards have no fire: 0)
  spread = int((played.any(axis=2) & (fires[:, resets:] > fires[:, resets - 1:-1])).sum())
  return dict(quit_per_agent=per_agent.astype(np.int32), quit_whole=whole, quit_solo=solo, quit_tail=tail, quit_others_done=others_done,
              quit_fire_spread=spread)


# ---- multi-agent launch-path rows (tests/test_action_domain_gpu.py) ----
# The "ma" / "ima" / "sav" rows of tests/launch_paths.py, continuing the size cycle, and one turn-mode row of the two-agent
# island: action / observation direction mode 2 / 2 is a pair in which the reference plays 5..8, so the turning
# actions are live next to 9.  The tape is the row's sgw_fill_actions stream with the overlay laid over every agent's column
# from that agent's own gate stream.  It is NOT edited for the round order: it holds rounds in which a play follows a QUIT, which
# the reference does not define and the engine drops -- pinned here, kernel against oracle, and nowhere else.
MA_TURN_ROW = dict(LP.BY_ID["island_ex_ma"], id="island_ex_ma_turn",
                   kw=dict(level=9, action_direction_mode=2, observation_direction_mode=2, max_iterations=13))
MA_MORE_CALLS = {}
MA_ROWS = [dict(r, n=SIZES[i % len(SIZES)], calls=MA_MORE_CALLS.get(r["id"], CALLS))
           for i, r in enumerate([r for r in LP.ROWS if r["oracle"] in ("ma", "ima", "sav")] + [MA_TURN_ROW])]
MA_BY_ID = {r["id"]: r for r in MA_ROWS}


def ma_steps_of(row):
  return row["calls"] * T


def ma_inputs(row, spec):
  return LP.inputs(row, spec, 100 + MA_ROWS.index(row))


def turns_survive(spec):
  """The reference plays 5..8 in this configuration (tests/golden/probe_turn_pairs.py; the table is in DESIGN.md)."""
  am, om = spec.config.get("action_direction_mode", 0), spec.config.get("observation_direction_mode", 0)
  return (am, om) in ((0, 0), (2, 0), (2, 2))


def ma_overlay(base, spec, env_ids, step0=0):
  """base int8 [S, E, A] -> the overlay on every agent's column."""
  return np.stack([overlay(base[..., a], env_ids, step0, agent=a, turns=turns_survive(spec)) for a in range(base.shape[2])], axis=-1)


def ma_host_tape(row, spec, steps=None):
  """int8 [steps, n, A]: sgw_fill_actions restated on the host (one Philox stream per agent), with the overlay."""
  ids, steps = np.arange(row["n"]), np.arange(ma_steps_of(row) if steps is None else steps)
  base = np.stack([philox.actions(SEED, ids, steps, spec.action_lo, spec.n_actions, agent=a) for a in range(spec.A)], axis=-1)
  return ma_overlay(base, spec, ids)


def ma_slots(row, spec):
  """The agent columns that are present (firemaker keeps the '1', '2', 'S' layout)."""
  return list(spec.agent_slots) if row["oracle"] == "ma" else list(range(spec.A))


def ma_quit_rounds(row, spec, tape, want, steps):
  """From the tape and the oracle's arrays alone: per round of steps 1..steps, whether a 9 was played, by whom, and whether a
  play was dropped behind it.  The order the oracle drew is not recorded, so a quitter is told from the rounds in which exactly
  one live submitted agent holds a 9; a drop is certain where two or more live agents submitted and the round ended with QUIT
  after fewer frames than submitters.  Returns dict(per_agent [A'], dropped, whole)."""
  off = LP.resets(row) - 1
  slots = ma_slots(row, spec)
  st, fr, tr = want["step_type"][:, off:off + steps + 1], want["frame"][:, off:off + steps + 1], want["term_reason"][:, off:off + steps + 1]
  acts = np.moveaxis(tape[:steps], 0, 1)[:, :, slots]                     # [E, steps, A']
  before, after = st[:, :-1][:, :, slots], st[:, 1:][:, :, slots]
  live = ~(before >= 2).all(axis=2)
  sub = (acts >= 0) & (before < 2) & live[..., None]                        # submitted = alive and action >= 0
  ended = live & (after >= 2).all(axis=2) & (tr[:, 1:][:, :, slots] == QUIT).any(axis=2)
  plays = fr[:, 1:] - fr[:, :-1]                                            # frames the round played
  nine = sub & (acts == QUIT_ACTION)
  lone = ended & (nine.sum(axis=2) == 1)
  per_agent = (nine & lone[..., None]).sum(axis=(0, 1))
  n_sub = sub.sum(axis=2)
  dropped = int((ended & (n_sub > 1) & (plays < n_sub)).sum())
  whole = int((ended & (n_sub > 1) & (plays == n_sub)).sum())
  return dict(per_agent=per_agent, dropped=dropped, whole=whole, ended=int(ended.sum()))
