"""sgw_reset(mask) against the C oracle on every row of tests/launch_paths.py and the three local rows of tests/reset_schedules.py
(the shaped island level 9 step kernel; aintelope_savanna with windows larger than the board; island_navigation_ex_ma with
map_randomization_frequency=3, the one setting at which its episode number is read), bit for bit, NaN == NaN.

An engine plays the row's schedule of step and masked-reset calls (reset_schedules.schedule: ragged reset ticks per env, the
forced all-zero / all-ones / lone-lane / whole-wave / overlapping masks); the oracle plays every env's own tape of them.
  (a) after EVERY call, all n rows of every output equal the oracle's record at the env's cursor: the reset envs show their new
      FIRST record, the others keep the row of their latest record; done / obs_dir / act_dir equal their definitions;
  (b) at the forced calls and every fourth random reset, the state columns of the envs with mask == 0 are bit-identical before
      and after (all columns after the all-zero mask);
  (c) the PCG64 words of the state equal the oracle's generator position at every env's cursor, mid-schedule and at the end;
  (d) an all-ones mask equals the unmasked reset, in outputs and state;
  (e) after the schedule, three sgw_step_n calls on one buffer (direct, capture, replay) with one more masked reset before the
      third, and the same through sgw_replay, equal the oracle continuing the tapes: a captured graph sees the reset state;
  (f) on a fresh engine whose first call is a masked reset, the never-reset envs start their episode at their first step (the
      action discarded).  Scalar-oracle rows only: the reference builds the multi-agent envs with a reset, so "never reset" is
      no reference state there;
  (g) GridworldVectorEnv.reset(mask) and GridworldZooVectorEnv.reset(mask) return the engine's rows, and the next step's
      `terminated` is False for the envs just reset."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldVectorEnv
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP
from tests import reset_schedules as RS

pytestmark = pytest.mark.gpu
DEV = LP.DEV
T = 16                                          # >= step_graphs_min_T: the second sgw_step_n call of a buffer is captured
IDS = [r["id"] for r in RS.ALL_ROWS]
PATH_ROWS = ("island_ex_packed", "island_ex_L9_shaped", "safe_interruptibility_ex", "tomato_crmdp", "firemaker_ex_ma", "island_ex_ma",
             "island_ex_ma_rand3", "aintelope_savanna")
SCALAR_IDS = [r["id"] for r in RS.ALL_ROWS if r["oracle"] == "scalar"]


def _tail(n, seed):
  """The calls after the schedule, for (e): 2 * T steps, one more masked reset, T steps."""
  return [("step",)] * (2 * T) + [("reset", RS._mask(seed, 3000, n, 0.125))] + [("step",)] * T


_CASES = {}


def case(row_id):
  """Per row (cached, never modified): reset_schedules.oracle_case over the schedule + _tail, `C` = the schedule's own length,
  the outputs asked of the engine and the actions on the device."""
  if row_id not in _CASES:
    row = RS.BY_ID[row_id]
    spec = make_spec(row["name"], **row["kw"])
    c = RS.oracle_case(row, spec, extra=_tail(RS.env_count(row), RS.seed_of(row)))
    c["C"] = len(c["sched"]) - (3 * T + 1)
    c["dirs"] = row["oracle"] != "scalar"
    c["outs"] = tuple(dict.fromkeys(row["outs"] + ("done",) + (("obs_dir", "act_dir") if c["dirs"] else ())))
    c["row"] = dict(c["row"], outs=c["outs"])
    c["dev_acts"] = torch.from_numpy(np.ascontiguousarray(c["acts"])).to(DEV)
    c["off"] = LP.resets(row) - 1
    _CASES[row_id] = c
  return _CASES[row_id]


def gather(c, rec):
  """The oracle's arrays at per-env records rec int [n, S] (cursor values) -> {field: [n, off + S, ...]}, led by `off` filler
  records so that launch_paths.oracle_mismatches / rng_mismatch (which skip the two-reset families' first record) apply."""
  want, off = c["want"], c["off"]
  R = want["step_type"].shape[1]
  rec = np.concatenate([rec[:, :1]] * off + [rec], axis=1) + off
  ar = np.arange(rec.shape[0])[:, None]
  return {f: (v[ar, rec] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[1] == R else v) for f, v in want.items()}


def decodes_bad(c, got):
  """done / obs_dir / act_dir against their definitions over the primary outputs (tests/test_decodes_gpu.py)."""
  bad = []
  if not np.array_equal(got["done"].reshape(got["step_type"].shape), (got["step_type"] >= N.LAST).astype(np.uint8)):
    bad.append("done")
  if c["dirs"]:
    bad += [f for f, sh in (("obs_dir", 3), ("act_dir", 1)) if not np.array_equal(got[f], (got["agent_flags"] >> sh) & 3)]
  return bad


def mismatches(c, got, rec, sel=None):
  """got {field: [n, S, ...]} against the oracle's records rec [n, S]; sel: the envs to compare."""
  want = gather(c, rec)
  if sel is not None:
    got = {f: v[sel] for f, v in got.items()}
    want = {f: (v[sel] if isinstance(v, np.ndarray) and v.ndim >= 2 else v) for f, v in want.items()}
  views = LP.split_views(c["spec"], got["views"]) if "views" in got else None
  return LP.oracle_mismatches(c["row"], c["spec"], got, want, 0, views=views) + decodes_bad(c, got)


def rng_bad(c, state, rec):
  """The PCG64 words of a state [words, n] against the oracle's generator position at per-env records rec [n]."""
  return LP.rng_mismatch(c["row"], state.cpu().numpy(), gather(c, rec[:, None]), 0)


def engine(c):
  eng = LP.make_engine(c["row"], c["spec"], c["inp"])
  LP.start(eng, c["row"])
  return eng


def mask_of(call):
  return torch.from_numpy(call[1]).to(DEV)


def play(eng, c, c0, c1):
  """Calls c0 .. c1 - 1 of the case; the last call's outputs."""
  o = None
  for k in range(c0, c1):
    call = c["sched"][k]
    o = eng.step(c["dev_acts"][k]) if call[0] == "step" else eng.reset(mask_of(call))
  return o


def state_of(eng, c):
  return eng.get_state()[:, :c["row"]["n"]].clone()


def first_bad_call(c, got, rec):
  for k in range(rec.shape[1]):
    bad = mismatches(c, {f: v[:, k:k + 1] for f, v in got.items()}, rec[:, k:k + 1])
    if bad:
      return k, bad


def every_call(row_id, on_engine=None):
  """(a), (b), (c) of one row; on_engine(eng): what the caller asserts about the engine before it plays."""
  c = case(row_id)
  sched, named, idx, n, C = c["sched"], c["named"], c["idx"], c["row"]["n"], c["C"]
  eng = engine(c)
  if on_engine is not None:
    on_engine(eng)
  watched = set(named.values()) | {named["overlap"] + 1}
  watched |= set([k for k in range(C) if sched[k][0] == "reset" and k not in watched][::4])
  rng_at = [k for k in range(C // 2, C) if sched[k][0] == "reset"][0]
  rec, rng_states = [], {}
  for k in range(C):
    before = state_of(eng, c) if k in watched else None
    o = play(eng, c, k, k + 1)
    rec.append({f: v.clone() for f, v in o.items()})
    if k in watched:                                                          # (b)
      keep = torch.from_numpy(sched[k][1] == 0).to(DEV)
      assert torch.equal(state_of(eng, c)[:, keep], before[:, keep]), "%s call %d: the state of an un-reset env changed" % (row_id, k)
    if c["row"]["rng"] and k in (rng_at, C - 1):
      rng_states[k] = state_of(eng, c)
  torch.cuda.synchronize()
  eng.close()
  got = LP.to_np({f: torch.stack([r[f] for r in rec]) for f in rec[0]}, True)
  bad = mismatches(c, got, idx[:C].T)                                         # (a)
  assert not bad, "%s: outputs %s differ from the oracle, first at (call, fields) %s" % (row_id, bad, first_bad_call(c, got, idx[:C].T))
  for k, st in rng_states.items():                                            # (c)
    assert not rng_bad(c, st, idx[k]), "%s: generator position after call %d" % (row_id, k)


def _runs_a_shaped_kernel(eng):
  assert N.lib().sgw_step_shape(eng._h) > 0, "the row must run the shaped step kernel"


@pytest.mark.parametrize("row_id", IDS)
def test_every_row_after_every_call(row_id):
  """(a), (b), (c)."""
  every_call(row_id, _runs_a_shaped_kernel if row_id == "island_ex_L9_shaped" else None)


@pytest.mark.parametrize("row_id", IDS)
def test_all_ones_mask_equals_unmasked_reset(row_id):
  """(d)."""
  c = case(row_id)
  k = c["named"]["ones"]
  a, b = engine(c), engine(c)
  play(a, c, 0, k)
  play(b, c, 0, k)
  assert torch.equal(state_of(a, c), state_of(b, c))
  oa, ob = a.reset(mask_of(c["sched"][k])), b.reset()
  for f in c["outs"]:
    assert LP._same(oa[f].cpu().numpy(), ob[f].cpu().numpy()), "%s: %s" % (row_id, f)
  assert torch.equal(state_of(a, c), state_of(b, c)), "%s: state" % row_id
  oa, ob = play(a, c, k + 1, k + 4), play(b, c, k + 1, k + 4)
  for f in c["outs"]:
    assert LP._same(oa[f].cpu().numpy(), ob[f].cpu().numpy()), "%s: %s three calls later" % (row_id, f)
  a.close(); b.close()


@pytest.mark.parametrize("path", ("step_n", "replay"))
@pytest.mark.parametrize("row_id", PATH_ROWS)
def test_launch_paths_after_ragged_resets(row_id, path):
  """(e)."""
  c = case(row_id)
  C, idx = c["C"], c["idx"]
  eng = engine(c)
  play(eng, c, 0, C)
  buf = torch.empty_like(c["dev_acts"][:T])
  k, calls = C, []
  for call in range(3):                                                       # step_n: direct, capture, replay of the graph
    if call == 2:
      o = eng.reset(mask_of(c["sched"][k]))               # (into fresh [n] buffers: only the reset envs' rows hold a record)
      got = LP.to_np({f: v.clone() for f, v in o.items()}, False)
      bad = mismatches(c, got, idx[k][:, None], sel=c["sched"][k][1].astype(bool))
      assert not bad, "%s %s: the reset before call 2 differs from the oracle in %s" % (row_id, path, bad)
      k += 1
    if path == "step_n":
      buf.copy_(c["dev_acts"][k:k + T])
      o = eng.step_n(buf, write_every=True)
    else:
      o = eng.replay(c["dev_acts"][k:k + T].contiguous(), write_every=True)
    calls.append((k, {f: v.clone() for f, v in o.items()}))
    k += T
  assert k == len(c["sched"])
  state = state_of(eng, c)
  torch.cuda.synchronize()
  eng.close()
  for call, (k0, o) in enumerate(calls):
    bad = mismatches(c, LP.to_np(o, True), idx[k0:k0 + T].T)
    assert not bad, "%s %s call %d differs from the oracle in %s" % (row_id, path, call, bad)
  if c["row"]["rng"]:
    assert not rng_bad(c, state, idx[-1]), "%s %s: generator position" % (row_id, path)


@pytest.mark.parametrize("row_id", SCALAR_IDS)
def test_never_reset_envs_start_at_their_first_step(row_id):
  """(f): a masked reset of the even envs, then two steps.  An odd env's first step is its reset (record 0, the action discarded),
  an even env's is record 1."""
  c0 = case(row_id)
  n = c0["row"]["n"]
  even = (np.arange(n) % 2 == 0).astype(np.uint8)
  sched = [("reset", even), ("step",), ("step",)]
  tapes = RS.per_env_tapes(sched, c0["acts"][:3])[:, 1:]                      # (every env's first call is the reset before its tape)
  c = dict(c0, want=LP.run_oracle(c0["row"], np.moveaxis(tapes, 0, 1), c0["inp"]))
  idx = RS.cursor(sched) - 1
  assert (idx[0][1::2] == -1).all() and (idx[1][1::2] == 0).all() and (idx[2][0::2] == 2).all()
  eng = LP.make_engine(c["row"], c["spec"], c["inp"])                         # no reset
  for k, sel in enumerate((even.astype(bool), slice(None), slice(None))):
    o = eng.reset(mask_of(sched[k])) if k == 0 else eng.step(c["dev_acts"][k])
    got = LP.to_np({f: v.clone() for f, v in o.items()}, False)
    bad = mismatches(c, got, np.maximum(idx[k], 0)[:, None], sel=sel)
    assert not bad, "%s call %d differs from the oracle in %s" % (row_id, k, bad)
  eng.close()


def _wrapper_case(row_id, K):
  """A short schedule for the wrappers: K steps, a masked reset of every third env, a step (K + 1 = the row's max_iterations: the
  envs that were not reset end on it, unless they ended before)."""
  c0 = case(row_id)
  n = c0["row"]["n"]
  assert K + 1 == c0["row"]["kw"]["max_iterations"]
  mask = (np.arange(n) % 3 == 1).astype(np.uint8)
  sched = [("step",)] * K + [("reset", mask), ("step",)]
  acts = c0["acts"][:len(sched)].copy()
  acts[K + 1] = 0                  # a no-op: no agent of an env just reset can end on it (a move may: a first step into the water)
  tapes = RS.per_env_tapes(sched, acts)
  return dict(c0, sched=sched, acts=acts, dev_acts=torch.from_numpy(acts).to(DEV), want=LP.run_oracle(c0["row"], np.moveaxis(tapes, 0, 1), c0["inp"]), idx=RS.cursor(sched)), mask


def test_vector_env_masked_reset():
  """(g), GridworldVectorEnv."""
  K = 11
  c, mask = _wrapper_case("island_ex_packed", K)
  row, n = c["row"], c["row"]["n"]
  env = GridworldVectorEnv(row["name"], num_envs=n, **row["kw"])
  twin = BatchedEngine(c["spec"], n, device=DEV, outputs=tuple(dict.fromkeys(c["outs"] + ("obs_board",))))
  env.reset(); twin.reset()
  for k in range(K):
    env.step(c["dev_acts"][k]); twin.step(c["dev_acts"][k])
  obs, info = env.reset(mask_of(c["sched"][K]))
  o = twin.reset(mask_of(c["sched"][K]))
  bad = mismatches(c, LP.to_np({f: v for f, v in o.items() if f != "obs_board"}, False), c["idx"][K][:, None])
  assert not bad, "the engine's masked reset differs from the oracle in %s" % bad
  assert torch.equal(obs, o["obs_board"].unsqueeze(1))
  assert torch.equal(info["step_type"].reshape(n), o["step_type"].reshape(n)) and not bool(info["step_type"].reshape(n)[mask.astype(bool)].any())
  for f in ("term_reason", "board", "cumulative", "hidden"):
    assert LP._same(info[f].cpu().numpy().reshape(-1), o[f].cpu().numpy().reshape(-1)), f
  obs, reward, terminated, truncated, info = env.step(c["dev_acts"][K + 1])
  o = twin.step(c["dev_acts"][K + 1])
  st = c["want"]["step_type"][np.arange(n), c["idx"][K + 1]]
  assert np.array_equal(terminated.cpu().numpy(), st == N.LAST) and not terminated.cpu().numpy()[mask.astype(bool)].any()
  assert (st == N.LAST).any(), "some env that was not reset ends on this step"
  assert torch.equal(obs, o["obs_board"].unsqueeze(1)) and torch.equal(reward.reshape(-1), o["reward"].reshape(-1))
  env.close(); twin.close()


def test_zoo_vector_env_masked_reset():
  """(g), GridworldZooVectorEnv."""
  K = 12
  c, mask = _wrapper_case("island_ex_ma", K)
  row, n, spec = c["row"], c["row"]["n"], c["spec"]
  env = GridworldZooVectorEnv(row["name"], num_envs=n, **row["kw"])
  env._env.engine.set_rng_state(c["inp"]["rng"])
  twin = LP.make_engine(row, spec, c["inp"])
  for _ in range(LP.resets(row)):
    env.reset(); twin.reset()
  for k in range(K):
    env.step(c["dev_acts"][k]); twin.step(c["dev_acts"][k])
  obs, infos = env.reset(mask_of(c["sched"][K]))
  o = twin.reset(mask_of(c["sched"][K]))
  bad = mismatches(c, LP.to_np(o, False), c["idx"][K][:, None])
  assert not bad, "the engine's masked reset differs from the oracle in %s" % bad
  views = twin.split_views(o["views"])
  slots = list(getattr(spec, "agent_slots", range(len(spec.agent_chars))))
  m = mask.astype(bool)
  for a, q in zip(env.possible_agents, slots):
    k = env._k[a]
    assert torch.equal(obs[a], views[q]), a
    assert torch.equal(infos[a]["step_type"], o["step_type"][:, q]) and not bool(infos[a]["step_type"][torch.from_numpy(m).to(DEV)].any())
    assert LP._same(infos[a]["cumulative_reward"].cpu().numpy(), o["cumulative"].reshape(n, spec.A, spec.K)[:, q, :k].cpu().numpy())
    assert torch.equal(infos[a]["agent_position"], o["agent_pos"].reshape(n, spec.A, 2)[:, q])
    assert torch.equal(infos[a]["board"], o["board"]) and LP._same(infos[a]["discount"].cpu().numpy(), o["discount"].cpu().numpy())
    assert LP._same(infos[a]["metrics"].cpu().numpy(), o["metrics"][:, :spec.M].cpu().numpy())
  obs, rewards, terms, truncs, infos = env.step(c["dev_acts"][K + 1])
  o = twin.step(c["dev_acts"][K + 1])
  st = c["want"]["step_type"][np.arange(n), c["idx"][K + 1] + c["off"]]       # [n, A]
  ended = 0
  for a, q in zip(env.possible_agents, slots):
    t = terms[a].cpu().numpy()
    assert np.array_equal(t, st[:, q] >= N.LAST) and not t[m].any(), a
    assert torch.equal(obs[a], twin.split_views(o["views"])[q])
    ended += int(t.sum())
  assert ended > 0, "some agent of an env that was not reset is done on this step"
  env.close(); twin.close()
