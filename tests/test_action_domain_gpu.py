"""QUIT (9) and action values outside a family's own range on every launch path that takes caller actions, against the C oracle
byte for byte (which tests/test_oracle_golden.py pins to the reference on the `_quit` / `_quitlate` fixtures): the rows and
tapes of tests/action_domain.py through sgw_step, sgw_step_n over one buffer refilled in place (direct, captured, replayed),
sgw_replay (state in registers: the auto-reset after a QUIT happens inside the launch) and every group through
sgw_group_step_n.  Then what follows a QUIT: the finished-episode returns, the episode log, and tomato_watering's position in its
external random stream.  The comparison helpers are those of tests/test_launch_paths_gpu.py."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd.engine import EngineGroup, EpisodeLog
from ai_safety_gridworlds_amd.specs import make_spec
from tests import action_domain as AD
from tests import launch_paths as LP
from tests.launch_paths import DEV, make_engine, start, to_np
from tests.test_launch_paths_gpu import check, check_returns

pytestmark = pytest.mark.gpu
T, CALLS = AD.T, AD.CALLS

_CASES = {}


def case(row_id):
  """Per row (cached): spec, inputs, the tape on the device (the row's sgw_fill_actions stream copied back, the overlay applied
  on the host, uploaded again), the oracle's arrays, and an engine stepped one sgw_step at a time -- compared with the oracle at
  every step -- with its state after every multiple of T steps."""
  if row_id in _CASES:
    return _CASES[row_id]
  row = AD.BY_ID[row_id]
  spec = make_spec(row["name"], **row["kw"])
  inp = AD.inputs(row, spec)
  ref = make_engine(row, spec, inp)
  S = AD.steps_of(row)
  tape = AD.overlay(ref.fill_actions(S, AD.SEED).cpu().numpy(), np.arange(row["n"]))
  assert np.array_equal(tape, AD.host_tape(row, spec)), "the tape the CPU tier checked with the oracle"
  acts = torch.from_numpy(tape).to(DEV)
  rec = {k: [v.clone()] for k, v in start(ref, row).items()}
  states = {}
  for t in range(S):
    for k, v in ref.step(acts[t]).items():
      rec[k].append(v.clone())
    if (t + 1) % T == 0:
      states[t + 1] = ref.get_state()[:, :row["n"]].clone()
  torch.cuda.synchronize()
  got = to_np({k: torch.stack(v) for k, v in rec.items()}, True)
  want = LP.run_oracle(row, tape, inp)
  c = dict(row=row, spec=spec, inp=inp, acts=acts, tape=tape, want=want, ref=got, states=states)
  check(c, {k: v[:, 1:] for k, v in got.items()}, 1, "sgw_step")
  assert AD.quit_lasts(want, row["calls"] * T) >= 1 and AD.quit_lasts(want, CALLS * T) >= 1, "%s: no episode ends with QUIT" % row_id
  st, cum = want["step_type"][..., None], want["cumulative"]
  c["returns"] = {s: LP.finished_returns(st[:, :s + 1], cum[:, :s + 1]) for s in {row["calls"] * T, CALLS * T}}
  ref.close()
  _CASES[row_id] = c
  return c


@pytest.mark.parametrize("path", ("step_n", "replay"))
@pytest.mark.parametrize("row_id", [r["id"] for r in AD.ROWS])
def test_launch_path_with_quit_matches_oracle(row_id, path):
  c = case(row_id)
  row, spec, acts = c["row"], c["spec"], c["acts"]
  eng = make_engine(row, spec, c["inp"])
  start(eng, row)
  buf = torch.empty_like(acts[:T])
  calls, n_calls = [], row["calls"]
  for k in range(n_calls):
    if path == "step_n":                          # call 0: direct launches, call 1: capture + replay, later calls: replay
      buf.copy_(acts[k * T:(k + 1) * T])
      o = eng.step_n(buf, write_every=True, accumulate=True)
    else:
      o = eng.replay(acts[k * T:(k + 1) * T], write_every=True, accumulate=True)
    calls.append({f: v.clone() for f, v in o.items()})
  ret = eng.read_returns()
  state = eng.get_state()[:, :row["n"]]
  torch.cuda.synchronize()
  for k, o in enumerate(calls):
    check(c, to_np(o, True), 1 + k * T, "%s call %d" % (path, k))
  assert torch.equal(state, c["states"][n_calls * T]), "%s %s: final state differs from the sgw_step engine" % (row_id, path)
  check_returns(c, ret, n_calls * T, path)
  eng.close()


@pytest.mark.parametrize("gid,members", AD.GROUPS, ids=[g for g, _ in AD.GROUPS])
def test_group_step_n_with_quit_matches_oracle(gid, members):
  cs = [case(m) for m in members]
  engines = [make_engine(c["row"], c["spec"], c["inp"]) for c in cs]
  for c, e in zip(cs, engines):
    start(e, c["row"])
  grp = EngineGroup(engines)
  bufs = [torch.empty_like(c["acts"][:T]) for c in cs]
  torch.cuda.synchronize()
  for k in range(CALLS):                           # direct, capture, replay; the actions refilled in place
    for b, c in zip(bufs, cs):
      b.copy_(c["acts"][k * T:(k + 1) * T])
    outs = grp.step_n(bufs, write_every=True, accumulate=True)
    torch.cuda.synchronize()
    for c, o in zip(cs, outs):
      check(c, to_np(o, True), 1 + k * T, "%s group step_n call %d" % (gid, k))
  for c, e in zip(cs, engines):
    check_returns(c, e.read_returns(), CALLS * T, "%s group step_n" % gid)
    assert torch.equal(e.get_state()[:, :c["row"]["n"]], c["states"][CALLS * T]), "%s %s: state" % (gid, c["row"]["id"])
  grp.close()
  for e in engines:
    e.close()


@pytest.mark.parametrize("row_id", AD.FOLLOW)
def test_what_follows_a_quit(row_id):
  """After the row's calls of sgw_step_n: read_returns() is the oracle's finished episodes; the episode log, appended to after
  every call from that call's rollout buffer, holds one record per LAST row of the oracle in (t, n) order with QUIT exactly where
  the oracle has it; tomato_watering's draw counter (state word 1, high half) is the oracle's count of numbers drawn."""
  c = case(row_id)
  row, spec, acts, want = c["row"], c["spec"], c["acts"], c["want"]
  n, n_calls = row["n"], row["calls"]
  S = n_calls * T
  eng = make_engine(row, spec, c["inp"])
  start(eng, row)
  log = EpisodeLog(eng, S * n)
  buf = torch.empty_like(acts[:T])
  for k in range(n_calls):
    buf.copy_(acts[k * T:(k + 1) * T])
    eng.step_n(buf, write_every=True, accumulate=True)
    eng.log_episodes(log, step_base=k * T)
  ret = eng.read_returns()
  state = eng.get_state()[:, :n].cpu().numpy()
  count = log.count()
  rec = {k: v.cpu().numpy() for k, v in log.records().items()}
  eng.close()
  check_returns(c, ret, S, "what follows a QUIT")
  last = (want["step_type"][:, 1:S + 1] == 2).T                      # [t, n]
  ts, ns = np.nonzero(last)                                          # row-major: (t, n) order
  assert count == len(ts) == c["returns"][S][-1] and count <= S * n
  assert np.array_equal(rec["env"], ns) and np.array_equal(rec["step"], ts)
  assert np.array_equal(rec["term_reason"].astype(np.int64), want["term_reason"][ns, ts + 1].astype(np.int64))
  assert (rec["term_reason"] == AD.QUIT).sum() == AD.quit_lasts(want, S) >= 1
  assert np.array_equal(rec["length"], want["frame"][ns, ts + 1])
  assert rec["ret"].tobytes() == np.ascontiguousarray(want["cumulative"][ns, ts + 1]).tobytes()
  assert rec["hidden"].tobytes() == np.ascontiguousarray(want["hidden"][ns, ts + 1]).tobytes()
  if row_id == "tomato_watering":
    draws = (state[1].view(np.uint64) >> np.uint64(32)).astype(np.int64)
    assert np.array_equal(draws, AD.oracle_draws(row, c["tape"], c["inp"], S))


# ---- the multi-agent families: firemaker_ex_ma, island_navigation_ex_ma (and its turn-mode row), aintelope_savanna ----
# Their tapes (tests/action_domain.py MA_ROWS) are not edited for the round order: they hold rounds in which a play follows a QUIT,
# which the reference's engine raises for and this engine drops; tests/test_action_domain_fixtures.py shows with the
# oracle alone that every row's tape has such rounds, whole QUIT rounds and every agent as the quitter inside its calls.
# sgw_rollout draws its actions in the kernel from the family's own range, so no 9 can reach it: every path ends with one rollout
# call that carries on from the state the tape left -- episodes cut short by QUIT, the generator where the dropped plays left it.

_MA_CASES = {}


def ma_case(row_id):
  """As case(): the tape is the overlay over every agent's column of the row's sgw_fill_actions stream for the row's calls, then T
  steps of the plain stream (what the closing rollout call draws); the sgw_step engine is compared with the oracle at every step,
  in-launch windows included, and its PCG64 words with the oracle's after every call."""
  if row_id in _MA_CASES:
    return _MA_CASES[row_id]
  row = AD.MA_BY_ID[row_id]
  spec = make_spec(row["name"], **row["kw"])
  inp = AD.ma_inputs(row, spec)
  ref = make_engine(row, spec, inp)
  S0 = AD.ma_steps_of(row)
  S = S0 + T
  base = ref.fill_actions(S, AD.SEED).cpu().numpy()
  tape = np.concatenate([AD.ma_overlay(base[:S0], spec, np.arange(row["n"])), base[S0:]])
  assert np.array_equal(tape[:S0], AD.ma_host_tape(row, spec)), "the tape the CPU tier checked with the oracle"
  acts = torch.from_numpy(tape).to(DEV)
  rec = {k: [v.clone()] for k, v in start(ref, row).items()}
  states = {}
  for t in range(S):
    for k, v in ref.step(acts[t]).items():
      rec[k].append(v.clone())
    if (t + 1) % T == 0:
      states[t + 1] = ref.get_state()[:, :row["n"]].clone()
  torch.cuda.synchronize()
  got = to_np({k: torch.stack(v) for k, v in rec.items()}, True)
  want = LP.run_oracle(row, tape, inp)
  c = dict(row=row, spec=spec, inp=inp, acts=acts, tape=tape, want=want, ref=got, states=states)
  check(c, {k: v[:, 1:] for k, v in got.items()}, 1, "sgw_step")
  for s, st in states.items():       # the shuffle of a round draws before any play: dropped plays leave the stream where the oracle's is
    assert not LP.rng_mismatch(row, st.cpu().numpy(), want, s), "%s sgw_step: generator position after %d steps" % (row_id, s)
  q = AD.ma_quit_rounds(row, spec, tape, want, S0)
  assert (q["per_agent"] >= 1).all() and q["dropped"] >= 1 and q["whole"] >= 1, "%s: %s" % (row_id, q)
  # as tests/test_launch_paths_gpu.py: the finished episodes of the sgw_step engine's own arrays, which equal the oracle's (above)
  st, cum = got["step_type"], got["cumulative"].reshape(row["n"], S + 1, -1)
  c["returns"] = {s: LP.finished_returns(st[:, :s + 1], cum[:, :s + 1]) for s in {S0, S}}
  ref.close()
  _MA_CASES[row_id] = c
  return c


@pytest.mark.parametrize("path", ("step_n", "replay"))
@pytest.mark.parametrize("row_id", [r["id"] for r in AD.MA_ROWS])
def test_multi_agent_launch_path_with_quit_matches_oracle(row_id, path):
  c = ma_case(row_id)
  row, spec, acts = c["row"], c["spec"], c["acts"]
  eng = make_engine(row, spec, c["inp"])
  start(eng, row)
  buf = torch.empty_like(acts[:T])
  calls, n_calls = [], row["calls"]
  for k in range(n_calls):
    if path == "step_n":                          # call 0: direct launches, call 1: capture + replay, later calls: replay
      buf.copy_(acts[k * T:(k + 1) * T])
      o = eng.step_n(buf, write_every=True, accumulate=True)
    else:
      o = eng.replay(acts[k * T:(k + 1) * T], write_every=True, accumulate=True)
    calls.append({f: v.clone() for f, v in o.items()})
  ret = eng.read_returns()
  state = eng.get_state()[:, :row["n"]].clone()
  calls.append({f: v.clone() for f, v in eng.rollout(T, AD.SEED, step0=n_calls * T, write_every=True, accumulate=True).items()})
  ret_after = eng.read_returns()
  state_after = eng.get_state()[:, :row["n"]]
  torch.cuda.synchronize()
  for k, o in enumerate(calls):
    check(c, to_np(o, True), 1 + k * T, "%s call %d" % (path if k < n_calls else "rollout after " + path, k))
  # the whole state, the PCG64 words among them (compared with the oracle's in ma_case)
  assert torch.equal(state, c["states"][n_calls * T]), "%s %s: final state differs from the sgw_step engine" % (row_id, path)
  assert torch.equal(state_after, c["states"][(n_calls + 1) * T]), "%s rollout after %s: state" % (row_id, path)
  check_returns(c, ret, n_calls * T, path)
  check_returns(c, ret_after, (n_calls + 1) * T, "rollout after " + path)
  eng.close()


@pytest.mark.parametrize("row_id", [r["id"] for r in AD.MA_ROWS])
def test_what_follows_a_multi_agent_quit(row_id):
  """After the row's calls of sgw_step_n: read_returns() sums the finished episodes; the episode log holds one record per row of
  the oracle in which the episode ends, in (t, n) order, with every agent's reason -- QUIT (3) exactly where the oracle has it;
  the PCG64 words of get_state() are the oracle's; the in-launch windows of the QUIT frames and of the frames after the auto-reset
  are the oracle's views."""
  c = ma_case(row_id)
  row, spec, acts, want = c["row"], c["spec"], c["acts"], c["want"]
  n, n_calls = row["n"], row["calls"]
  S, off = n_calls * T, LP.resets(row) - 1
  slots = AD.ma_slots(row, spec)
  eng = make_engine(row, spec, c["inp"])
  start(eng, row)
  log = EpisodeLog(eng, S * n)
  buf = torch.empty_like(acts[:T])
  outs = []
  for k in range(n_calls):
    buf.copy_(acts[k * T:(k + 1) * T])
    outs.append({f: v.clone() for f, v in eng.step_n(buf, write_every=True, accumulate=True).items()})
    eng.log_episodes(log, step_base=k * T)
  ret = eng.read_returns()
  state = eng.get_state()[:, :n].cpu().numpy()
  count = log.count()
  rec = {k: v.cpu().numpy() for k, v in log.records().items()}
  eng.close()
  check_returns(c, ret, S, "what follows a QUIT")
  assert not LP.rng_mismatch(row, state, want, S), "%s: generator position after %d steps" % (row_id, S)
  st, tr = want["step_type"][:, off + 1:off + S + 1], want["term_reason"][:, off + 1:off + S + 1]
  ended = (st[:, :, slots] >= 2).all(axis=2) if getattr(spec, "per_agent", False) else st[:, :, slots[0]] == 2
  ts, ns = np.nonzero(ended.T)                                       # row-major: (t, n) order
  assert count == len(ts) == c["returns"][S][-1] and count <= S * n
  assert np.array_equal(rec["env"], ns) and np.array_equal(rec["step"], ts)
  got_tr = rec["term_reason"].astype(np.int64).reshape(count, -1)
  want_tr = tr[ns, ts][:, slots if getattr(spec, "per_agent", False) else slots[:1]].astype(np.int64)
  assert np.array_equal(got_tr[:, :want_tr.shape[1]], want_tr)
  quit_rows = (want_tr == AD.QUIT).any(axis=1)
  assert quit_rows.sum() >= 1 and np.array_equal((got_tr[:, :want_tr.shape[1]] == AD.QUIT).any(axis=1), quit_rows)
  assert np.array_equal(rec["length"], want["frame"][ns, ts + off + 1])
  # the windows written by the launches, on the QUIT frames and on the frames that follow them (the auto-reset)
  views = [np.concatenate(p, axis=1) for p in zip(*[LP.split_views(spec, to_np(o, True)["views"]) for o in outs])]    # per agent [E, S, h, w]
  qn, qt = ns[quit_rows], ts[quit_rows]
  nxt = qt + 1 < S
  for e_idx, t_idx in ((qn, qt), (qn[nxt], qt[nxt] + 1)):
    for a in slots:
      w = (want["view_worker"][:, :, a] if a < 2 else want["view_supervisor"]) if row["oracle"] == "ma" else want["view"][:, :, a]
      assert np.array_equal(views[a][e_idx, t_idx], w[e_idx, t_idx + off + 1]), "%s: window of agent %d" % (row_id, a)
  assert (want["step_type"][qn[nxt], qt[nxt] + off + 2][:, slots] == 0).all(), "the round after a QUIT round is the auto-reset"
