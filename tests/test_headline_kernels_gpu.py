"""Kernel x feature for the headline (island_navigation_ex level 9, default parameters): every feature whose tests build a default
level 9 engine, on each of the four kernels that can step it (tests/headline_kernels.py: fork, one_wave, shape_only, generic), at
test sizes.  sgw_create picks the kernel silently and by size, so without this file a feature is checked on whichever kernel the
default selection happens to run at 65 envs.  select() fixes the kernel for the whole test and asserts the
(sgw_step_rules, sgw_step_shape, sgw_step_fork) triple of EVERY engine the test creates, forks, lookahead twins and the
facades' engines included.  Every cell is compared with the C oracle or with the feature's own host reference, bit for bit, NaN
== NaN; the helpers, schedules and assertions are those of the feature's own test file, called from here:

  (a) masked resets       the island_ex_L9_shaped row (333 envs, max_iterations 15) through (a), (b), (e), (f) of
                          tests/test_masked_reset_gpu.py
  (b) QUIT, 0, 5..8       the `_quitlate` tape of tests/action_domain.py on the default spec, 48 steps at 1, 65 and 257 envs, as
                          three sgw_step_n calls over one buffer and as 48 sgw_step calls: every output of FIELDS, the returns
                          exactly, the episode log against the oracle's ends (term_reason QUIT among them)
  (c) packed state        island_default_655 of tests/state_fields.py (cumulative rewards at -32750 in 10 state words) through the
                          step path, replay, checkpoint and log of tests/test_state_fields_gpu.py; island_default_656 (the plain
                          state, 22 words) has no compiled rules to run
  (d) ragged returns      island_shaped of tests/test_returns_ragged_gpu.py (max_iterations 5, 24 steps) at 1, 63, 65, 129 envs
                          through `step` and `step_n` (the fused `rollout` runs no step kernel: once)
  (e) closed loop         run_twins and the hand-written route of tests/test_policy_step_n_gpu.py, the sampled chain of
                          tests/test_softmax_gpu.py: the step launch inside a captured 2T + 1 chain; the recorded outputs also
                          against the oracle on the recorded tape
  (f) copy, fork, lookahead   the fork that stays equal across episode ends and the one-step lookahead of
                          tests/test_copy_envs_gpu.py on the default spec at 130 and 70 envs, the fork's continued run and every
                          candidate's step also against the oracle
  (g) facades             BatchedSafetyEnvironment(scalarise=True, track_performance=True) and GridworldVectorEnv(episode_log=)
                          at 65 envs, 32 steps against the oracle and tests/scalarise_ref.py

Sizes: 1 (a lone lane), 63 / 65 (a ragged first / second wave), 129 / 257 (a last workgroup with dead env-waves for two / four
env-waves per workgroup); tests/test_headline_kernels.py checks the tapes' conditions on the oracle alone.

Measured on one MI355X, the file run alone: 4.6 s for its 125 tests, oracle runs included; the slowest is
test_masked_resets_after_every_call[fork] with 0.67 s (it builds the row's schedule and oracle records, which the other cells
reuse), every other test stays under 0.1 s."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine, EpisodeLog
from ai_safety_gridworlds_amd.environments import BatchedSafetyEnvironment
from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldVectorEnv
from ai_safety_gridworlds_amd.specs import make_spec
from tests import action_domain as AD
from tests import headline_kernels as HK
from tests import launch_paths as LP
from tests import scalarise_ref as R
from tests import state_fields as SF
from tests import test_copy_envs_gpu as CE
from tests import test_masked_reset_gpu as MR
from tests import test_policy_step_n_gpu as PS
from tests import test_returns_ragged_gpu as RR
from tests import test_softmax_gpu as SM
from tests import test_state_fields_gpu as SFG
from tests.test_headline_prologue_gpu import FIELDS, _returns
from tests.test_step_fork_gpu import _compare

pytestmark = pytest.mark.gpu

DEV = LP.DEV
NAME = HK.NAME
kernels = pytest.mark.parametrize("kernel", HK.IDS)


# ---- (a) masked resets --------------------------------------------------------------------------------------------------------------
RESET_ROW = "island_ex_L9_shaped"


@kernels
def test_masked_resets_after_every_call(kernel, monkeypatch):
  """(a) and (b) of tests/test_masked_reset_gpu.py: every call of the schedule, the state of the un-reset envs unchanged."""
  made = HK.select(kernel, monkeypatch)
  MR.every_call(RESET_ROW)
  assert len(made) == 1


@pytest.mark.parametrize("path", ("step_n", "replay"))
@kernels
def test_masked_resets_before_captured_and_replayed_calls(kernel, path, monkeypatch):
  """(e): three sgw_step_n calls with a reset before the third, and the same through sgw_replay."""
  made = HK.select(kernel, monkeypatch)
  MR.test_launch_paths_after_ragged_resets(RESET_ROW, path)
  assert len(made) == 1


@kernels
def test_masked_reset_as_the_first_call_of_a_fresh_engine(kernel, monkeypatch):
  """(f): the never-reset envs start their episode on their first step."""
  made = HK.select(kernel, monkeypatch)
  MR.test_never_reset_envs_start_at_their_first_step(RESET_ROW)
  assert len(made) == 1


# ---- (b) QUIT and actions outside the range ---------------------------------------------------------------------------------------
def _log_equals_the_oracles_ends(log, want, n, S, label):
  """As tests/test_action_domain_gpu.py test_what_follows_a_quit: one record per LAST row of the oracle in (t, n) order."""
  count = log.count()
  rec = {k: v.cpu().numpy() for k, v in log.records().items()}
  ts, ns = np.nonzero((want["step_type"][:, 1:S + 1] == 2).T)
  assert count == len(ts) <= S * n, "%s: %d records, the oracle ends %d episodes" % (label, count, len(ts))
  assert np.array_equal(rec["env"], ns) and np.array_equal(rec["step"], ts), label
  assert np.array_equal(rec["term_reason"].astype(np.int64), want["term_reason"][ns, ts + 1].astype(np.int64)), label
  assert (rec["term_reason"] == AD.QUIT).sum() == AD.quit_lasts(want, S) == HK.QUIT_ENDS[n], label
  assert np.array_equal(rec["length"], want["frame"][ns, ts + 1]), label
  assert rec["ret"].tobytes() == np.ascontiguousarray(want["cumulative"][ns, ts + 1]).tobytes(), label
  assert rec["hidden"].tobytes() == np.ascontiguousarray(want["hidden"][ns, ts + 1]).tobytes(), label
  m = want["metrics"].shape[-1]
  assert LP._same(rec["metrics"][:, :m], want["metrics"][ns, ts + 1]), label


@pytest.mark.parametrize("n", HK.QUIT_NS)
@pytest.mark.parametrize("path", ("step_n", "step"))
@kernels
def test_quit_and_out_of_range_actions(kernel, path, n, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  tape, want = HK.quit_case(n)
  T, S = HK.QUIT_T, HK.QUIT_STEPS
  label = "%s %s n=%d" % (kernel, path, n)
  dev = torch.from_numpy(tape).to(DEV)
  eng = BatchedEngine(make_spec(NAME), n, device=DEV, outputs=FIELDS)
  log = EpisodeLog(eng, S * n)
  first = {k: v.clone() for k, v in eng.reset().items()}
  if path == "step_n":                                   # one buffer refilled in place: direct launches, capture, replay
    buf = torch.empty_like(dev[:T])
    for call in range(HK.QUIT_CALLS):
      buf.copy_(dev[call * T:(call + 1) * T])
      got = {k: v.clone() for k, v in eng.step_n(buf, write_every=True, accumulate=True).items()}
      eng.log_episodes(log, step_base=call * T)
      _compare(got, want, 1 + call * T, n, FIELDS, "%s call %d" % (label, call))
    r, w = eng.read_returns().cpu().numpy(), _returns(want, S)
    assert w[-1] >= HK.QUIT_ENDS[n] and np.array_equal(r, w), "%s: returns %s, the oracle's %s" % (label, r, w)
  else:
    rec = {k: [v] for k, v in first.items()}
    for t in range(S):
      for k, v in eng.step(dev[t]).items():
        rec[k].append(v.clone())
      eng.log_episodes(log, step_base=t)
    _compare({k: torch.stack(v) for k, v in rec.items()}, want, 0, n, FIELDS, label)
  _log_equals_the_oracles_ends(log, want, n, S, label)
  eng.close()
  assert len(made) == 1


# ---- (c) the packed state at its limit ----------------------------------------------------------------------------------------------
@kernels
def test_packed_state_at_its_limit(kernel, monkeypatch):
  """island_default_655 through the step path (with the log of the end window), the fused replay and the checkpoint of
  tests/test_state_fields_gpu.py, whose run cache is emptied for the test: the step path it compares with is this kernel's."""
  made = HK.select(kernel, monkeypatch)
  monkeypatch.setattr(SFG, "_RUNS", {})
  case = SF.BY_ID["island_default_655"]
  assert case["state_words"] == 10 and case["kw"] == dict(level=9, max_iterations=655)       # (_run asserts sgw_state_words)
  SFG.test_step_path_matches_the_oracle_at_the_limit(case["id"])
  SFG.test_fused_replay_matches_the_step_path_at_the_limit(case["id"])
  SFG.test_checkpoint_one_step_before_the_limit_resumes_bit_for_bit(case["id"])
  assert len(made) == 3 and SFG._RUNS[case["id"]]["log"] is not None


def test_one_step_past_the_packable_limit_runs_generic_rules(monkeypatch):
  """island_default_656 does not pack: 22 state words, and with the default selection no compiled rules.  (Not a row of the
  table: the one shaped entry of csrc/sgw_api.hip is the packed state's, so the plain state steps with its generic kernel.)"""
  HK.select("fork", monkeypatch, watch=False)
  case = SF.BY_ID["island_default_656"]
  eng = BatchedEngine(SF.spec_of(case), 65, device=DEV, outputs=("step_type",))
  try:
    assert N.lib().sgw_state_words(eng._h) == 22 == case["state_words"]
    assert HK.triple_of(eng) == (0, 0, 0), "only the packed state has a shaped kernel, and with it compiled rules and a fork"
  finally:
    eng.close()


# ---- (d) ragged returns -------------------------------------------------------------------------------------------------------------
def _ragged(n, path):
  c = RR.case("island_shaped", n)
  assert c["last"].any(axis=1).all()
  r, _ = RR._play(LP.make_engine(c["row"], c["spec"], c["inp"]), c, path)
  w = c["returns"]
  assert r[-1] == w[-1], "n=%d %s: %d finished episodes, the oracle has %d" % (n, path, r[-1], w[-1])
  assert np.array_equal(r, w), "n=%d %s: returns %s, the oracle's %s" % (n, path, r, w)


@pytest.mark.parametrize("path", ("step", "step_n"))
@pytest.mark.parametrize("n", RR.NS)
@kernels
def test_ragged_returns(kernel, n, path, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  _ragged(n, path)
  assert len(made) == 1


@pytest.mark.parametrize("n", RR.NS)
def test_ragged_returns_of_the_fused_rollout(n, monkeypatch):
  made = HK.select("fork", monkeypatch)
  _ragged(n, "rollout")
  assert len(made) == 1


# ---- (e) the closed loop ------------------------------------------------------------------------------------------------------------
LOOP_T = 8                                               # the capture threshold: the second call is captured, the third replayed


def _recorded_run_equals_the_oracle(record, write_every, label):
  """The calls' outputs of engine A (run_twins / _closed_loop) against the oracle on A's recorded tape."""
  from oracle import oracle as O
  tape = np.concatenate([t[:, :, 0] for t in record["tapeA"]])             # [calls * T, N]
  fields = sorted(record["A"][0])
  want = O.run_streams(O.make_config(NAME), tape.T.copy(), fields=fields, nthreads=8)
  n = tape.shape[1]
  assert (want["step_type"][:, 1:] == 2).any(), "no episode ends inside the chain"
  for call, res in enumerate(record["A"]):
    got = {k: torch.from_numpy(v if write_every else v[None]) for k, v in res.items()}
    _compare(got, want, 1 + call * LOOP_T if write_every else (call + 1) * LOOP_T, n, fields, "%s call %d" % (label, call))


@pytest.mark.parametrize("write_every", [False, True])
@kernels
def test_greedy_closed_loop(kernel, write_every, monkeypatch):
  """run_twins: four policy_step_n calls (direct, captured, replayed, replayed over rewritten tables; accumulate on the second)
  against a host loop of act + step and against step_n over the tape, on forks."""
  made = HK.select(kernel, monkeypatch)
  _, record = PS.run_twins(NAME, dict(level=9), "board", LOOP_T, write_every)
  _recorded_run_equals_the_oracle(record, write_every, "%s greedy" % kernel)
  assert len(made) == 4


@pytest.mark.parametrize("write_every", [False, True])
@kernels
def test_sampled_closed_loop(kernel, write_every, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  record = {}
  SM._closed_loop("island_l9_board", write_every, SM.BETAS[1], "ssss", record=record)
  _recorded_run_equals_the_oracle(record, write_every, "%s sampled" % kernel)
  assert len(made) == 4


@kernels
def test_hand_written_route(kernel, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  PS.test_per_cell_route_against_the_oracle()
  assert len(made) == 1


# ---- (f) copy, fork, lookahead ------------------------------------------------------------------------------------------------------
_DEFAULT = {}


def _default_case(n, what):
  """Per (n, what), cached: the row of the default spec at n envs, its spec and inputs, and the oracle's arrays -- what == "fork":
  of the FORK_STEPS steps of the fork check's tape; "look": per candidate b, of the LOOK_AT steps and then candidate b's."""
  if (n, what) not in _DEFAULT:
    row = LP._row("island_default_n%d" % n, NAME, {}, n, None)
    spec = make_spec(NAME)
    inp = LP.inputs(row, spec, 0)
    ids = np.arange(n)
    stream = lambda seed, steps: philox.actions(seed, ids, np.arange(steps), spec.action_lo, spec.n_actions).astype(np.int8)
    if what == "fork":
      want = LP.run_oracle(row, stream(CE.FORK_SEED, CE.FORK_STEPS), inp)
    else:
      before, cand = stream(CE.LOOK_SEED, CE.LOOK_AT), stream(CE.LOOK_CAND_SEED, CE.LOOK_B)
      want = [LP.run_oracle(row, np.concatenate([before, cand[b:b + 1]]), inp) for b in range(CE.LOOK_B)]
    _DEFAULT[(n, what)] = (row, spec, inp, want)
  return _DEFAULT[(n, what)]


@pytest.mark.parametrize("n", (CE.N_SRC, CE.N_DST))
@kernels
def test_fork_stays_equal_and_continues_as_the_oracle(kernel, n, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  row, spec, inp, want = _default_case(n, "fork")
  rec = CE.fork_stays_equal(row, LP.make_engine(row, spec, inp))
  assert (want["step_type"][:, CE.FORK_AT + 1:] == 2).any()
  assert LP.oracle_mismatches(row, spec, LP.to_np(rec, True), want, CE.FORK_AT + 1) == []
  assert len(made) == 2


@pytest.mark.parametrize("n", (CE.N_SRC, CE.N_DST))
@kernels
def test_lookahead_is_the_oracles_next_step(kernel, n, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  row, spec, inp, wants = _default_case(n, "look")
  res = CE.lookahead_is_the_step_not_taken(row, LP.make_engine(row, spec, inp), LP.make_engine(row, spec, inp))
  for b, want in enumerate(wants):
    got = {k: v[b].cpu().numpy()[:, None] for k, v in res.items()}
    assert LP.oracle_mismatches(row, spec, got, want, CE.LOOK_AT + 1) == [], "candidate %d" % b
  assert len(made) == 3, "the engine, the snapshot's engine and lookahead()'s cached fork"


# ---- (g) the facades ----------------------------------------------------------------------------------------------------------------
FACADE_N, FACADE_T, FACADE_SEED = 65, 32, 0xFACADE
_FACADE = {}


def _facade_case():
  """The tape (the spec's Philox stream), the oracle's arrays and, from them alone, what the facades derive: the three scalar
  sums per step, and per env the last finished episode's return, the left-to-right sum of the returns and their count."""
  if not _FACADE:
    row = LP._row("island_default_facade", NAME, {}, FACADE_N, None)
    spec = make_spec(NAME)
    tape = philox.actions(FACADE_SEED, np.arange(FACADE_N), np.arange(FACADE_T), spec.action_lo, spec.n_actions).astype(np.int8)
    want = LP.run_oracle(row, tape, LP.inputs(row, spec, 0))
    K = want["cumulative"].shape[-1]
    last, sums, cnt = np.full((FACADE_N, K), np.nan), np.zeros((FACADE_N, K)), np.zeros(FACADE_N, np.int64)
    for t in range(1, FACADE_T + 1):
      for e in np.nonzero(want["step_type"][:, t] == 2)[0]:
        last[e] = want["cumulative"][e, t]
        sums[e] = sums[e] + last[e]
        cnt[e] += 1
    assert (cnt > 0).any() and (cnt > 1).any()
    with np.errstate(all="ignore"):
      mean = sums / cnt.astype(np.float64)[:, None]
    _FACADE.update(row=row, spec=spec, tape=tape, want=want, last=R.loop_sums(last), overall=R.loop_sums(mean), episodes=cnt,
                   scalar_reward=R.loop_sums(want["reward"]), scalar_cumulative=R.loop_sums(want["cumulative"]),
                   scalar_average=R.loop_averages(want["cumulative"], want["frame"]))
  return _FACADE


def _nan_equal_bits(got, want):
  nan = np.isnan(want)
  return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and R.same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want))


@kernels
def test_l4_facade_with_scalarise_and_performance(kernel, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  c = _facade_case()
  want = c["want"]
  env = BatchedSafetyEnvironment(NAME, num_envs=FACADE_N, device=DEV, scalarise=True, track_performance=True)
  try:
    HK.assert_selected(env.engine, kernel)
    acts = env.engine.fill_actions(FACADE_T, FACADE_SEED).clone()
    assert np.array_equal(acts.cpu().numpy(), c["tape"])
    scalars = ("scalar_reward", "scalar_cumulative", "scalar_average")
    keep = {k: [] for k in LP.SCALAR_FIELDS + ("metrics", "safety") + scalars + ("ts_reward", "ts_step_type")}
    for t in range(FACADE_T + 1):
      ts = env.reset() if t == 0 else env.step(acts[t - 1])
      for k in keep:
        v = ts.reward if k == "ts_reward" else ts.step_type if k == "ts_step_type" else ts.observation[k]
        keep[k].append(v.clone())
    got = LP.to_np({k: torch.stack(v) for k, v in keep.items()}, True)
    assert LP.oracle_mismatches(c["row"], c["spec"], {k: got[k] for k in LP.SCALAR_FIELDS + ("metrics", "safety")}, want, 0) == []
    assert np.array_equal(got["ts_step_type"].reshape(want["step_type"].shape), want["step_type"])
    for k in scalars:
      assert R.same_bits(got[k].reshape(c[k].shape), c[k]), k
    assert R.same_bits(got["ts_reward"].reshape(c["scalar_reward"].shape), c["scalar_reward"]), "TimeStep.reward is the scalar reward"
    assert np.array_equal(env.episodes_finished().cpu().numpy(), c["episodes"])
    assert _nan_equal_bits(env.get_last_performance().cpu().numpy(), c["last"])
    assert _nan_equal_bits(env.get_overall_performance().cpu().numpy(), c["overall"])
  finally:
    env.close()
  assert len(made) == 1


@kernels
def test_vector_env_with_scalarise_and_episode_log(kernel, monkeypatch):
  made = HK.select(kernel, monkeypatch)
  c = _facade_case()
  want = c["want"]
  env = GridworldVectorEnv(NAME, FACADE_N, device=DEV, scalarise=True, episode_log=FACADE_T * FACADE_N)
  try:
    HK.assert_selected(env._env.engine, kernel)
    acts = torch.from_numpy(c["tape"]).to(DEV)
    env.reset()
    keep = {k: [] for k in ("reward", "done", "board", "cumulative", "hidden", "term_reason", "cumulative_reward", "average_reward")}
    for t in range(FACADE_T):
      obs, reward, done, truncated, info = env.step(acts[t])
      assert not bool(truncated.any())
      for k in keep:
        keep[k].append((reward if k == "reward" else done if k == "done" else info[k]).clone())
    got = LP.to_np({k: torch.stack(v) for k, v in keep.items()}, True)
    sl = slice(1, FACADE_T + 1)
    assert np.array_equal(got["done"], want["step_type"][:, sl] == 2)
    for k, w in (("reward", "scalar_reward"), ("cumulative_reward", "scalar_cumulative"), ("average_reward", "scalar_average")):
      assert R.same_bits(got[k].reshape(FACADE_N, FACADE_T), c[w][:, sl]), k
    for k in ("board", "cumulative", "hidden"):
      assert LP._same(got[k].reshape(want[k][:, sl].shape), want[k][:, sl]), k
    tr = got["term_reason"].astype(np.int16).reshape(FACADE_N, FACADE_T)
    tr[tr == 255] = -1
    assert np.array_equal(tr, want["term_reason"][:, sl])
    rec = {k: v.cpu().numpy() for k, v in env.episode_log.records().items()}
    ts, ns = np.nonzero((want["step_type"][:, sl] == 2).T)
    assert env.episode_log.count() == len(ts) == c["episodes"].sum()
    assert np.array_equal(rec["env"], ns) and np.array_equal(rec["step"], ts)
    assert np.array_equal(rec["length"], want["frame"][ns, ts + 1])
    assert np.array_equal(rec["term_reason"].astype(np.int64), want["term_reason"][ns, ts + 1].astype(np.int64))
    assert rec["ret"].tobytes() == np.ascontiguousarray(want["cumulative"][ns, ts + 1]).tobytes()
  finally:
    env.close()
  assert len(made) == 1
