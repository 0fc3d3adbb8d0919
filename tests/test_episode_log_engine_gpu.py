"""The episode log on real engines: sgw_log_episodes over the [T, N_pad] buffers of step_n / rollout and after every step of the
L4 environment and of both vector wrappers, against the loop `for t: for n < N: if ended: append` over the same arrays, bytes for
bytes.  The seeds are ones for which the CPU oracle shows several finished episodes per env (island_navigation_ex, 100 envs x 64
Philox steps: 804; island_navigation_ex_ma, 70 envs x 96 rounds: 540), and every test asserts count >= N: a log of nothing does not pass."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import ALL_OUTPUTS, BatchedEngine, EpisodeLog
from ai_safety_gridworlds_amd.environments import BatchedSafetyEnvironment
from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldVectorEnv
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv
from ai_safety_gridworlds_amd.specs import make_spec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 1
ISLAND_N, ISLAND_T = 100, 64
IMA_N, IMA_T = 70, 96
SOURCE = {"length": "frame", "term_reason": "term_reason", "ret": "cumulative", "hidden": "hidden", "metrics": "metrics"}


def _loop(spec, bufs, n, step_base=0):
  """for t: for n < N: if ended: append -- over padded numpy buffers [T, N_pad, ...]."""
  st = bufs["step_type"]
  per_agent = bool(getattr(spec, "per_agent", False))
  ts, ns = [], []
  for t in range(st.shape[0]):
    for e in range(n):
      if (st[t, e] >= N.LAST).all() if per_agent else st[t, e, 0] == N.LAST:
        ts.append(t)
        ns.append(e)
  ts, ns = np.array(ts, dtype=np.int64), np.array(ns, dtype=np.int64)
  rec = {"env": ns.astype(np.int32), "step": step_base + ts}
  for f, s in SOURCE.items():
    rec[f] = bufs[s][ts, ns]
  return rec


def _padded(eng, T):
  """The engine's own output buffers of T rows as numpy [T, N_pad(, columns)]."""
  out = {}
  for k in ("step_type", "frame", "term_reason", "cumulative", "hidden", "metrics"):
    a = eng._bufs[k].cpu().numpy()
    out[k] = a.reshape(T, eng.n_pad) if k in ("frame", "hidden") else a.reshape(T, eng.n_pad, -1)
  return out


def _np(records):
  return {k: v.cpu().numpy() for k, v in records.items()}


def _assert_same(got, want, what):
  assert set(got) == set(want), what
  for f in want:
    assert got[f].shape[0] == want[f].shape[0], (what, f, got[f].shape, want[f].shape)
    assert np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), (what, f)


@pytest.fixture(scope="module")
def island_batch():
  """island_navigation_ex, 100 envs, 64 Philox steps through step_n(write_every=True): (actions, the log's records, count)."""
  spec = make_spec("island_navigation_ex")
  eng = BatchedEngine(spec, ISLAND_N, device=DEV, outputs=ALL_OUTPUTS)
  try:
    eng.reset()
    acts = eng.fill_actions(ISLAND_T, SEED)
    eng.step_n(acts, write_every=True)
    log = EpisodeLog(eng, ISLAND_T * ISLAND_N)
    eng.log_episodes(log)
    want = _loop(spec, _padded(eng, ISLAND_T), ISLAND_N)
    count, rec = log.count(), _np(log.records())
    assert not log.overflowed()
    again = EpisodeLog(eng, ISLAND_T * ISLAND_N)                     # from kept copies of the buffers: the `outputs` form
    eng.log_episodes(again, outputs={k: v.clone() for k, v in eng._bufs.items()})
    return dict(spec=spec, acts=acts, want=want, count=count, rec=rec, again=_np(again.records()))
  finally:
    eng.close()


def test_step_n_buffers_give_the_loops_records(island_batch):
  b = island_batch
  assert b["count"] == len(b["want"]["env"]) >= ISLAND_N, "several finished episodes per env (the oracle shows 804)"
  _assert_same(b["rec"], b["want"], "step_n")
  _assert_same(b["again"], b["want"], "outputs=")
  assert b["rec"]["ret"].shape[1:] == (b["spec"].K,) and b["rec"]["metrics"].shape[1:] == (b["spec"].M,)
  assert (b["rec"]["length"] > 0).all() and (b["rec"]["term_reason"] != N.TERM_NONE).all()


def test_rollout_gives_the_same_log(island_batch):
  eng = BatchedEngine(island_batch["spec"], ISLAND_N, device=DEV, outputs=ALL_OUTPUTS)
  try:
    eng.reset()
    eng.rollout(ISLAND_T, SEED, step0=0, write_every=True)
    log = EpisodeLog(eng, ISLAND_T * ISLAND_N)
    eng.log_episodes(log)
    assert log.count() == island_batch["count"]
    _assert_same(_np(log.records()), island_batch["want"], "rollout")
  finally:
    eng.close()


def test_missing_output_is_refused():
  eng = BatchedEngine(make_spec("island_navigation_ex"), 10, device=DEV, outputs=("board", "step_type", "cumulative"))
  try:
    eng.reset()
    with pytest.raises(N.SgwError):
      eng.log_episodes(EpisodeLog(eng, 10))                          # keeps length / hidden / ...: their outputs were not asked for
    log = EpisodeLog(eng, 10, fields=("env", "step", "ret"))
    eng.log_episodes(log)
    assert log.count() == 0 and log.records()["ret"].shape == (0, eng.spec.K)
    other = BatchedEngine(make_spec("boat_race"), 10, device=DEV)
    try:
      with pytest.raises(N.SgwError):
        other.log_episodes(log)                                      # a log made for another engine's record layout
    finally:
      other.close()
  finally:
    eng.close()


def test_one_step_at_a_time_through_the_environment(island_batch):
  """The same 64 steps through BatchedSafetyEnvironment(episode_log=cap): the same log; and the log's performances reproduce the
  device-side bookkeeping of sgw_track_performance env by env, bit for bit."""
  acts = island_batch["acts"]
  env = BatchedSafetyEnvironment("island_navigation_ex", num_envs=ISLAND_N, device=DEV, track_performance=True,
                                 episode_log=ISLAND_T * ISLAND_N)
  try:
    env.reset()
    for t in range(ISLAND_T):
      env.step(acts[t])
    assert env.episode_log.count() == island_batch["count"] >= ISLAND_N
    _assert_same(_np(env.episode_log.records()), island_batch["want"], "one step at a time")
    envs, perf = env.episodic_performances()
    envs, perf = envs.cpu().numpy(), perf.cpu().numpy()
    cols = perf.shape[1]
    sums, last, cnt = np.zeros((ISLAND_N, cols)), np.full((ISLAND_N, cols), np.nan), np.zeros(ISLAND_N, np.int64)
    for e, p in zip(envs, perf):                                     # the reference's left-to-right sum(performances)
      sums[e] = sums[e] + p
      last[e] = p
      cnt[e] += 1
    assert sums.tobytes() == env._performance_sum.cpu().numpy().tobytes()
    assert np.array_equal(cnt, env.episodes_finished().cpu().numpy())
    assert np.array_equal(last, env.get_last_performance().cpu().numpy(), equal_nan=True)
    assert (cnt > 0).all()
  finally:
    env.close()


def test_island_ma_rounds_with_per_agent_reasons():
  spec = make_spec("island_navigation_ex_ma")
  eng = BatchedEngine(spec, IMA_N, device=DEV, outputs=ALL_OUTPUTS)
  try:
    eng.set_rng_seeds(321 + SEED + np.arange(IMA_N))
    eng.reset()
    acts = eng.fill_actions(IMA_T, SEED)
    eng.step_n(acts, write_every=True)
    log = EpisodeLog(eng, IMA_T * IMA_N)
    eng.log_episodes(log, step_base=7)
    want = _loop(spec, _padded(eng, IMA_T), IMA_N, step_base=7)
    assert log.count() == len(want["env"]) >= IMA_N
    rec = _np(log.records())
    assert rec["term_reason"].shape[1:] == (spec.A,) and rec["ret"].shape[1:] == (spec.A, spec.K)
    rec["ret"] = rec["ret"].reshape(len(rec["env"]), -1)
    _assert_same(rec, want, "island_navigation_ex_ma")
    assert (rec["term_reason"] != N.TERM_NONE).all(), "reasons are set once every agent is done"
  finally:
    eng.close()


def test_gridworld_vector_env_logs_what_its_steps_returned(island_batch):
  acts = island_batch["acts"]
  env = GridworldVectorEnv("island_navigation_ex", ISLAND_N, device=DEV, episode_log=ISLAND_T * ISLAND_N)
  try:
    assert isinstance(env.episode_log, EpisodeLog)
    env.reset()
    got = {k: [] for k in ("env", "step", "ret", "hidden", "term_reason", "length", "metrics")}
    for t in range(ISLAND_T):
      obs, reward, done, trunc, info = env.step(acts[t])
      idx = torch.nonzero(done).reshape(-1)                          # what a caller does today, with a synchronisation per step
      got["env"].append(idx.to(torch.int32).cpu().numpy())
      got["step"].append(np.full(len(idx), t, np.int64))
      got["ret"].append(info["cumulative"][idx].cpu().numpy())
      got["hidden"].append(info["hidden"][idx].cpu().numpy())
      got["term_reason"].append(info["term_reason"][idx].cpu().numpy())
      got["length"].append(env._env._last["frame"][idx].cpu().numpy())
      got["metrics"].append(env._env._last["metrics"][idx].cpu().numpy())
    got = {k: np.concatenate(v) for k, v in got.items()}
    assert env.episode_log.count() == len(got["env"]) >= ISLAND_N
    _assert_same(_np(env.episode_log.records()), got, "GridworldVectorEnv")
    _assert_same(_np(env.episode_log.records()), island_batch["want"], "GridworldVectorEnv against step_n")
  finally:
    env.close()


def test_zoo_vector_env_logs_what_its_steps_returned():
  env = GridworldZooVectorEnv("island_navigation_ex_ma", IMA_N, device=DEV, seed=321 + SEED, episode_log=IMA_T * IMA_N)
  try:
    sp, eng = env.spec_, env._env.engine
    assert isinstance(env.episode_log, EpisodeLog)
    env.reset()
    acts = eng.fill_actions(IMA_T, SEED)
    got = {k: [] for k in ("env", "step", "ret", "metrics", "term_reason")}
    slots = env._slots
    for t in range(IMA_T):
      obs, rewards, terms, truncs, infos = env.step(acts[t])
      done = torch.stack([terms[a] for a in env.possible_agents], dim=1).all(dim=1)
      idx = torch.nonzero(done).reshape(-1)
      got["env"].append(idx.to(torch.int32).cpu().numpy())
      got["step"].append(np.full(len(idx), t, np.int64))
      ret = np.zeros((len(idx), sp.A, sp.K))
      for i, a in enumerate(env.possible_agents):
        ret[:, slots[i], :env._k[a]] = infos[a]["cumulative_reward"][idx].cpu().numpy()
      got["ret"].append(ret)
      got["metrics"].append(infos[env.possible_agents[0]]["metrics"][idx].cpu().numpy())
      got["term_reason"].append(env._env._last["term_reason"][idx].cpu().numpy())
    got = {k: np.concatenate(v) for k, v in got.items()}
    rec = _np(env.episode_log.records())
    assert env.episode_log.count() == len(got["env"]) >= IMA_N
    for i, a in enumerate(env.possible_agents):                      # the columns an agent has; the others are the engine's own
      k = env._k[a]
      assert rec["ret"][:, slots[i], :k].tobytes() == got["ret"][:, slots[i], :k].tobytes(), a
    for f in ("env", "step", "metrics", "term_reason"):
      assert np.ascontiguousarray(rec[f]).tobytes() == np.ascontiguousarray(got[f]).tobytes(), f
    assert (rec["length"] > 0).all()
  finally:
    env.close()
