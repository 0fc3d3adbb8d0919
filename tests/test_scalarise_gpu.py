"""GPU tier of scalarise=True: the kernel on synthetic tensors through the C ABI, the reference's fixtures replayed through the
L4 facade, a 130-env run on every way the sums can be asked for (step, step_n + scalarise(T), under graph capture), and the L5
facades.  Expected values always come from the explicit left-to-right loop of tests/scalarise_ref.py, bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.environments import BatchedSafetyEnvironment
from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldGymEnv, GridworldVectorEnv
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_aec_env import GridworldZooAecEnv
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_parallel_env import GridworldZooParallelEnv
from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv
from ai_safety_gridworlds_amd.specs import make_spec
from tests import scalarise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ERR_ARG = -1
SENTINEL = -777.25
SPECS = {"island": ("island_navigation_ex", dict(level=9)), "savanna": ("aintelope_savanna", dict(amount_agents=2))}
# k_agent per engine: None = NULL (K for every agent); different per agent, 0 included
K_SETS = {"island": (None, [10], [3], [0]), "savanna": (None, [4, 0], [2, 3], [0, 4])}


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def engines():
  made = {}

  def get(kind, n):
    if (kind, n) not in made:
      name, kw = SPECS[kind]
      made[(kind, n)] = BatchedEngine(make_spec(name, **kw), n, device=DEV, outputs=("reward", "cumulative", "frame", "step_type"))
    return made[(kind, n)]

  yield get
  for e in made.values():
    e.close()


def _dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _karr(ks):
  return None if ks is None else (C.c_int32 * N.MAX_AGENTS)(*(list(ks) + [0] * (N.MAX_AGENTS - len(ks))))


def _synthetic(rng, T, n, n_pad, A, K):
  """reward / cumulative [T, n_pad, A, K] and frame [T, n_pad]: integers, fractions and magnitudes 1e-3 .. 1e12 mixed, so that
  the order of the additions shows in the last bits; padding rows hold NaN and a frame of -1 (a division by zero if it were read)."""
  def values():
    v = rng.integers(-60, 60, size=(T, n_pad, A, K)).astype(np.float64)
    v += rng.choice([0.0, 0.1, 1.0 / 3.0, 1e-3], size=v.shape)
    v *= rng.choice([1.0, 1.0, 1e3, 1e12], size=v.shape)
    v[:, n:] = np.nan
    return v
  reward, cum = values(), values()
  frame = rng.integers(0, 100, size=(T, n_pad)).astype(np.int32)
  frame[:, n:] = -1
  rows = [(t, i) for t in range(T) for i in range(n)]
  special = {}
  if len(rows) >= 3:
    special = {"negzero": rows[0], "cancel": rows[len(rows) // 2], "nan": rows[-1]}
    for arr in (reward, cum):
      arr[special["negzero"]] = -0.0
      arr[special["cancel"]] = 0.0
      arr[special["cancel"]][:, :4] = (1e16, 1.0, -1e16, 1.0)
      arr[special["nan"]][:, 0] = np.nan
  return reward, cum, frame, special


def _expected(reward, cum, frame, n, ks, K):
  A = reward.shape[2]
  ks = [K] * A if ks is None else ks
  want = [np.zeros(reward.shape[:3]) for _ in range(3)]
  for a in range(A):
    want[0][:, :n, a] = R.loop_sums(reward[:, :n, a], ks[a])
    want[1][:, :n, a] = R.loop_sums(cum[:, :n, a], ks[a])
    want[2][:, :n, a] = R.loop_averages(cum[:, :n, a], frame[:, :n], ks[a])
  return want


def _check(got, want, n, what):
  got = got.cpu().numpy()
  assert R.same_bits(got[:, n:], np.full_like(got[:, n:], SENTINEL)), "%s: a padding row was written" % what
  g, w = got[:, :n], want[:, :n]
  nan = np.isnan(w)
  assert (np.isnan(g) == nan).all(), "%s: NaN rows differ" % what
  assert R.same_bits(np.where(nan, 0.0, g), np.where(nan, 0.0, w)), "%s: %d of %d values differ, first want %r got %r" % (
      what, int((g != w).sum()), g.size, w[(g != w) & ~nan][:1], g[(g != w) & ~nan][:1])


# ---- 1. the kernel on synthetic tensors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("kind", ["island", "savanna"])
def test_kernel_on_synthetic_rows(engines, kind, n, T):
  e = engines(kind, n)
  A, K = e.spec.A, e.spec.K
  assert (A, K) == {"island": (1, 10), "savanna": (2, 4)}[kind]
  rng = np.random.default_rng(1000 * n + 10 * T + A)
  reward, cum, frame, special = _synthetic(rng, T, n, e.n_pad, A, K)
  d_reward, d_cum, d_frame = _dev(reward), _dev(cum), _dev(frame)
  for ks in K_SETS[kind]:
    outs = [torch.full((T, e.n_pad, A), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(3)]
    rc = e._lib.sgw_scalarise(e._h, d_reward.data_ptr(), d_cum.data_ptr(), d_frame.data_ptr(), T, _karr(ks),
                              outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), _stream())
    assert rc == 0, e._lib.sgw_last_error()
    torch.cuda.synchronize()
    want = _expected(reward, cum, frame, n, ks, K)
    for o, w, nm in zip(outs, want, ("scalar_reward", "scalar_cumulative", "scalar_average")):
      _check(o, w, n, "%s k_agent=%s" % (nm, ks))
    full = [K] * A if ks is None else ks
    if special:
      for a in range(A):
        t, i = special["negzero"]
        for o in outs:                       # a row of -0.0 sums to +0.0 (the accumulator starts at +0.0), also with k == 0
          v = o[t, i, a].item()
          assert v == 0.0 and not np.signbit(v)
        t, i = special["cancel"]
        if full[a] >= 4:                       # (the columns past the fourth hold 0.0)
          assert outs[0][t, i, a].item() == 1.0 and outs[1][t, i, a].item() == 1.0      # pairwise / reversed / compensated orders give 2.0 or 0.0
        t, i = special["nan"]
        assert np.isnan(outs[0][t, i, a].item()) == (full[a] > 0)


def test_every_output_subset(engines):
  e = engines("island", 65)
  A, K, T, n = e.spec.A, e.spec.K, 1, 65
  reward, cum, frame, _ = _synthetic(np.random.default_rng(5), T, n, e.n_pad, A, K)
  d = {"reward": _dev(reward), "cumulative": _dev(cum), "frame": _dev(frame)}
  want = _expected(reward, cum, frame, n, None, K)
  needs = ({"reward"}, {"cumulative"}, {"cumulative", "frame"})
  for subset in itertools.product((False, True), repeat=3):
    if not any(subset):
      continue
    outs = [torch.full((T, e.n_pad, A), SENTINEL, dtype=torch.float64, device=DEV) for _ in range(3)]
    need = set().union(*[needs[j] for j in range(3) if subset[j]])
    src = [d[k].data_ptr() if k in need else None for k in ("reward", "cumulative", "frame")]     # a source nobody asks for may be NULL
    ptrs = [outs[j].data_ptr() if subset[j] else None for j in range(3)]
    assert e._lib.sgw_scalarise(e._h, src[0], src[1], src[2], T, None, ptrs[0], ptrs[1], ptrs[2], _stream()) == 0, (subset, e._lib.sgw_last_error())
    torch.cuda.synchronize()
    for j in range(3):
      if subset[j]:
        _check(outs[j], want[j], n, "subset %s output %d" % (subset, j))
      else:
        assert (outs[j] == SENTINEL).all()


def test_bad_arguments(engines):
  e = engines("savanna", 65)
  L, A, K = e._lib, e.spec.A, e.spec.K
  r = torch.zeros((e.n_pad, A, K), dtype=torch.float64, device=DEV)
  f = torch.zeros(e.n_pad, dtype=torch.int32, device=DEV)
  o = torch.full((e.n_pad, A), SENTINEL, dtype=torch.float64, device=DEV)
  R_, F_, O_ = r.data_ptr(), f.data_ptr(), o.data_ptr()
  s = _stream()
  assert L.sgw_scalarise(None, R_, R_, F_, 1, None, O_, O_, O_, s) == ERR_ARG
  for T in (0, -1):
    assert L.sgw_scalarise(e._h, R_, R_, F_, T, None, O_, O_, O_, s) == ERR_ARG
  for bad in ([-1, 0], [K + 1, 0], [0, K + 1], [0, -3]):
    assert L.sgw_scalarise(e._h, R_, R_, F_, 1, _karr(bad), O_, O_, O_, s) == ERR_ARG, bad
    assert b"k_agent" in L.sgw_last_error()
  assert L.sgw_scalarise(e._h, R_, R_, F_, 1, None, None, None, None, s) == ERR_ARG, "all three outputs NULL"
  assert L.sgw_scalarise(e._h, None, R_, F_, 1, None, O_, None, None, s) == ERR_ARG, "scalar_reward needs reward"
  assert L.sgw_scalarise(e._h, R_, None, F_, 1, None, None, O_, None, s) == ERR_ARG, "scalar_cumulative needs cumulative"
  assert L.sgw_scalarise(e._h, R_, None, F_, 1, None, None, None, O_, s) == ERR_ARG, "scalar_average needs cumulative"
  assert L.sgw_scalarise(e._h, R_, R_, None, 1, None, None, None, O_, s) == ERR_ARG, "scalar_average needs frame"
  assert L.sgw_scalarise(e._h, R_ + 8, R_, F_, 1, None, O_, None, None, s) == ERR_ARG, "rows move as 16-byte accesses"
  torch.cuda.synchronize()
  assert (o == SENTINEL).all(), "a refused call writes nothing"
  assert L.sgw_scalarise(e._h, R_, R_, F_, 1, _karr([K, 0]), O_, None, None, s) == 0     # and the engine still works


# ---- 2. the reference's runs through the L4 facade ------------------------------------------------------------------------
def _nan_equal_bits(got, want):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  nan = np.isnan(want)
  return got.shape == want.shape and bool((np.isnan(got) == nan).all()) and R.same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want))


@pytest.mark.parametrize("scalarise", [True, False])
@pytest.mark.parametrize("name", R.CONFIGS)
def test_fixture_replay_through_the_l4_facade(name, scalarise):
  z = R.load(name)
  env_name, kw = R.ENVS[name]
  env = BatchedSafetyEnvironment(env_name, num_envs=1, device=DEV, scalarise=scalarise, **kw)
  try:
    K = z["reward"].shape[1]
    rows = []

    def record(ts):
      o = ts.observation
      lp, op = env.get_last_performance(), env.get_overall_performance()
      shape = (1,) if scalarise else (1, K)
      lp = torch.full(shape, float("nan"), dtype=torch.float64, device=DEV) if lp is None else lp
      op = torch.full(shape, float("nan"), dtype=torch.float64, device=DEV) if op is None else op
      keep = [ts.reward, o["reward"], o["cumulative"], o["frame"].to(torch.float64), ts.step_type.to(torch.float64), lp, op]
      if scalarise:
        keep += [o["scalar_reward"], o["scalar_cumulative"], o["scalar_average"]]
      else:
        assert "scalar_reward" not in o and "scalar_average" not in o
      rows.append(torch.cat([t.reshape(-1).clone() for t in keep]))

    record(env.reset())
    for t, a in enumerate(z["actions"]):
      if t == int(z["reset_at"]):
        record(env.reset())
      record(env.step(torch.tensor([int(a)], dtype=torch.int8, device=DEV)))
    got = torch.stack(rows).cpu().numpy()
    S = z["frame"].shape[0]
    assert got.shape[0] == S
    c = 0

    def take(w):
      nonlocal c
      c += w
      return got[:, c - w:c]

    reward = take(1 if scalarise else K)
    vec_reward, vec_cum, frame, step_type = take(K), take(K), take(1)[:, 0], take(1)[:, 0]
    lp, op = take(1 if scalarise else K), take(1 if scalarise else K)
    assert (frame == z["frame"]).all() and (step_type == z["step_type"]).all()
    assert R.same_bits(vec_reward, z["reward"]) and R.same_bits(vec_cum, z["cumulative_reward"]), "the vectors are what they were"
    if scalarise:
      assert R.same_bits(reward[:, 0], z["scalar_reward"]), "TimeStep.reward is the reference's scalar reward"
      assert R.same_bits(take(1)[:, 0], z["scalar_reward"])
      assert R.same_bits(take(1)[:, 0], z["scalar_cumulative_reward"])
      assert R.same_bits(take(1)[:, 0], z["scalar_average_reward"])
      assert _nan_equal_bits(lp[:, 0], z["scalar_last_performance"])
      assert _nan_equal_bits(op[:, 0], z["scalar_overall_performance"])
    else:
      assert R.same_bits(reward, z["reward"])
      assert _nan_equal_bits(lp, z["last_performance"])
      assert _nan_equal_bits(op, z["overall_performance"])
  finally:
    env.close()


@pytest.mark.parametrize("name", R.MA_CONFIGS)
def test_two_agent_fixture_replay_through_the_l4_facade(name):
  """firemaker_ex_ma (a worker with 2 dimensions, an absent column, a supervisor with 3) and aintelope_savanna (two agents with 11
  each) from the generator state of the reference run: per agent the scalar reward, cumulative reward, average reward and overall
  performance of the reference's scalarise=True run; the vectors beside them are those of its scalarise=False run."""
  z = R.load(name)
  env_name, kw = R.ma_env(z)
  slots, ks = z["meta_slots"].tolist(), z["k_agent"].tolist()
  env = BatchedSafetyEnvironment(env_name, num_envs=1, device=DEV, scalarise=True, **kw)
  try:
    A, K = env.spec.A, env.spec.K
    assert env.engine._agent_ks() == ks and z["reward"].shape[1:] == (A, K)
    env.engine.set_rng_state(z["rng_state"].reshape(1, 4))
    for _ in range(int(z["constructor_resets"])):
      env.reset()
    rows = []

    def record(ts):
      o = ts.observation
      keep = [ts.reward, o["scalar_cumulative"], o["scalar_average"], env.get_overall_performance(), env.get_last_performance(),
              o["reward"], o["cumulative"], o["frame"].to(torch.float64), o["step_type"].to(torch.float64)]
      rows.append(torch.cat([t.reshape(-1).clone() for t in keep]))

    record(env.reset())
    for t, a in enumerate(z["actions"]):
      if t == int(z["reset_at"]):
        record(env.reset())
      acts = [int(a[q]) if q in slots else 0 for q in range(A)]        # an absent agent's column carries 0, as the Zoo facade sends it
      record(env.step(torch.tensor(acts, dtype=torch.int8, device=DEV)))
    got = torch.stack(rows).cpu().numpy()
    S = z["frame"].shape[0]
    c = 0

    def take(*shape):
      nonlocal c
      w = int(np.prod(shape))
      c += w
      return got[:, c - w:c].reshape((S,) + shape)

    reward, cum, avg, overall, last = take(A), take(A), take(A), take(A), take(A)
    vec_reward, vec_cum, frame, step_type = take(A, K), take(A, K), take(1)[:, 0], take(A)
    assert (frame == z["frame"]).all() and (step_type[:, slots] == z["step_type"][:, slots]).all()
    for q in range(A):
      if q not in slots:                                     # an agent that does not exist has no dimensions: every sum is 0.0
        assert ks[q] == 0 and not reward[:, q].any() and not cum[:, q].any() and not avg[:, q].any()
        continue
      k = ks[q]
      assert R.same_bits(vec_reward[:, q, :k], z["reward"][:, q, :k]) and R.same_bits(vec_cum[:, q, :k], z["cumulative_reward"][:, q, :k])
      assert R.same_bits(reward[:, q], z["scalar_reward"][:, q]), "TimeStep.reward of agent column %d" % q
      assert R.same_bits(cum[:, q], z["scalar_cumulative_reward"][:, q])
      assert R.same_bits(avg[:, q], z["scalar_average_reward"][:, q])
      assert _nan_equal_bits(overall[:, q], z["scalar_overall_performance"][:, q])
      # the reference's MoMa get_last_performance raises under scalarise; here: the sum of the last finished episode's return
      ended = np.nonzero((z["step_type"][:, slots] == 2).all(axis=1))[0]
      for i, row in enumerate(ended):
        upto = ended[i + 1] if i + 1 < len(ended) else S
        assert (last[row:upto, q] == R.loop_sum(z["cumulative_reward"][row, q, :k])).all()
      assert np.isnan(last[:ended[0], q]).all()
  finally:
    env.close()


# ---- 3. 130 envs, every way to ask ---------------------------------------------------------------------------------------------
N_ENVS, T_RUN = 130, 40


def _loops(reward, cum, frame):
  """[T, N, K], [T, N, K], [T, N] -> the three scalar arrays [T, N]."""
  return R.loop_sums(reward), R.loop_sums(cum), R.loop_averages(cum, frame)


@pytest.fixture(scope="module")
def island_run():
  """The 130-env run through step(): per step the vectors and the scalars the facade returned, and the action tape."""
  env = BatchedSafetyEnvironment("island_navigation_ex", num_envs=N_ENVS, device=DEV, level=9, scalarise=True)
  try:
    acts = env.engine.fill_actions(T_RUN, 0x5CA1).clone()
    env.reset()
    keep = {k: [] for k in ("reward", "cumulative", "frame", "scalar_reward", "scalar_cumulative", "scalar_average", "ts_reward")}
    for t in range(T_RUN):
      ts = env.step(acts[t])
      for k in keep:
        keep[k].append((ts.reward if k == "ts_reward" else ts.observation[k]).clone())
    out = {k: torch.stack(v).cpu().numpy() for k, v in keep.items()}
    out["actions"] = acts
    out["loops"] = _loops(out["reward"], out["cumulative"], out["frame"])
    return out
  finally:
    env.close()


def test_130_envs_through_step(island_run):
  r = island_run
  assert r["scalar_reward"].shape == (T_RUN, N_ENVS) and r["scalar_reward"].dtype == np.float64
  assert (r["frame"] > 0).any() and (np.abs(r["reward"]).sum(axis=2) > 0).any()
  for got, want in zip((r["scalar_reward"], r["scalar_cumulative"], r["scalar_average"]), r["loops"]):
    assert R.same_bits(got, want)
  assert R.same_bits(r["ts_reward"], r["loops"][0])
  naive = r["loops"][1] / (r["frame"] + 1.0)
  assert (naive != r["scalar_average"]).any(), "the run tells the sum of the quotients from the quotient of the sum"


def test_130_envs_through_step_n_and_scalarise_T(island_run):
  e = BatchedEngine(make_spec("island_navigation_ex", level=9), N_ENVS, device=DEV, outputs=("reward", "cumulative", "frame", "step_type"))
  try:
    e.reset()
    o = e.step_n(island_run["actions"], write_every=True)
    s = e.scalarise(T=T_RUN)
    assert s["scalar_reward"].shape == (T_RUN, N_ENVS)
    got = {k: v.cpu().numpy() for k, v in s.items()}
    vec = {k: o[k].cpu().numpy() for k in ("reward", "cumulative", "frame")}
    want = _loops(vec["reward"], vec["cumulative"], vec["frame"])
    for k, w in zip(("scalar_reward", "scalar_cumulative", "scalar_average"), want):
      assert R.same_bits(got[k], w), k
      assert R.same_bits(got[k], island_run[k]), "the same tape from the same start: what step() gave"
    ptrs = {k: v.data_ptr() for k, v in s.items()}
    s2 = e.scalarise(T=T_RUN, buffers={k: o[k] for k in ("reward", "cumulative", "frame")})      # the views a write_every call returned
    assert {k: v.data_ptr() for k, v in s2.items()} == ptrs, "result tensors are allocated once per shape and reused"
    for k in got:
      assert R.same_bits(s2[k].cpu().numpy(), got[k])
    with pytest.raises(N.SgwError):
      e.scalarise(T=1)                         # the engine holds [T, N_pad] buffers now
  finally:
    e.close()


def test_scalarise_under_graph_capture():
  """A plain launch on the caller's stream: a step and the sums after it, captured by torch.cuda.graph on a side stream after a
  warm-up outside the capture, replayed three times over an action buffer refilled in place."""
  e = BatchedEngine(make_spec("island_navigation_ex", level=9), N_ENVS, device=DEV, outputs=("reward", "cumulative", "frame", "step_type"))
  try:
    acts = e.fill_actions(8, 77).clone()
    abuf = acts[0].clone()
    e.reset()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      for t in range(1, 4):                    # warm-up outside the capture (and a few steps in, so that the sums are not all zero)
        abuf.copy_(acts[t])
        e.step(abuf)
        s = e.scalarise()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      e.step(abuf)
      s2 = e.scalarise()
    assert all(s2[k].data_ptr() == s[k].data_ptr() for k in s)
    for rep in range(3):
      abuf.copy_(acts[4 + rep])
      graph.replay()
      torch.cuda.synchronize()
      vec = {k: e._bufs[k][:N_ENVS].cpu().numpy() for k in ("reward", "cumulative", "frame")}
      want = _loops(vec["reward"], vec["cumulative"], vec["frame"])
      assert (vec["frame"] == 4 + rep).any(), "the replay stepped (three warm-up steps, then one per replay)"
      for k, w in zip(("scalar_reward", "scalar_cumulative", "scalar_average"), want):
        assert R.same_bits(s[k].cpu().numpy(), w), (rep, k)
  finally:
    e.close()


# ---- 4. the L5 facades ---------------------------------------------------------------------------------------------------------
def test_gym_env_returns_float64_scalars():
  z = R.load("island_L9")
  env = GridworldGymEnv("island_navigation_ex", level=9, scalarise=True)
  l4 = BatchedSafetyEnvironment("island_navigation_ex", num_envs=1, device=DEV, level=9, scalarise=True)
  try:
    _, info = env.reset()
    l4.reset()
    assert type(info["cumulative_reward"]) is np.float64 and type(info["average_reward"]) is np.float64
    for t, a in enumerate(z["actions"][:int(z["reset_at"])]):
      _, reward, done, truncated, info = env.step(int(a))
      ts = l4.step(torch.tensor([int(a)], dtype=torch.int8, device=DEV))
      i = t + 1
      if z["reward_none"][i]:
        assert reward == 0.0                    # an auto-reset step: as for the vectors
      else:
        assert type(reward) is np.float64
      assert reward == z["scalar_reward"][i] == ts.reward.item()
      assert info["observed_reward"] == reward
      for key, col, obs in (("cumulative_reward", "scalar_cumulative_reward", "scalar_cumulative"),
                            ("average_reward", "scalar_average_reward", "scalar_average")):
        assert type(info[key]) is np.float64 and info[key].shape == ()
        assert info[key] == z[col][i] == ts.observation[obs].item(), key
      assert done == (z["step_type"][i] == 2) and truncated is False
      assert len(info["cumulative_reward_dict"]) == 10, "the dicts keep their dimensions"
  finally:
    env.close(); l4.close()


@pytest.mark.parametrize("full_info", [False, True])
def test_vector_env_returns_n_tensors(full_info):
  n, T = N_ENVS, 12
  v = GridworldVectorEnv("island_navigation_ex", n, device=DEV, full_info=full_info, level=9, scalarise=True)
  l4 = BatchedSafetyEnvironment("island_navigation_ex", num_envs=n, device=DEV, level=9, scalarise=True)
  try:
    acts = l4.engine.fill_actions(T, 0xBEEF).clone()
    v.reset(); l4.reset()
    for t in range(T):
      _, reward, done, _, info = v.step(acts[t])
      ts = l4.step(acts[t])
      assert reward.shape == (n,) and reward.dtype == torch.float64 and reward.is_cuda
      assert torch.equal(reward, ts.reward)
      for key, obs in (("cumulative_reward", "scalar_cumulative"), ("average_reward", "scalar_average")):
        assert info[key].shape == (n,) and info[key].dtype == torch.float64
        assert torch.equal(info[key], ts.observation[obs]), key
      assert info["cumulative"].shape == (n, 10), "the raw output keeps its K axis"
    assert (ts.observation["scalar_cumulative"] != 0).any()
  finally:
    v.close(); l4.close()


def test_zoo_vector_env_returns_n_tensors_per_agent():
  n, T, seed = 65, 12, 3
  kw = dict(amount_agents=2, max_iterations=8)
  v = GridworldZooVectorEnv("aintelope_savanna", n, device=DEV, seed=seed, scalarise=True, **kw)
  twin = GridworldZooVectorEnv("aintelope_savanna", n, device=DEV, seed=seed, **kw)
  l4 = BatchedSafetyEnvironment("aintelope_savanna", num_envs=n, device=DEV, scalarise=True, **kw)
  try:
    l4.engine.seed_rng(base=seed)
    acts = l4.engine.fill_actions(T, 0xF00D).clone()            # int8 [T, N, A] in the library's column order
    v.reset(); twin.reset(); l4.reset()
    slots = list(getattr(v.spec_, "agent_slots", range(len(v.possible_agents))))
    seen = 0.0
    for t in range(T):
      _, rewards, terms, _, infos = v.step(acts[t])
      _, vec_rewards, vec_terms, _, vec_infos = twin.step(acts[t])
      ts = l4.step(acts[t])
      for i, a in enumerate(v.possible_agents):
        q = slots[i]
        r = rewards[a]
        assert r.shape == (n,) and r.dtype == torch.float64 and r.is_cuda
        assert torch.equal(r, ts.reward[:, q]), "the L4 facade's value"
        assert R.same_bits(r.cpu().numpy(), R.loop_sums(vec_rewards[a].cpu().numpy()))
        c = infos[a]["cumulative_reward"]
        assert c.shape == (n,) and torch.equal(c, ts.observation["scalar_cumulative"][:, q])
        assert R.same_bits(c.cpu().numpy(), R.loop_sums(vec_infos[a]["cumulative_reward"].cpu().numpy()))
        assert torch.equal(infos[a]["average_reward"], ts.observation["scalar_average"][:, q])
        assert torch.equal(terms[a], vec_terms[a]), "dead agents and auto-resets are handled as for the vectors"
        seen += float(c.abs().sum().item())
    assert seen > 0
  finally:
    v.close(); twin.close(); l4.close()


def test_zoo_parallel_and_aec_envs_return_float64_scalars():
  """The PettingZoo forms (what the reference's Zoo API tests construct with "scalarise": True): per agent an np.float64 reward,
  0.0 on an auto-reset round and nothing for a dead agent exactly as for the vectors; the info dicts' cumulative_reward /
  average_reward are np.float64 per agent character."""
  kw = dict(amount_agents=2, max_iterations=6)
  env = GridworldZooParallelEnv("aintelope_savanna", seed=11, scalarise=True, **kw)
  twin = GridworldZooParallelEnv("aintelope_savanna", seed=11, **kw)
  try:
    env.reset(); twin.reset()
    rng = np.random.default_rng(4)
    seen = 0
    for t in range(16):
      assert env.agents == twin.agents
      if not env.agents:                                       # every agent is done: the caller starts the next episode
        env.reset(); twin.reset()
      acts = {a: int(rng.integers(0, 5)) for a in env.agents}
      _, rewards, terms, _, infos = env.step(dict(acts))
      _, vec_rewards, vec_terms, _, vec_infos = twin.step(dict(acts))
      assert set(rewards) == set(vec_rewards) and terms == vec_terms
      for a, r in rewards.items():
        v = vec_rewards[a]
        if isinstance(v, float):                               # an auto-reset round: 0.0 in both forms
          assert r == 0.0 and v == 0.0
        else:
          assert type(r) is np.float64 and r == R.loop_sum(v)
          seen += int(r != 0)
        assert infos[a]["observed_reward"] == r
        for key in ("cumulative_reward", "average_reward"):
          for ch, x in infos[a][key].items():
            assert type(x) is np.float64 and x.shape == ()
            assert x == R.loop_sum(vec_infos[a][key][ch]), key
        assert infos[a]["reward_dict"] == vec_infos[a]["reward_dict"], "the dicts keep their dimensions"
    assert seen > 0
  finally:
    env.close(); twin.close()
  aec = GridworldZooAecEnv("aintelope_savanna", seed=11, scalarise=True, **kw)
  try:
    aec.reset()
    for i, agent in enumerate(aec.agent_iter(12)):
      _, reward, terminated, truncated, _ = aec.last()
      assert isinstance(reward, float), "np.float64 is a float: the accumulated scalar reward since the agent's last step"
      assert np.ndim(reward) == 0
      aec.step(None if terminated or truncated else (i % 5))
  finally:
    aec.close()
