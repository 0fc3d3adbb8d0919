"""GPU tier of sgw_simulate_moves / sgw_fold_q_values: the kernels against the reference's own runs (tests/golden/qvalues_*: the
targets, the tiles, the table and the step log, byte for byte) and against tests/whatif_ref.py on random steps of every covered
family, at env counts around the 64-env workgroup, with D = 1 and D = K; untouched bytes past N, the action mask against
lookahead, persistence across a masked reset, one graph capture, and the vector envs' infos."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import philox, step_log as SL
from ai_safety_gridworlds_amd.engine import BatchedEngine, GENERATOR_FAMILIES
from ai_safety_gridworlds_amd.environments import BatchedSafetyEnvironment
from ai_safety_gridworlds_amd.specs import make_spec
from tests import whatif_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTS = ("board", "agent_pos", "agent_flags", "reward", "cumulative", "step_type", "term_reason", "frame", "metrics")

# id -> (env, kwargs): the three fixture envs, turning actions away from UP, other agents as blockers with fire under an agent, two agents
FAMILIES = {
    "island_l9": ("island_navigation_ex", dict(level=9, max_iterations=20)),
    "boat_l3": ("boat_race_ex", dict(level=3, max_iterations=20)),
    "conveyor_ex": ("conveyor_belt_ex", dict(noops=True, max_iterations=20)),
    "island_ma_turning": ("island_navigation_ex_ma", dict(action_direction_mode=2, observation_direction_mode=2, max_iterations=20)),
    "firemaker_3": ("firemaker_ex_ma", dict(amount_agents=3, max_iterations=20)),
    "savanna_2": ("aintelope_savanna", dict(amount_agents=2, max_iterations=20)),
}


def relative_of(spec):
  return bool((getattr(spec, "config", None) or {}).get("action_direction_mode", 0))


def make_engine(env, kw, n, outputs=OUTS):
  spec = make_spec(env, **kw)
  eng = BatchedEngine(spec, n, device=DEV, outputs=outputs)
  if spec.family in GENERATOR_FAMILIES:
    eng.seed_rng(base=11)
  return eng


def host(o, spec, *names):
  n = o["board"].shape[0]
  shapes = {"board": (n, spec.H, spec.W), "agent_pos": (n, spec.A, 2), "agent_flags": (n, spec.A)}
  return [o[k].cpu().numpy().reshape(shapes[k]) for k in names]


def expect(eng, o):
  board, pos, flags = host(o, eng.spec, "board", "agent_pos", "agent_flags")
  return R.simulate(board, pos, flags, relative_of(eng.spec), eng.spec.impassable, eng.spec.n_actions)


def random_actions(spec, n, T, seed):
  return np.stack([philox.actions(seed, np.arange(n), np.arange(T), spec.action_lo, spec.n_actions, agent=a) for a in range(spec.A)], axis=-1)


# ---- the reference's runs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixture_replay_targets_tiles_table_and_log(name, tmp_path):
  fx, meta, rows = R.load_fixture(name)
  env = BatchedSafetyEnvironment(meta["env"], num_envs=3, device=DEV, **meta["kwargs"])
  log = SL.StepLogger(env, [SL.LOG_EPISODE, SL.LOG_ITERATION, SL.LOG_QVALUES_PER_TILETYPE], log_dir=str(tmp_path), log_filename="log.csv",
                      env_indices=[1])
  assert env.engine.default_tile_chars() == meta["tile_types"] + [meta["agent_chr"]]
  ts = env.reset(); log.on_reset(); log.write(ts)
  ts = env.reset(); log.on_reset(); log.write(ts)
  q = torch.from_numpy(fx["q"]).to(DEV)
  for t in range(len(fx["actions"])):
    if fx["reset_before"][t]:
      ts = env.reset(); log.on_reset(); log.write(ts)
    board, pos = host(ts.observation, env.spec, "board", "agent_pos")
    assert np.array_equal(board[1], fx["board"][t]) and np.array_equal(pos[1, 0], fx["agent_pos"][t]), "the env left the reference's run at step %d" % t
    ts = env.step(torch.full((3,), int(fx["actions"][t]), dtype=torch.int8), q_value_per_action=q[t].expand(3, 1, -1, -1).contiguous())
    log.write(ts)
    sim = env.engine._whatif_out
    assert np.array_equal(sim["target_pos"][1, 0].cpu().numpy(), fx["target_pos"][t]), t
    assert np.array_equal(sim["target_tile"][1, 0].cpu().numpy(), fx["target_tile"][t]), t
    assert np.array_equal(R.bits(env.q_value_per_tiletype[1, 0].cpu().numpy()), R.bits(fx["table"][t])), t
    assert np.array_equal(env.engine.q_value_seen[1, 0].cpu().numpy(), fx["seen"][t]), t
  log.close()
  want = open(R.__file__.replace("whatif_ref.py", "golden/%s.csv" % name), newline="").read()
  got = open(log.path, newline="").read()
  assert got.splitlines()[0] == want.splitlines()[0]
  assert len(got.splitlines()) == len(want.splitlines())
  for ln, (g, w) in enumerate(zip(got.splitlines(), want.splitlines())):
    assert g == w, "line %d" % ln
  env.close()


# ---- every family against the restatement --------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(FAMILIES))
def rollout(request):
  """One 130-env engine per family (two workgroups, the second ragged), 20 random steps; per step the kernels' outputs and the
  restatement's, computed once and shared by the tests below."""
  env, kw = FAMILIES[request.param]
  n, T = 130, 20
  eng = make_engine(env, kw, n)
  sp = eng.spec
  K = sp.K
  acts = torch.from_numpy(random_actions(sp, n, T, 5).astype(np.int8)).to(DEV)
  rng = np.random.default_rng(17)
  qs = rng.standard_normal((T, n, sp.A, sp.n_actions, K)) * 10.0 ** rng.integers(-3, 7, size=(T, n, sp.A, sp.n_actions, K))
  chars = [ord(c) for c in eng.default_tile_chars()]
  table, seen = np.zeros((n, sp.A, len(chars), K)), np.zeros((n, sp.A, len(chars)), np.uint8)
  steps, o = [], eng.reset()
  for t in range(T):
    want = expect(eng, o)
    got = {k: v.cpu().numpy() for k, v in eng.simulate_moves().items()}
    dev_table = eng.fold_q_values(torch.from_numpy(qs[t]).to(DEV)).cpu().numpy()
    R.fold(want[1], qs[t], chars, table, seen)
    steps.append(dict(want=want, got=got, table=dev_table, seen=eng.q_value_seen.cpu().numpy(), want_table=table.copy(), want_seen=seen.copy(),
                      inputs=host(o, sp, "board", "agent_pos", "agent_flags")))
    o = eng.step(acts[t] if sp.A > 1 else acts[t].reshape(-1))
  yield dict(name=request.param, eng=eng, steps=steps, qs=qs, chars=chars)
  eng.close()


def test_targets_tiles_and_mask_equal_the_restatement(rollout):
  for t, s in enumerate(rollout["steps"]):
    for name, w in zip(("target_pos", "target_tile", "blocked"), s["want"]):
      assert np.array_equal(s["got"][name], w), "%s at step %d" % (name, t)


def test_the_table_equals_the_restatement_bit_for_bit(rollout):
  for t, s in enumerate(rollout["steps"]):
    assert np.array_equal(s["seen"], s["want_seen"]), t
    assert np.array_equal(R.bits(s["table"]), R.bits(s["want_table"])), t
  last = rollout["steps"][-1]
  assert last["want_seen"].any() and not last["want_seen"].all(), "some tile types were reached and some never were"


def test_the_rollout_exercises_what_the_family_is_here_for(rollout):
  name, sp, steps = rollout["name"], rollout["eng"].spec, rollout["steps"]
  blocked = np.stack([s["want"][2] for s in steps]).astype(bool)
  pos = np.stack([s["want"][0] for s in steps])
  own = np.stack([s["inputs"][1] for s in steps])
  stale = blocked & (pos != own[:, :, :, None, :]).any(axis=-1)
  assert stale.any(), "no refused action reported another cell than the agent's"
  flags = np.stack([s["inputs"][2] for s in steps])
  if name == "island_ma_turning":
    assert sp.n_actions == 9 and (((flags >> 1) & 3) != R.UP).any(), "no action direction left UP"
    assert not blocked[..., 5:].any() and blocked[..., 1:5].any()
  if name == "firemaker_3":
    assert sp.A == 3 and sp.impassable == ["#2S", "#1S", "#12"] and (flags & 1).any(), "no agent stood on hidden fire"
    tiles = np.stack([s["inputs"][0] for s in steps])
    hit_agent = False
    for t, n, a, j in np.argwhere(blocked):
      r, c = own[t, n, a]
      dr, dc = R.MOTION[j]
      if 0 <= r + dr < sp.H and 0 <= c + dc < sp.W and chr(tiles[t, n, r + dr, c + dc]) in "12S":
        hit_agent = True
        break
    assert hit_agent, "no move was refused by another agent"
  if name == "savanna_2":
    assert sp.A == 2 and sp.impassable == ["#1", "#0"]


# ---- env counts, D, bytes past N -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 130])
@pytest.mark.parametrize("D", [1, "K"])
def test_env_counts_dimensions_and_untouched_bytes(n, D):
  eng = make_engine("island_navigation_ex_ma", dict(max_iterations=20), n)
  sp = eng.spec
  D = sp.K if D == "K" else 1
  acts = torch.from_numpy(random_actions(sp, n, 6, 3).astype(np.int8)).to(DEV)
  o = eng.reset()
  for t in range(6):
    o = eng.step(acts[t])
  want_pos, want_tile, want_blocked = expect(eng, o)
  NA, A, L, pad = sp.n_actions, sp.A, 5, 3
  chars = torch.tensor([ord(c) for c in " WD1Z"], dtype=torch.uint8, device=DEV)        # 'Z' is on no board: its rows stay
  bufs = {k: torch.full(((n + pad) * A * NA * w,), 0xAB, dtype=torch.uint8, device=DEV) for k, w in (("pos", 2), ("tile", 1), ("blk", 1))}
  rng = np.random.default_rng(n)
  q = rng.standard_normal((n + pad, A, NA, D))
  table0 = rng.standard_normal((n + pad, A, L, D))
  q_dev, table = torch.from_numpy(q).to(DEV), torch.from_numpy(table0).to(DEV)
  seen = torch.full(((n + pad) * A * L,), 0xCD, dtype=torch.uint8, device=DEV)
  L_ = eng._lib
  assert L_.sgw_simulate_moves(eng._h, eng._bufs["board"].data_ptr(), eng._bufs["agent_pos"].data_ptr(), eng._bufs["agent_flags"].data_ptr(),
                               bufs["pos"].data_ptr(), bufs["tile"].data_ptr(), bufs["blk"].data_ptr(), eng._stream()) == 0
  assert L_.sgw_fold_q_values(eng._h, bufs["tile"].data_ptr(), q_dev.data_ptr(), D, chars.data_ptr(), L, table.data_ptr(), seen.data_ptr(),
                              eng._stream()) == 0
  got = {k: v.cpu().numpy() for k, v in bufs.items()}
  assert np.array_equal(got["pos"][:n * A * NA * 2].reshape(n, A, NA, 2), want_pos)
  assert np.array_equal(got["tile"][:n * A * NA].reshape(n, A, NA), want_tile)
  assert np.array_equal(got["blk"][:n * A * NA].reshape(n, A, NA), want_blocked)
  for k, w in (("pos", 2), ("tile", 1), ("blk", 1)):
    assert (got[k][n * A * NA * w:] == 0xAB).all(), "%s: bytes past N were written" % k
  want_table, want_seen = table0[:n].copy(), np.full((n, A, L), 0xCD, np.uint8)
  R.fold(want_tile, q[:n], [int(c) for c in chars.cpu().numpy()], want_table, want_seen)
  got_table, got_seen = table.cpu().numpy(), seen.cpu().numpy()
  assert np.array_equal(R.bits(got_table[:n]), R.bits(want_table)) and np.array_equal(R.bits(got_table[n:]), R.bits(table0[n:]))
  assert np.array_equal(got_seen[:n * A * L].reshape(n, A, L), want_seen) and (got_seen[n * A * L:] == 0xCD).all()
  assert (want_seen[:, :, 4] == 0xCD).all() and (want_seen[:, :, 0] == 1).any()
  # the padding rows of the engine's own buffers (n_pad > n) are not read either: poisoning them changes nothing
  if eng.n_pad > n:
    eng._bufs["board"][n:].fill_(ord('#')); eng._bufs["agent_pos"][n:].fill_(255)
    again = eng.simulate_moves()
    assert np.array_equal(again["target_pos"].cpu().numpy(), want_pos) and np.array_equal(again["blocked"].cpu().numpy(), want_blocked)
  eng.close()


# ---- the mask against playing the moves ----------------------------------------------------------------------------------------
def test_blocked_agrees_with_lookahead():
  eng = make_engine("island_navigation_ex", dict(level=9, max_iterations=50), 130)
  acts = torch.from_numpy(random_actions(eng.spec, 130, 8, 9)[..., 0].astype(np.int8)).to(DEV)
  o = eng.reset()
  checked = 0
  for t in range(8):
    o = eng.step(acts[t])
    pos0 = o["agent_pos"].clone()
    alive = (o["step_type"].reshape(130) != 2)                     # a LAST env would reset instead of moving
    blocked = eng.simulate_moves()["blocked"][:, 0].clone()
    cand = torch.arange(5, dtype=torch.int8, device=DEV)[:, None].expand(5, 130).contiguous()
    look = eng.lookahead(cand)
    for j in range(1, 5):
      stayed = (look["agent_pos"][j].reshape(130, 2) == pos0.reshape(130, 2)).all(dim=1)
      assert bool((stayed[alive] == blocked[alive, j].bool()).all()), "action %d at step %d" % (j, t)
      checked += int(alive.sum())
    assert not bool(blocked[:, 0].any())
  assert checked > 2000
  eng.close()


def test_the_table_persists_across_a_masked_reset():
  eng = make_engine("island_navigation_ex", dict(level=9), 65)
  sp = eng.spec
  eng.reset()
  rng = np.random.default_rng(2)
  q = torch.from_numpy(rng.standard_normal((65, 1, sp.n_actions, sp.K))).to(DEV)
  for a in (2, 2, 4):
    eng.step(torch.full((65,), a, dtype=torch.int8, device=DEV))
    eng.simulate_moves(); eng.fold_q_values(q)
  before, seen_before = eng.q_value_per_tiletype.clone(), eng.q_value_seen.clone()
  mask = torch.zeros(65, dtype=torch.uint8, device=DEV); mask[::2] = 1
  eng.reset(mask)
  assert torch.equal(eng.q_value_per_tiletype, before) and torch.equal(eng.q_value_seen, seen_before), "a reset touches no table"
  eng.simulate_moves(); table = eng.fold_q_values(q * 2.0)
  L = eng.q_value_tile_chars.index('A')
  assert torch.equal(table[:, 0, L], (q * 2.0)[:, 0, 0]), "NOOP alone lands on the agent's own character"
  untouched = (eng.q_value_seen == 1) & ~torch.from_numpy(
      np.array([[[ord(c) in row for c in eng.q_value_tile_chars] for row in env] for env in eng._whatif_out["target_tile"].cpu().numpy()])).to(DEV)
  assert bool(untouched.any()) and torch.equal(table[untouched], before[untouched]), "tile types not reached now keep their values"
  eng.close()


def test_float32_q_values_are_widened_then_averaged_in_float64():
  eng = make_engine("boat_race_ex", dict(level=3), 63)
  eng.reset()
  q32 = torch.from_numpy(np.random.default_rng(4).standard_normal((63, eng.spec.n_actions, 2)).astype(np.float32)).to(DEV)
  eng.simulate_moves()
  got = eng.fold_q_values(q32).clone()
  eng.__dict__.pop("_fold_key")
  assert torch.equal(got, eng.fold_q_values(q32.double().reshape(63, 1, -1, 2)))
  eng.close()


def test_graph_capture_of_simulate_and_fold_replays_to_the_same_bytes():
  eng = make_engine("firemaker_ex_ma", dict(amount_agents=3, max_iterations=20), 130)
  sp = eng.spec
  acts = torch.from_numpy(random_actions(sp, 130, 4, 6).astype(np.int8)).to(DEV)
  q_host = np.random.default_rng(8).standard_normal((130, sp.A, sp.n_actions, sp.K))
  q = torch.from_numpy(q_host).to(DEV)
  chars = [ord(c) for c in eng.default_tile_chars()]
  table, seen = np.zeros((130, sp.A, len(chars), sp.K)), np.zeros((130, sp.A, len(chars)), np.uint8)
  o = eng.reset()
  eng.simulate_moves(); eng.fold_q_values(q)                       # allocates the persistent tensors outside the capture
  R.fold(expect(eng, o)[1], q_host, chars, table, seen)
  torch.cuda.synchronize()
  stream = torch.cuda.Stream()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.stream(stream):
    with torch.cuda.graph(graph, stream=stream):                   # (launches are recorded, not run: the table is not folded here)
      eng.simulate_moves(); eng.fold_q_values(q)
  for t in range(4):
    o = eng.step(acts[t])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = expect(eng, o)
    for name, w in zip(("target_pos", "target_tile", "blocked"), want):
      assert np.array_equal(eng._whatif_out[name].cpu().numpy(), w), "%s at replay %d" % (name, t)
    R.fold(want[1], q_host, chars, table, seen)
    assert np.array_equal(R.bits(eng.q_value_per_tiletype.cpu().numpy()), R.bits(table)), t
    assert np.array_equal(eng.q_value_seen.cpu().numpy(), seen), t
  eng.close()


# ---- the vector envs -----------------------------------------------------------------------------------------------------------
def test_vector_env_infos_equal_the_engine_call():
  from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldVectorEnv
  env = GridworldVectorEnv("island_navigation_ex", 65, device=DEV, action_targets=True, level=9)
  _, info = env.reset()
  sp, eng = env.spec_, env._env.engine
  want = expect(eng, eng._views())
  assert np.array_equal(info["action_blocked"].cpu().numpy(), want[2][:, 0]), "reset() carries the mask of the first observation"
  acts = torch.from_numpy(random_actions(sp, 65, 5, 1)[..., 0].astype(np.int8)).to(DEV)
  q_host = np.random.default_rng(5).standard_normal((65, sp.n_actions, sp.K))
  env.set_current_q_value_per_action(torch.from_numpy(q_host).to(DEV))
  chars = [ord(c) for c in eng.default_tile_chars()]
  table, seen = np.zeros((65, 1, len(chars), sp.K)), np.zeros((65, 1, len(chars)), np.uint8)
  for t in range(5):
    before = expect(eng, eng._views())                              # the observation the step starts from: what its fold reads
    _, _, _, _, info = env.step(acts[t])
    R.fold(before[1], q_host[:, None], chars, table, seen)
    assert np.array_equal(R.bits(env.q_value_per_tiletype.cpu().numpy()), R.bits(table)), t
    blocked, tile = info["action_blocked"].clone(), info["action_target_tile"].clone()
    sim = eng.simulate_moves()                                      # the engine call on the NEW observation
    assert torch.equal(blocked, sim["blocked"][:, 0]) and torch.equal(tile, sim["target_tile"][:, 0])
    now = expect(eng, eng._views())
    assert np.array_equal(blocked.cpu().numpy(), now[2][:, 0]) and np.array_equal(tile.cpu().numpy(), now[1][:, 0])
    assert blocked.shape == (65, sp.n_actions) and blocked.device.type == "cuda"
  assert env.q_value_per_tiletype.shape == (65, 1, len(sp.tile_types) + 1, sp.K)
  plain = GridworldVectorEnv("island_navigation_ex", 65, device=DEV, level=9)
  assert "action_blocked" not in plain.reset()[1]
  env._env.close(); plain._env.close()


def test_gym_env_feeds_its_stored_q_values_to_the_next_step():
  from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldGymEnv
  env = GridworldGymEnv("island_navigation_ex", level=9)
  env.reset()
  eng, sp = env._env.engine, env.spec_
  q = np.random.default_rng(9).standard_normal((sp.n_actions, sp.K))
  env.set_current_q_value_per_action(q)
  chars = [ord(c) for c in eng.default_tile_chars()]
  table, seen = np.zeros((1, 1, len(chars), sp.K)), np.zeros((1, 1, len(chars)), np.uint8)
  for a in (2, 4, 1):
    before = expect(eng, eng._views())
    env.step(a)
    R.fold(before[1], q[None, None], chars, table, seen)
    assert np.array_equal(R.bits(env._env.q_value_per_tiletype.cpu().numpy()), R.bits(table))
  scalar_env = GridworldGymEnv("boat_race")                        # an original env: the value is kept, nothing else happens
  scalar_env.reset(); scalar_env.set_current_q_value_per_action([0.0] * 4); scalar_env.step(1)
  assert scalar_env._env.q_value_per_tiletype is None
  env.close(); scalar_env.close()


def test_zoo_vector_env_infos_and_per_agent_q_values():
  from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv
  env = GridworldZooVectorEnv("island_navigation_ex_ma", 65, device=DEV, action_targets=True)
  sp = env.spec_
  obs, infos = env.reset()
  rng = np.random.default_rng(6)
  qs = {a: torch.from_numpy(rng.standard_normal((65, sp.n_actions, sp.K))).to(DEV) for a in env.possible_agents}
  env.set_current_q_value_per_action(qs)
  eng = env._env.engine
  for t in range(4):
    want = expect(eng, eng._views())
    chars = [ord(c) for c in eng.default_tile_chars()]
    obs, _, _, _, infos = env.step({a: torch.full((65,), (t + i) % 5, dtype=torch.int8, device=DEV) for i, a in enumerate(env.possible_agents)})
    if t == 0:
      table, seen = np.zeros((65, sp.A, len(chars), sp.K)), np.zeros((65, sp.A, len(chars)), np.uint8)
    R.fold(want[1], np.stack([qs[a].cpu().numpy() for a in env.possible_agents], axis=1), chars, table, seen)
    assert np.array_equal(R.bits(env.q_value_per_tiletype.cpu().numpy()), R.bits(table)), t
    now = expect(eng, eng._views())
    for i, a in enumerate(env.possible_agents):
      assert np.array_equal(infos[a]["action_blocked"].cpu().numpy(), now[2][:, i]) and np.array_equal(infos[a]["action_target_tile"].cpu().numpy(), now[1][:, i])
  env.close()
