"""GridworldZooVectorEnv.reset(seed=, options={"env_layout_seed": ...}) against the reference run of tests/golden/
make_fixtures_reseed.py (island_navigation_ex_ma, three envs with constructor seeds 2000 + e, a segment from construction, one
after reset(options={"env_layout_seed": 2}), one after reset(env_layout_seed=3, seed=2**32 + 77 + e)): boards, rewards, step
types and termination reasons of every round; a masked reseed leaves the other envs on their streams."""
import zlib

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd.helpers.gridworld_zoo_vector_env import GridworldZooVectorEnv
from tests import golden_util as G

pytestmark = pytest.mark.gpu
NAME = "reseed_ima_L10_rand3"
M64 = (1 << 64) - 1


def numpy_words(seed):
  st = np.random.PCG64(np.random.SeedSequence(int(seed))).state["state"]
  return [st["state"] >> 64, st["state"] & M64, st["inc"] >> 64, st["inc"] & M64]


def layout_crc(original_seed, layout_seed):
  return zlib.crc32(b"".join(int(x).to_bytes(4, byteorder="big") for x in (original_seed, layout_seed, 17122023)))


def rng_words(env):
  n = env.num_envs
  return env._env.engine.get_state()[3:7, :n].cpu().numpy().view(np.uint64).T


def check(env, fx, s, t, obs, rewards, terms, infos, what):
  E = env.num_envs
  H, W = fx["board"].shape[-2:]
  for ai, a in enumerate(env.possible_agents):
    k = rewards[a].shape[1] if rewards is not None else 0
    assert np.array_equal(infos[a]["board"].cpu().numpy().reshape(E, H, W), fx["board"][:, s, t]), (what, s, t, "board")
    assert np.array_equal(infos[a]["step_type"].cpu().numpy(), fx["step_type"][:, s, t, ai]), (what, s, t, a, "step_type")
    tr = infos[a]["term_reason"].cpu().numpy().astype(np.int16)
    tr[tr == 255] = -1
    assert np.array_equal(tr, fx["term_reason"][:, s, t, ai]), (what, s, t, a, "term_reason")
    assert np.array_equal(obs[a].cpu().numpy(), fx["view"][:, s, t, ai]), (what, s, t, a, "window")
    kc = infos[a]["cumulative_reward"].shape[1]
    assert np.array_equal(infos[a]["cumulative_reward"].cpu().numpy(), fx["cumulative"][:, s, t, ai, :kc]), (what, s, t, a, "cumulative")
    if rewards is not None:
      assert k == fx["reward"].shape[-1]
      assert np.array_equal(rewards[a].cpu().numpy(), fx["reward"][:, s, t, ai, :k]), (what, s, t, a, "reward")
      assert np.array_equal(terms[a].cpu().numpy(), fx["step_type"][:, s, t, ai] >= 2), (what, s, t, a, "terminated")
  assert np.array_equal(rng_words(env), fx["rng"][:, s, t]), (what, s, t, "generator words")


@pytest.mark.parametrize("seed_form", ["int", "tensor"])
def test_vector_env_replays_the_reseeding_fixture(seed_form):
  fx, meta = G.load(NAME)
  E, T, SEG = int(meta["E"]), int(meta["T"]), int(meta["segments"])
  env = GridworldZooVectorEnv("island_navigation_ex_ma", num_envs=E, env_id_base=0, seed=2000, **meta["kwargs"])
  assert env.possible_agents == ["agent_1", "agent_2"]
  acts = torch.from_numpy(np.ascontiguousarray(fx["actions"])).to(env.device)          # [E, SEG, T, A]
  for s in range(SEG):
    if s == 0:
      obs, infos = env.reset()                                # the constructor's reset of the reference: draws the first map
      assert np.array_equal(infos["agent_1"]["board"].cpu().numpy().reshape(fx["board"].shape[0], *fx["board"].shape[-2:]), fx["board"][:, 0, 0])
      assert np.array_equal(rng_words(env), fx["rng"][:, 0, 0])
    else:
      if s == 1:
        obs, infos = env.reset(options={"env_layout_seed": 2})
      elif seed_form == "int":
        obs, infos = env.reset(seed=2**32 + 77, options={"env_layout_seed": 3})          # env e: 2**32 + 77 + its global id
      else:
        seeds = torch.tensor([2**32 + 77 + e for e in range(E)], dtype=torch.int64, device=env.device)
        obs, infos = env.reset(seed=seeds, options={"trial_no": 3})
      check(env, fx, s, 0, obs, None, None, infos, "reseeding reset")
    obs, infos = env.reset()
    check(env, fx, s, 1, obs, None, None, infos, "reset")
    for t in range(T):
      obs, rewards, terms, truncs, infos = env.step({a: acts[:, s, t, ai] for ai, a in enumerate(env.possible_agents)})
      check(env, fx, s, t + 2, obs, rewards, terms, infos, "round")
  env.close()


def test_masked_reseed_leaves_the_other_envs_on_their_streams():
  fx, meta = G.load(NAME)
  E, T = int(meta["E"]), int(meta["T"])
  acts = torch.from_numpy(np.ascontiguousarray(fx["actions"])).to("cuda:0")
  a = GridworldZooVectorEnv("island_navigation_ex_ma", num_envs=E, seed=2000, **meta["kwargs"])
  b = GridworldZooVectorEnv("island_navigation_ex_ma", num_envs=E, seed=2000, **meta["kwargs"])
  for env in (a, b):
    env.reset(); env.reset()
    for t in range(5):
      env.step({ag: acts[:, 0, t, ai] for ai, ag in enumerate(env.possible_agents)})
  mask = torch.tensor([0, 1, 0], dtype=torch.uint8, device="cuda:0")
  before = a._env.engine.get_state().clone()
  a._reseed(mask, None, 5)                                               # the reseeding half of reset(mask, options=...) by itself
  after = a._env.engine.get_state()
  others = [i for i in range(after.shape[1]) if i != 1]
  assert torch.equal(after[:, others], before[:, others]), "no word of another env (or of a padding lane) moved"
  assert np.array_equal(rng_words(a)[1], np.array(numpy_words(layout_crc(2001, 5)), dtype=np.uint64))
  _, ia = a.reset(mask, options={"env_layout_seed": 5})
  _, ib = b.reset(mask)
  wa, wb = rng_words(a), rng_words(b)
  assert np.array_equal(wa[[0, 2]], wb[[0, 2]]) and not np.array_equal(wa[1], wb[1])
  for t in range(5, T):
    step = {ag: acts[:, 0, t, ai] for ai, ag in enumerate(a.possible_agents)}
    oa, ra, ta, _, ia = a.step(step)
    ob, rb, tb, _, ib = b.step(step)
    for ag in a.possible_agents:
      for x, y in ((oa[ag], ob[ag]), (ra[ag], rb[ag]), (ta[ag], tb[ag]), (ia[ag]["board"], ib[ag]["board"])):
        assert torch.equal(x[[0, 2]], y[[0, 2]]), (t, ag)
  assert np.array_equal(rng_words(a)[[0, 2]], rng_words(b)[[0, 2]])
  with pytest.raises(OverflowError):
    a.reset(options={"env_layout_seed": 1 << 32})
  with pytest.raises(OverflowError):
    a.reset(mask, options={"trial_no": 1 << 32})
  a.close(); b.close()
