"""GridworldZooVectorEnv: N lockstep instances of a multi-agent safety gridworld behind the PettingZoo-parallel calling
convention, every array a DEVICE tensor and no host synchronisation on the step path.

    env = GridworldZooVectorEnv("firemaker_ex_ma", num_envs=16384, amount_agents=3, seed=0)
    obs, infos = env.reset()                                   # obs[agent]: uint8 [N, h_a, w_a] ascii codes (cuda)
    obs, rewards, terminateds, truncateds, infos = env.step({agent: int8 [N] cuda tensor, ...})

What one env of the batch returns is what `GridworldZooParallelEnv` (the reference's wrapper surface,
helpers/gridworld_zoo_parallel_env.py:429-615) returns for it:
  obs[agent]         the agent-centric window of the rendered board (get_agent_perspective, safety_game_moma.py:1996-2101):
                     ascii codes uint8 [N, h, w], or the value-mapped float32 board with ascii_observation_format=False
  rewards[agent]     float64 [N, K_agent] in the agent's sorted reward-dimension order (0 at an auto-reset round); with
                     scalarise=True float64 [N], the reference's left-to-right sum over those dimensions (one more library call
                     per round, sgw_scalarise), and infos[agent]["cumulative_reward"] / ["average_reward"] are [N] as well
  terminateds[agent] bool [N]: the agent's StepType is LAST or DEAD;  truncateds[agent]: all False
  infos[agent]       device tensors: "step_type" [N], "term_reason" uint8 [N] (255 until the episode is over), "cumulative_reward" [N, K_agent], "agent_position" [N, 2],
                     "discount" [N] (NaN = None), "metrics" [N, M], "board" uint8 [N, H, W] (the global board, shared),
                     "observation_direction" / "action_direction" uint8 [N] (Directions LEFT=0 RIGHT=1 UP=2 DOWN=3);
                     with layers_in_observation=True also the wrapper's layer cubes as tensors (zoo.py:296-316, 337-359):
                     "info_observation_layers_cube" uint8 [N, L, H, W] (shared) and "info_agent_observation_layers_cube"
                     uint8 [N, L, h_a, w_a], both in `layers_order` = the sorted layer characters;
                     with object_coordinates=True also the wrapper's coordinate lists as padded tensors (two more launches,
                     sgw_layer_coords / sgw_agent_layer_coords): "info_observation_coordinates" int16 [N, L, cap, 2] = (row, col)
                     of every layer's set cells in np.argwhere order with "info_observation_coordinates_count" int32 [N, L]
                     (shared), and "info_agent_observation_coordinates" int16 [N, L, cap_a, 2] = (x - ax, y - ay) inside the
                     agent's window with "info_agent_observation_coordinates_count" int32 [N, L] (-1 on every layer: the agent is
                     not in its own layers, the wrapper's []); entries past a count are not written (they keep what an earlier step left there);
                     coordinates_cap=None: H*W / the largest window's cells, which is lossless
A finished env auto-resets at its next round exactly like the reference adapter (the round's actions are discarded); agents of
the per-agent families that are already LAST/DEAD can be given -1 ("not in the dict").  One round = ONE kernel launch: the
step (shuffled sequential plays, fire spread, rewards, auto-reset) writes the agent windows too (sgw_out.views / obs_views;
families without the in-kernel windows take a second launch, sgw_agent_views).
"""
import numpy as np
import torch

from .. import _native as N
from ..engine import fused_views
from ..environments import BatchedSafetyEnvironment
from ..specs import make_spec
from .gridworld_zoo_parallel_env import INFO_AGENT_OBSERVATION_COORDINATES, INFO_OBSERVATION_COORDINATES

OUTS = ("board", "reward", "cumulative", "step_type", "term_reason", "discount", "metrics", "agent_pos", "agent_flags", "done")


class GridworldZooVectorEnv(object):
  metadata = {"name": "ai_safety_gridworlds_amd_vector"}

  def __init__(self, env_name, num_envs, ascii_observation_format=True, layers_in_observation=False, seed=None, device="cuda:0",
               env_id_base=0, object_coordinates=False, coordinates_cap=None, episode_log=None, scalarise=False, action_targets=False,
               **kwargs):
    # action_targets=True: infos[agent]["action_target_tile"] / ["action_blocked"] uint8 [N, n_actions] of the NEW observation --
    # the tile each action of the agent's next step would land on and the mask of the refused ones (BatchedEngine.simulate_moves:
    # one more launch per step for all agents, no synchronisation)
    self._targets = bool(action_targets)
    self._q = None
    self._packed_for = self._view_buf = self._cached = None      # _pack's views of the engine's outputs, built at the first step
    sp0 = make_spec(env_name, **kwargs)                        # what decides the output set, in front of the engine
    self._fused = fused_views(sp0)
    self._ascii = bool(ascii_observation_format)
    cfg0 = sp0.config
    self._turning = bool(cfg0.get("action_direction_mode", 0) or cfg0.get("observation_direction_mode", 0))
    # `terminated` and the decoded directions leave with the step launch (sgw_out.done / obs_dir / act_dir): no torch launch per step
    outs = OUTS + (("obs_dir", "act_dir") if self._turning else ()) + ((("views",) if self._ascii else ("obs_views",)) if self._fused else ())
    self._env = BatchedSafetyEnvironment(env_name, num_envs=num_envs, device=device, env_id_base=env_id_base, outputs=outs,
                                         track_performance=False, episode_log=episode_log, scalarise=scalarise, **kwargs)
    self.episode_log = self._env.episode_log                   # episode_log=cap: an EpisodeLog every step appends to (None: no log)
    sp = self.spec_ = self._env.spec
    if sp.A < 2 and not sp.per_agent:
      raise NotImplementedError("%s is a single-agent env: use GridworldVectorEnv" % env_name)
    self.num_envs = int(num_envs)
    self.device = self._env.device
    self._per_agent = sp.per_agent
    self._slots = sp.agent_slots
    self.possible_agents = ["agent_%s" % c for c in sp.agent_chars]
    self.agent_name_mapping = dict(zip(self.possible_agents, sp.agent_chars))
    self._k = {a: len(sp.agent_dim_names[c]) for a, c in self.agent_name_mapping.items()}
    self._layers = bool(layers_in_observation)
    self._coords = bool(object_coordinates)
    if self._coords:                                           # persistent (count, list) buffers, zeroed once: a launch writes the lists only
      n, L = int(num_envs), len(sp.layer_chars)
      cap = sp.H * sp.W if coordinates_cap is None else int(coordinates_cap)
      cap_a = max(h * w for (h, w) in sp.view_shapes) if coordinates_cap is None else int(coordinates_cap)
      self._coords_out = (torch.zeros((n, L), dtype=torch.int32, device=self.device),
                          torch.zeros((n, L, cap, 2), dtype=torch.int16, device=self.device))
      self._agent_coords_out = (torch.zeros((n, sp.A, L), dtype=torch.int32, device=self.device),
                                torch.zeros((n, sp.A, L, cap_a, 2), dtype=torch.int16, device=self.device))
    self.layers_order = list(sp.layer_chars)                   # get_layers_order(...) of the reference: sorted layer keys
    self._vm = torch.tensor([sp.native.value_map[i] for i in range(128)], dtype=torch.float32, device=self.device)
    self._acts = torch.zeros((self.num_envs, sp.A), dtype=torch.int8, device=self.device)
    self._never = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)            # truncated: always False
    self._up = torch.full((self.num_envs,), 2, dtype=torch.uint8, device=self.device)         # Directions.UP: the fixed-direction envs
    # the original seed of env i (environment_data[SEED] of the reference) is (seed or 0) + its global id
    self._seed_base, self._env_id_base = (0 if seed is None else int(seed)), int(env_id_base)
    self._has_rng = sp.needs_rng
    if self._has_rng:
      # env i draws from Generator(PCG64(SeedSequence(seed + global id))): what seeding.np_random gives N separately seeded envs;
      # seeded by one launch (sgw_seed_rng: the engine adds env_id_base itself)
      self._env.engine.seed_rng(base=self._seed_base)

  @property
  def agents(self):
    return list(self.possible_agents)

  def observation_shape(self, agent):
    return tuple(self.spec_.view_shapes[self._slots[self.possible_agents.index(agent)]])

  def action_range(self, agent):
    return (self.spec_.action_lo, self.spec_.action_lo + self.spec_.n_actions - 1)

  def close(self):
    self._env.close()

  def _pack(self, o):
    """A step from Python is host-bound (every torch op is a launch, every view a microsecond).  The step's outputs live in
    persistent buffers -- the `terminated` flags and the decoded directions among them (sgw_out.done / obs_dir / act_dir) -- so the
    per-agent dicts of views are built ONCE; a step then only refreshes the agent windows where the step launch does not write them
    (one launch into a reused buffer).  The returned tensors are valid until the next step / reset, like the engine's outputs."""
    sp = self.spec_
    n = self.num_envs
    eng = self._env.engine
    sc = eng.scalarise() if self._env.scalarise else None      # scalarise=True: one more library call, into persistent tensors
    if self._packed_for is not o.get("reward"):       # first call, or the engine reallocated its outputs
      self._packed_for = o.get("reward")
      if self._fused:                                              # the step launch wrote the windows (ascii or value-mapped)
        views = eng.split_views(o["views" if self._ascii else "obs_views"])
      else:
        self._view_buf = torch.empty((n, eng.view_bytes), dtype=torch.uint8, device=self.device)
        views = eng.agent_views(out=self._view_buf)
      st, tr = o["step_type"].reshape(n, -1), o["term_reason"].reshape(n, -1)
      self._done = o["done"].reshape(n, -1).view(torch.bool)
      rew = o["reward"].reshape(n, sp.A, sp.K)
      cum = o["cumulative"].reshape(n, sp.A, sp.K)
      pos = o["agent_pos"].reshape(n, sp.A, 2)
      if self._turning:
        self._odir, self._adir = o["obs_dir"].reshape(n, sp.A), o["act_dir"].reshape(n, sp.A)
      metrics = o["metrics"][:, :sp.M]
      obs, rewards, terms, truncs, infos = {}, {}, {}, {}, {}
      for i, a in enumerate(self.possible_agents):
        q, k = self._slots[i], self._k[a]
        c = q if self._per_agent else 0
        obs[a] = views[q]
        rewards[a] = rew[:, q, :k]
        terms[a] = self._done[:, c]
        truncs[a] = self._never
        infos[a] = {"step_type": st[:, c], "term_reason": tr[:, c], "cumulative_reward": cum[:, q, :k], "agent_position": pos[:, q], "discount": o["discount"],
                    "metrics": metrics, "board": o["board"],
                    "observation_direction": self._odir[:, q] if self._turning else self._up,
                    "action_direction": self._adir[:, q] if self._turning else self._up}
        if sc is not None:                                         # float64 [N] each: the sums over the agent's dimensions
          rewards[a] = sc["scalar_reward"].reshape(n, sp.A)[:, q]
          infos[a]["cumulative_reward"] = sc["scalar_cumulative"].reshape(n, sp.A)[:, q]
          infos[a]["average_reward"] = sc["scalar_average"].reshape(n, sp.A)[:, q]
      self._cached = (obs, rewards, terms, truncs, infos)
    elif not self._fused:
      eng.agent_views(out=self._view_buf)
    obs, rewards, terms, truncs, infos = self._cached
    obs, infos = dict(obs), {a: dict(d) for a, d in infos.items()}
    if not self._ascii and not self._fused:
      obs = {a: self._vm[v.long()] for a, v in obs.items()}
    if self._layers or self._coords:                            # two more launches, tensors stay on the device
      cube = eng.observe_layers()
      agent_cubes = eng.agent_layer_views(layers=cube)
    if self._coords:                                            # and two for the coordinate lists, into persistent buffers
      eng.layer_coords(layers=cube, cap=self._coords_out[1].shape[2], out=self._coords_out)
      per_agent = eng.agent_layer_coords(agent_cubes, cap=self._agent_coords_out[1].shape[3], out=self._agent_coords_out)
      for i, a in enumerate(self.possible_agents):
        infos[a][INFO_OBSERVATION_COORDINATES + "_count"], infos[a][INFO_OBSERVATION_COORDINATES] = self._coords_out
        infos[a][INFO_AGENT_OBSERVATION_COORDINATES + "_count"], infos[a][INFO_AGENT_OBSERVATION_COORDINATES] = per_agent[self._slots[i]]
    if self._targets:
      sim = eng.simulate_moves()
      for i, a in enumerate(self.possible_agents):
        infos[a]["action_target_tile"], infos[a]["action_blocked"] = sim["target_tile"][:, self._slots[i]], sim["blocked"][:, self._slots[i]]
    if self._layers:
      for i, a in enumerate(self.possible_agents):
        infos[a]["info_observation_layers_order"] = self.layers_order
        infos[a]["info_observation_layers_cube"] = cube
        infos[a]["info_agent_observation_layers_order"] = self.layers_order
        infos[a]["info_agent_observation_layers_cube"] = agent_cubes[self._slots[i]]
    return obs, dict(rewards), dict(terms), dict(truncs), infos

  def _reseed(self, mask, seed, layout):
    """The reference's reseeding at a reset that names a seed or an env layout (safety_game_moma.py:822-864), for the masked envs:
    one launch (sgw_seed_rng) in front of the engine reset."""
    if not self._has_rng:
      raise N.SgwError("reset(seed= / env_layout_seed=): this env configuration draws from no env generator")
    if seed is not None:                                         # new_seed = int(seed) & 0xFFFFFFFF; the layout seed plays no part
      if torch.is_tensor(seed):
        self._env.engine.seed_rng(seeds=seed, mask=mask, low32=True)
      else:
        self._env.engine.seed_rng(base=int(seed), mask=mask, low32=True)
      return
    # new_seed = zlib.crc32(b''.join(x.to_bytes(4, 'big') for x in (original_seed, env_layout_seed, 17122023)))
    lo, hi = self._seed_base + self._env_id_base, self._seed_base + self._env_id_base + self.num_envs - 1
    if lo < 0 or hi >= 1 << 32:
      raise OverflowError("int too big to convert" if hi >= 1 << 32 else "can't convert negative int to unsigned")
    if not torch.is_tensor(layout):
      vals = [int(x) for x in np.asarray(layout, dtype=object).reshape(-1)]
      if any(x < 0 for x in vals):
        raise OverflowError("can't convert negative int to unsigned")
      if any(x >= 1 << 32 for x in vals):
        raise OverflowError("int too big to convert")
    self._env.engine.seed_rng(base=self._seed_base, layout_seeds=layout, mask=mask)

  def reset(self, mask=None, seed=None, options=None):
    """New episode in every env (or where mask[n] != 0).  seed (an int: env i gets (seed + global id) & 0xFFFFFFFF; or an [N]
    tensor: seed[i] & 0xFFFFFFFF) and options={"env_layout_seed": L} (an int or an [N] tensor; "trial_no" is its alias; env i gets
    crc32(original seed of env i, L, 17122023)) first give those envs a new generator stream, as the reference's reset does; naming
    a layout seed always reseeds."""
    layout = None
    if options:
      layout = options.get("env_layout_seed")
      if options.get("trial_no") is not None:
        layout = options["trial_no"]
    if seed is not None or layout is not None:
      self._reseed(mask, seed, layout)
    o = self._env.engine.reset(mask)             # straight to the engine: the L4 TimeStep bookkeeping is a dozen torch launches
    self._env._last = o
    obs, _, _, _, infos = self._pack(o)
    return obs, infos

  def set_current_q_value_per_action(self, q):
    """q: {agent: float64 (or float32, widened) device tensor [N, n_actions, D]} (an agent that is missing contributes zeros), or
    None: every following step() first folds the Q-vectors into `q_value_per_tiletype` [N, A, L, D] (agent columns in the
    library's order, `agent_slots`): where each action would lead from the current observation and the mean Q-vector per tile
    type, per agent, as the reference's step(actions, q_value_per_action) does for its one agent."""
    if q is None:
      self._q = None
      return
    first = next(iter(q.values()))
    full = torch.zeros((self.num_envs, self.spec_.A) + tuple(first.shape[1:]), dtype=torch.float64, device=self.device)
    for i, a in enumerate(self.possible_agents):
      if a in q:
        full[:, self._slots[i]] = q[a]
    self._q = full

  @property
  def q_value_per_tiletype(self):
    return self._env.q_value_per_tiletype

  def step(self, actions):
    """actions: {agent: int8 / int64 tensor [N] on the device (or a python int for every env)}; a missing agent does not play
    this round (EnvironmentMa.step plays exactly the agents in the dict).  Or ONE int8 tensor [N, A] already in the library's column order
    (`agent_slots`): no per-agent copy."""
    sp = self.spec_
    if torch.is_tensor(actions):                                 # already the library's layout: int8 [N, A] by column (no copy)
      acts = actions
    else:
      for i, a in enumerate(self.possible_agents):
        col = self._acts[:, self._slots[i]]
        v = actions.get(a)
        if v is None:                                            # not in the dict: the agent does not play this round (PM:173-246)
          col.fill_(-1)
        elif torch.is_tensor(v):
          col.copy_(v.reshape(-1))
        else:
          col.fill_(int(v))
      acts = self._acts
    if self._q is not None:
      self._env.fold_q_values(self._q)
    o = self._env.engine.step(acts.reshape(-1) if sp.A == 1 else acts)
    self._env._log_step()
    self._env._last = o
    return self._pack(o)
