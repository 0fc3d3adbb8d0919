"""BatchedSafetyEnvironment: the L4 `SafetyEnvironment*` surface (reset / step / get_last_performance /
environment_data-like accessors) for N lockstep env instances on one MI355X.

Mirrors shared/safety_game.py:82-316 and shared/safety_game_mo.py:148-1107 for what is on the step
path, step(actions, q_value_per_action) with its q_value_per_tiletype table included; CSV logging is
step_log.py; the class-level episode/trial counters are host-side observability and out of scope
(SURVEY.md §2 rows 13, 25).
"""
import collections
import enum

import numpy as np
import torch

from . import _native as N
from .engine import BatchedEngine, EpisodeLog, ALL_OUTPUTS
from .specs import make_spec


class StepType(enum.IntEnum):      # shared/rl/environment.py:62-80
  FIRST = 0
  MID = 1
  LAST = 2

  def first(self): return self is StepType.FIRST
  def mid(self): return self is StepType.MID
  def last(self): return self is StepType.LAST


class TerminationReason(enum.IntEnum):   # shared/termination_reason_enum.py:25-39
  TERMINATED = 0
  MAX_STEPS = 1
  INTERRUPTED = 2
  QUIT = 3


class TimeStep(collections.namedtuple("TimeStep", ["step_type", "reward", "discount", "observation"])):
  """Batched analogue of shared/rl/environment.py:29-60: every field is an array over envs."""
  __slots__ = ()


class BatchedSafetyEnvironment(object):

  def __init__(self, env_name, num_envs=1, device="cuda:0", env_id_base=0, outputs=None, track_performance=True, episode_log=None,
               scalarise=False, **kwargs):
    self.env_name = env_name
    self._track_performance = bool(track_performance)     # get_last_performance bookkeeping: two more device ops per step
    self.spec = make_spec(env_name, **kwargs)
    # scalarise=True (safety_game_mo.py:174, 276; safety_game_moma.py:177, 281): TimeStep.reward and the performance getters
    # become the reference's left-to-right sum over the reward dimensions, from one more library call per step (sgw_scalarise).
    # The constructors of the original scalar-reward envs take no such argument
    self.scalarise = bool(scalarise)
    if self.scalarise and self.spec.scalar:
      raise TypeError("%s: unknown argument 'scalarise'" % env_name)
    self.num_envs = int(num_envs)
    if outputs is None:        # everything the family produces ('safety2_<agent>' exists in aintelope_savanna only)
      outputs = ALL_OUTPUTS + (("safety2",) if self.spec.name == "aintelope_savanna" else ())
    if self.scalarise:         # what the sums read
      outputs = tuple(dict.fromkeys(tuple(outputs) + ("reward", "cumulative", "frame")))
    if episode_log is not None:       # the log's sources are asked for too
      outputs = tuple(dict.fromkeys(tuple(outputs) + ("step_type",) + tuple(EpisodeLog.SOURCE.values())))
    self.engine = BatchedEngine(self.spec, self.num_envs, device=device, env_id_base=env_id_base,
                                outputs=outputs)
    self.device = self.engine.device
    # episode_log=cap: every step() appends the episodes it ended to a device-side EpisodeLog of `cap` records (one more library
    # call per step, no torch op, no synchronisation); None: no log, no buffer, nothing changes
    self.episode_log = None if episode_log is None else EpisodeLog(self.engine, int(episode_log))
    self._steps = 0                   # steps taken so far: the `step` of the records
    self.q_value_per_action = None    # set_current_q_value_per_action: the Q-values of the next step()
    self._last = None
    self._last_performance = None     # [N, K] of the most recently finished episode per env (NaN = none yet)
    self._performance_sum = None      # [N, K] running sum over the env's finished episodes; _episodes int64 [N] their number
    self._episodes = None

  # ---- specs ----------------------------------------------------------------------------------
  def action_spec(self):
    """(minimum, maximum) inclusive, like BoundedArraySpec (pycolab_interface_mo.py:235-262)."""
    return (self.spec.action_lo, self.spec.action_lo + self.spec.n_actions - 1)

  @property
  def enabled_reward_dimension_keys(self):
    return list(self.spec.dim_names)

  # ---- stepping -------------------------------------------------------------------------------
  def _timestep(self, o):
    self._last = o
    st = o["step_type"].reshape(self.num_envs, -1)
    if self.spec.per_agent:                # agents finish individually: the env is LAST once all are LAST/DEAD
      done_all, first_all = (st >= N.LAST).all(dim=1), (st == N.FIRST).all(dim=1)
      st = torch.where(done_all, torch.full_like(st[:, 0], N.LAST), torch.where(first_all, torch.full_like(st[:, 0], N.FIRST),
                                                                               torch.full_like(st[:, 0], N.MID)))
    else:
      st = st[:, 0]                                           # all agents of an env share the step type
    if self._track_performance and ("cumulative" in o or "hidden" in o):      # _calculate_episode_performance (safety_game.py:253-263)
      self._track(o)
    reward = o.get("reward")
    if self.scalarise:                                        # the vectors stay in the observation; FIRST rows sum to 0.0
      o.update(self.engine.scalarise())
      reward = o["scalar_reward"]
    return TimeStep(step_type=st, reward=reward, discount=o.get("discount"), observation=o)

  def _perf_source(self, o):
    use_hidden = self.spec.scalar and self.spec.performance == "hidden"   # distributional_shift keeps the default: episode return
    return ("hidden", 1) if use_hidden and "hidden" in o else ("cumulative", self.spec.A * self.spec.K)

  def _track(self, o):
    """Device-side _episodic_performances bookkeeping (sgw_track_performance): last performance, running sum and episode count
    per env, updated where the step that just ran was LAST."""
    import ctypes as C
    name, cols = self._perf_source(o)
    if o.get(name) is None or "step_type" not in o:
      return
    if self._last_performance is None:
      self._last_performance = torch.full((self.num_envs, cols), float("nan"), dtype=torch.float64, device=self.device)
      self._performance_sum = torch.zeros((self.num_envs, cols), dtype=torch.float64, device=self.device)
      self._episodes = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
    eng = self.engine
    N.check(eng._lib.sgw_track_performance(eng._h, eng._bufs[name].data_ptr(), cols, eng._bufs["step_type"].data_ptr(),
                                           self._last_performance.data_ptr(), self._performance_sum.data_ptr(),
                                           self._episodes.data_ptr(), None, eng._stream()), "sgw_track_performance")

  def reset(self, mask=None):
    return self._timestep(self.engine.reset(mask))

  def set_current_q_value_per_action(self, q_value_per_action):
    """gym's step() takes no further arguments, so the Q-values of the NEXT step are left here (safety_game_mo.py:1256-1258):
    a [N, A, n_actions, D] device tensor ([N, n_actions, D] with one agent), or None.  The value stays until it is replaced."""
    self.q_value_per_action = q_value_per_action

  def fold_q_values(self, q_value_per_action):
    """What SafetyEnvironmentMo.step(actions, q_value_per_action) does BEFORE it plays the step (safety_game_mo.py:815-854): where
    each action would lead from the observation the envs are at (BatchedEngine.simulate_moves) and the per-tile-type means of
    the Q-vectors (BatchedEngine.fold_q_values) into `q_value_per_tiletype` float64 [N, A, L, D], which persists across steps,
    episodes and resets.  Two launches, no synchronisation.  Q-values are float64; a float32 tensor is widened, so the mean is
    a float64 mean of the widened values.  (The reference does this only while its `tiletype_qvalue` log column is on; here the
    table is kept whenever Q-values are given, and StepLogger reads it.)"""
    if not torch.is_tensor(q_value_per_action):
      q_value_per_action = torch.as_tensor(np.asarray(q_value_per_action, dtype=np.float64))
    q = q_value_per_action.to(self.device)
    self.engine.simulate_moves()
    return self.engine.fold_q_values(q)

  @property
  def q_value_per_tiletype(self):
    """float64 [N, A, L, D] over engine.q_value_tile_chars (the spec's tile_types, then the agents' characters); None before the
    first step with Q-values."""
    return getattr(self.engine, "q_value_per_tiletype", None)

  def step(self, actions, q_value_per_action=None):
    if not torch.is_tensor(actions):
      actions = torch.as_tensor(np.asarray(actions).reshape(-1), dtype=torch.int8)
    if q_value_per_action is None:
      q_value_per_action = self.q_value_per_action
    if q_value_per_action is not None:
      self.fold_q_values(q_value_per_action)
    o = self.engine.step(actions)
    self._log_step()
    return self._timestep(o)

  def _log_step(self):
    """After a step (the wrappers that call the engine themselves come here too): append the episodes it ended."""
    if self.episode_log is not None:
      self.engine.log_episodes(self.episode_log, step_base=self._steps)
      self._steps += 1

  def episodic_performances(self):
    """The reference's _episodic_performances (safety_game.py:253-263) as ONE list for the whole batch, in the order the episodes
    ended: (env int32 [n], performance float64 [n, cols]) from the source get_last_performance uses (hidden performance, or the
    episode return).  Needs episode_log; synchronises (EpisodeLog.count)."""
    if self.episode_log is None:
      raise N.SgwError("episodic_performances needs episode_log=<cap> at construction")
    rec = self.episode_log.records()
    name, cols = self._perf_source(self.engine._bufs)
    perf = rec["hidden"] if name == "hidden" else rec["ret"]
    return rec["env"], perf.reshape(perf.shape[0], cols)

  def get_last_performance(self, default=None):
    """Per env: performance of the last finished episode (safety_game.py:229-251); NaN rows = none yet."""
    if self._last_performance is None:
      return default
    if self.scalarise:                 # np.float64(sum(reward_dims)) per env (and agent: the reference's MoMa getter raises here)
      return self.engine.scalarise_rows(self._last_performance)
    return self._last_performance

  def get_overall_performance(self, default=None):
    """Per env: the mean of the performances of its finished episodes, sum(_episodic_performances) / len(...) in the reference's
    left-to-right order (safety_game.py:194-208, 234-244; safety_game_mo.py:917-938); NaN rows = no episode finished yet.
    `episodes_finished()` gives the counts."""
    if self._last_performance is None:
      return default
    mean = self._performance_sum / self._episodes.to(torch.float64)[:, None]      # 0 / 0 = NaN where none finished
    if self.scalarise:                 # the sum of the per-dimension means, left to right (safety_game_mo.py:932-934); NaN stays NaN
      return self.engine.scalarise_rows(mean)
    return mean

  def episodes_finished(self):
    return None if self._last_performance is None else self._episodes

  def set_episode_bits(self, bits, seed=0):
    self.engine.set_episode_bits(bits, seed)

  def close(self):
    self.engine.close()
