"""Table policies: closed-loop stepping without a host round trip (sgw_policy_act / sgw_policy_step_n, include/sgw.h).

A table policy is a linear score over the one-hot encoding of the observation bytes: per agent a, cell c, observation code g and
action j one float32 weight, summed over the cells in order (no multiply), plus a bias; the greedy action is the first maximum,
and with probability epsilon a Philox draw keyed by (seed, global env id, agent, step) replaces it.  With P tables and a per-env
table index one call evaluates a whole population -- tabular, evolution-strategy and policy-search loops rewrite `weights` in
place and replay one captured graph per generation:

    eng = BatchedEngine(make_spec("island_navigation_ex", level=9), 65536, outputs=("board", "reward", "cumulative", "frame", "step_type"))
    pol = TablePolicy(eng, n_policies=256)
    pol.set_policy_of_env(torch.arange(eng.n_envs, device=eng.device, dtype=torch.int32) % 256)
    eng.reset()
    for generation in range(100):
      pol.weights.copy_(candidates)                       # in place: the captured graph reads through the pointer
      traj = eng.policy_step_n(pol, 64, write_every=True)  # 129 launches, one graph replay from the third call on
      scal = eng.scalarise(T=64)                           # the [T, N_pad, ...] buffers feed scalarise / log_episodes as they are

The device tensors are owned by the policy and may be written at any time; their pointers must not change between calls that
are meant to hit the graph cache (assign with copy_ / fill_, not by rebinding the attributes).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _native as N

SOURCES = {"board": N.POLICY_BOARD, "views": N.POLICY_VIEWS}


def explore_below_of(epsilon):
  """epsilon in [0, 1] -> the threshold the 32-bit draw is compared with: explore iff x0 < explore_below (2^32 = always)."""
  if not (0.0 <= float(epsilon) <= 1.0):
    raise ValueError("epsilon must be in [0, 1]")
  return min(2 ** 32, int(float(epsilon) * 2 ** 32))


LOG2_E = 1.4426950408889634


def beta2_of(tau):
  """temperature -> beta2, the np.float32 the softmax entry points take (inverse temperature * log2(e)); None stays None."""
  if tau is None:
    return None
  tau = float(tau)
  if not tau > 0.0:
    raise ValueError("temperature must be > 0 (math.inf: uniform), or None for the greedy policy")
  beta2 = 0.0 if math.isinf(tau) else LOG2_E / tau
  if beta2 > float(np.finfo(np.float32).max):
    raise ValueError("temperature %r is too small: beta2 overflows float32" % tau)
  return np.float32(beta2)


def policy_cells(spec, source):
  """C of a table for this spec and source: H*W, or the largest window's h*w."""
  if source == "board":
    return int(spec.H * spec.W)
  shapes = spec.view_shapes
  return int(max([h * w for (h, w) in shapes] or [0]))


class TablePolicy(object):
  """weights float32 [P, A, C, G, n_actions] (zero-initialised), bias float32 [P, A, n_actions], step int64 [1], code_of uint8
  [256] on the engine's device.  Byte chars[i] has code i + 1, every other byte code 0; G = len(chars) + 1.  chars defaults to
  spec.layer_chars."""

  def __init__(self, engine, source="board", chars=None, n_policies=1, seed=0, epsilon=0.0):
    if source not in SOURCES:
      raise ValueError("source must be 'board' or 'views'")
    spec = engine.spec
    if chars is None:
      chars = spec.layer_chars
      if chars is None:
        raise ValueError("TablePolicy: this spec names no layer characters; pass chars")
    chars = [c if isinstance(c, str) else chr(c) for c in chars]
    if len(set(chars)) != len(chars) or not 0 <= len(chars) <= 63 or any(len(c) != 1 or ord(c) > 255 for c in chars):
      raise ValueError("chars must be at most 63 distinct single bytes")
    cells = policy_cells(spec, source)
    if cells <= 0:
      raise N.SgwError("TablePolicy: source 'views' on a spec without agent windows")
    if int(n_policies) < 1:
      raise ValueError("n_policies must be >= 1")
    self.spec, self.device, self.n_envs = spec, engine.device, engine.n_envs
    self.source, self.chars = source, "".join(chars)
    self.n_policies, self.cells, self.n_codes = int(n_policies), cells, len(chars) + 1
    self.n_actions, self.action_lo = int(spec.n_actions), int(spec.action_lo)
    self.seed = int(seed) & ((1 << 64) - 1)
    self.explore_below = explore_below_of(epsilon)
    code = np.zeros(256, np.uint8)
    for i, c in enumerate(chars):
      code[ord(c)] = i + 1
    dev = self.device
    self.code_of = torch.from_numpy(code).to(dev)
    self.weights = torch.zeros((self.n_policies, spec.A, cells, self.n_codes, self.n_actions), dtype=torch.float32, device=dev)
    self.bias = torch.zeros((self.n_policies, spec.A, self.n_actions), dtype=torch.float32, device=dev)
    self.policy_of_env = None
    self.beta2 = None          # None: greedy; else the float32 inverse temperature * log2(e) of the softmax policy (set_temperature)
    self.step = torch.zeros(1, dtype=torch.int64, device=dev)
    self._struct = None
    self._acc = None          # (acc_weights, acc_bias): the int64 gradient sums, allocated on first use
    self.acc_frac_bits = None  # the frac_bits of the sums now in the accumulators (None: they are zero)

  @property
  def acc_weights(self):
    """int64 [P, A, C, G, n_actions]: the fixed-point gradient sums of policy_accumulate (zeroed; allocated on first use)."""
    return self._accumulators()[0]

  @property
  def acc_bias(self):
    """int64 [P, A, n_actions]: the bias's gradient sums."""
    return self._accumulators()[1]

  def _accumulators(self):
    if self._acc is None:
      self._acc = (torch.zeros(tuple(self.weights.shape), dtype=torch.int64, device=self.device),
                   torch.zeros(tuple(self.bias.shape), dtype=torch.int64, device=self.device))
    return self._acc

  def code(self, ch):
    """The code of a byte (0 for every byte that is not among chars)."""
    ch = ch if isinstance(ch, str) else chr(ch)
    return self.chars.index(ch) + 1 if ch in self.chars else 0

  def set_epsilon(self, epsilon):
    self.explore_below = explore_below_of(epsilon)
    self._struct = None

  def set_temperature(self, tau):
    """None: the greedy policy (the first maximum).  tau > 0: a SOFTMAX policy, pi_j proportional to exp(score[j] / tau), sampled on
    the device by act / policy_step_n / policy_rollout (include/sgw.h fixes the arithmetic): beta2 = float32(log2(e) / tau).
    math.inf: beta2 = 0, uniform over the finite scores.  epsilon-exploration still comes first.  Returns the policy."""
    self.beta2 = beta2_of(tau)
    return self

  @property
  def temperature(self):
    """tau of set_temperature as beta2 restates it (None: greedy; inf for beta2 == 0)."""
    if self.beta2 is None:
      return None
    return math.inf if self.beta2 == 0 else LOG2_E / float(self.beta2)

  def set_policy_of_env(self, index):
    """int32 [N]: the table of every env (None: table 0 everywhere).  An index outside 0 .. P-1 makes that env's actions 0."""
    if index is None:
      self.policy_of_env = None
    else:
      index = torch.as_tensor(index).reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
      if index.numel() != self.n_envs:
        raise ValueError("policy_of_env must have n_envs entries")
      self.policy_of_env = index
    self._struct = None

  def native(self):
    """The sgw_policy of this policy (rebuilt only when a pointer or scalar changed: the graph cache compares it by value)."""
    ptrs = (self.code_of.data_ptr(), self.weights.data_ptr(), self.bias.data_ptr(),
            self.policy_of_env.data_ptr() if self.policy_of_env is not None else None, self.step.data_ptr(), self.explore_below, self.seed)
    if self._struct is None or self._struct[0] != ptrs:
      p = N.Policy()
      p.source, p.n_policies, p.n_codes, p.cells = SOURCES[self.source], self.n_policies, self.n_codes, self.cells
      p.code_of, p.weights, p.bias, p.policy_of_env, p.step_dev, p.explore_below, p.seed = ptrs
      self._struct = (ptrs, p)
    return self._struct[1]

  @classmethod
  def from_cell_actions(cls, engine, table, agent_chr=None):
    """The per-cell policy: `table` int [H*W] of actions; the agent standing on cell c takes table[c].  Weight 1.0 at
    (cell, code(agent's character), table[cell] - action_lo), source 'board'.  agent_chr: the character to look for (default:
    every agent its own, spec.agent_chars)."""
    spec = engine.spec
    table = np.asarray(table).reshape(-1)
    if table.size != spec.H * spec.W:
      raise ValueError("table must have H*W entries")
    pol = cls(engine, source="board")
    idx = table.astype(np.int64) - pol.action_lo
    if idx.min() < 0 or idx.max() >= pol.n_actions:
      raise ValueError("table holds an action outside the spec's range")
    w = np.zeros(tuple(pol.weights.shape), np.float32)
    chars = list(spec.agent_chars)
    slots = spec.agent_slots      # the output column of each present agent
    for a, own in zip(slots, chars):
      ch = agent_chr if agent_chr is not None else own
      g = pol.code(ch)
      if g == 0:
        raise ValueError("agent character %r is not among the policy's chars %r" % (ch, pol.chars))
      w[0, a, np.arange(table.size), g, idx] = 1.0
    pol.weights.copy_(torch.from_numpy(w))
    return pol
