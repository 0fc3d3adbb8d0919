"""BatchedEngine: N lockstep env instances behind libsgw.so.

PyTorch is used only as plumbing: it owns the output buffers (device tensors), the stream and --
for the multi-GPU case -- the process group.  Every compute step is one call through the C ABI
(include/sgw.h) into a hand-written HIP kernel; there is no eager/CPU fallback.

    eng = BatchedEngine(make_spec("island_navigation_ex"), n_envs=65536, device="cuda:0")
    obs = eng.reset()                       # dict of [N, ...] device tensors (views, rewritten by each call)
    obs = eng.step(actions_int8)            # one env.step() in every env (auto-reset after LAST)
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)

DEFAULT_OUTPUTS = ("board", "reward", "step_type", "term_reason")
# every family's outputs; "safety2": aintelope_savanna only; "views" / "obs_views": the families with agent windows
ALL_OUTPUTS = tuple(f for f in N.OUT_FIELDS if f not in ("safety2", "views", "obs_views", "obs_dir", "act_dir"))   # (family-specific outputs are asked for by name)


# families whose step launch can write the agent windows itself (sgw_out.views / obs_views)
FUSED_VIEW_FAMILIES = (N.FIREMAKER_EX_MA, N.ISLAND_NAVIGATION_EX_MA, N.AINTELOPE_SAVANNA)
# families whose envs own numpy generators (sgw_set_rng_state / sgw_seed_rng): the streams are state words
GENERATOR_FAMILIES = (N.FIREMAKER_EX_MA, N.ISLAND_NAVIGATION_EX_MA, N.AINTELOPE_SAVANNA)


def fused_views(spec):
  """Should this spec's windows come from the step launch itself (sgw_out.views / obs_views) rather than from sgw_agent_views?
  firemaker_ex_ma always (its workgroup's eight waves share the work); island_navigation_ex_ma / aintelope_savanna when no window
  is larger than the board.  Their step launch CAN write larger windows too (a chunk of envs at a time), but one wavefront per 64
  envs is slower at it than the separate launch: 126 vs 92 us per round for default aintelope_savanna at 65 536 envs, 79 vs 53 us
  for island_navigation_ex_ma with radius 3 (profiles/r06_views_inlaunch.json), so the wrappers keep two launches there."""
  if spec.family not in FUSED_VIEW_FAMILIES or not spec.view_shapes:
    return False
  return spec.family == N.FIREMAKER_EX_MA or all(h * w <= spec.H * spec.W for (h, w) in spec.view_shapes)


def _dtype_shape(spec, name):
  HW, A, K, M = spec.H * spec.W, spec.A, spec.K, max(spec.M, 1)
  per_agent = (A,) if spec.per_agent else ()     # agents terminate individually (island_navigation_ex_ma)
  return {
      "board": (torch.uint8, (HW,)), "obs_board": (torch.float32, (HW,)),
      "reward": (torch.float64, (A * K,)), "cumulative": (torch.float64, (A * K,)),
      "step_type": (torch.uint8, (A,)), "term_reason": (torch.uint8, per_agent),
      "actual_action": (torch.int8, (A,)), "discount": (torch.float64, ()),
      "hidden": (torch.float64, ()), "safety": (torch.int32, per_agent),
      "metrics": (torch.float64, (M,)), "frame": (torch.int32, ()), "agent_pos": (torch.uint8, (A * 2,)),
      "agent_flags": (torch.uint8, (A,)), "safety2": (torch.int32, per_agent),
      "views": (torch.uint8, (_view_bytes(spec),)), "obs_views": (torch.float32, (_view_bytes(spec),)),
      "done": (torch.uint8, (A,)), "obs_dir": (torch.uint8, (A,)), "act_dir": (torch.uint8, (A,)),
  }[name]


def _view_bytes(spec):
  """Bytes of one env's row of agent windows (sgw_view_bytes): the windows of the agents that have one, concatenated."""
  return int(sum(h * w for (h, w) in spec.view_shapes))


def _require(what, name, t, device, dtype, numel, layout="", contiguous=True, shape=None, also=None):
  """The one check of a tensor argument: `t` is a tensor on `device` of `dtype` (one, or a tuple of accepted ones), contiguous
  unless told otherwise, with `numel` elements (an int, a tuple of accepted ints, None: any), of `shape` if given, and `also(t)`
  holds if given.  Returns the element count that matched; SgwError otherwise, `layout` being the caller's words for the shape."""
  dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
  if (torch.is_tensor(t) and t.device == device and t.dtype in dtypes and (t.is_contiguous() or not contiguous)
      and (shape is None or tuple(t.shape) == tuple(shape)) and (also is None or also(t))):
    for m in (numel if isinstance(numel, tuple) else (numel,)):
      if m is None or t.numel() == m:
        return m
  names = [str(d).replace("torch.", "") for d in dtypes]
  raise N.SgwError("%s: %s must be a %s%s %stensor on %s (there is no CPU path)"
                   % (what, name, "contiguous " if contiguous else "", names[0] + "".join(" (or %s)" % d for d in names[1:]),
                      layout + " " if layout else "", device))


# the derived statistics of _process_timestep, in the order of the columns of sgw_derived_stats (average_reward: the K after them)
STAT_NAMES = ("gini_index", "cumulative_gini_index", "mo_variance", "cumulative_mo_variance", "average_mo_variance")


def _stats_dict(stats):
  """float64 [N, A, 5 + K] of sgw_derived_stats -> {name: [N(, A)]} and average_reward [N(, A), K], views of it."""
  st = stats[:, 0] if stats.shape[1] == 1 else stats
  out = {nm: st[..., i] for i, nm in enumerate(STAT_NAMES)}
  out["average_reward"] = st[..., len(STAT_NAMES):]
  return out


class EpisodeLog(object):
  """A device-side, append-only log of finished episodes (sgw_log_episodes): the reference's _episodic_performances
  (safety_game.py:253-263) for a whole batch, one record per episode in the order (step, env), with

      env int32 [cap], step int64 [cap], length int32 [cap], term_reason uint8 [cap] ([cap, A] where agents finish one by one),
      ret float64 [cap, A*K], hidden float64 [cap], metrics float64 [cap, M]

  for the `fields` asked for.  The log owns these tensors, the device counter and the launch's scratch (grown to the largest T
  logged).  Appending (BatchedEngine.log_episodes) never synchronises; `count()` is the one method that does.  Records beyond
  `cap` are counted but not stored (`overflowed()`)."""

  FIELDS = ("env", "step", "length", "term_reason", "ret", "hidden", "metrics")
  SOURCE = {"length": "frame", "term_reason": "term_reason", "ret": "cumulative", "hidden": "hidden", "metrics": "metrics"}

  @staticmethod
  def layout_of(spec):
    """(A, K, M, R): what decides the record's shape."""
    return (spec.A, spec.K, spec.M, spec.A if spec.per_agent else 1)

  def __init__(self, engine, cap, fields=FIELDS):
    self.fields = tuple(fields)
    for f in self.fields:
      if f not in self.FIELDS:
        raise KeyError("unknown episode-log field %r" % (f,))
    self.cap = int(cap)
    if self.cap < 0:
      raise ValueError("cap must be >= 0")
    self.device, self.n_envs, self.layout = engine.device, engine.n_envs, self.layout_of(engine.spec)
    if self.device.type != "cuda" or not torch.cuda.is_available():
      raise N.SgwError("EpisodeLog needs a HIP device (got %r); there is no CPU path" % (self.device,))
    self._lib = engine._lib
    A, K, M, R = self.layout
    shapes = {"env": (torch.int32, ()), "step": (torch.int64, ()), "length": (torch.int32, ()), "term_reason": (torch.uint8, (R,)),
              "ret": (torch.float64, (A * K,)), "hidden": (torch.float64, ()), "metrics": (torch.float64, (M,))}
    self._t = {f: torch.zeros((self.cap,) + shapes[f][1], dtype=shapes[f][0], device=self.device) for f in self.fields}
    self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
    self._scratch, self._scratch_T = None, 0
    self._x = N.Episodes()
    self._x.cap, self._x.count = self.cap, self._count.data_ptr()
    for f in self.fields:
      if self.cap > 0 and self._t[f].numel() > 0:
        setattr(self._x, f, self._t[f].data_ptr())

  def _struct(self, T):
    """The sgw_episodes of this log with scratch for T rows of the engine's envs."""
    if T > self._scratch_T:
      nbytes = int(self._lib.sgw_episode_scratch_bytes(self.n_envs, int(T)))
      if nbytes < 0:
        raise N.SgwError("sgw_episode_scratch_bytes(%d, %d) refused" % (self.n_envs, T))
      self._scratch, self._scratch_T = torch.empty(nbytes, dtype=torch.uint8, device=self.device), int(T)
      self._x.scratch = self._scratch.data_ptr()
    return self._x

  def clear(self):
    """Forget every record (zeroes the device counter; no synchronisation)."""
    self._count.zero_()

  def count(self):
    """Episodes logged so far, including those that did not fit.  Synchronises."""
    return int(self._count.item())

  def overflowed(self):
    return self.count() > self.cap

  def records(self):
    """{field: tensor [n, ...]} of the n = min(count, cap) stored records, views of the log's tensors; `ret` is [n, A, K] when
    A > 1, `term_reason` [n] unless agents finish one by one."""
    n = min(self.count(), self.cap)
    A, K, M, R = self.layout
    out = {}
    for f in self.fields:
      v = self._t[f][:n]
      if f == "ret" and A > 1:
        v = v.reshape(n, A, K)
      elif f == "term_reason" and R == 1:
        v = v.reshape(n)
      out[f] = v
    return out


# what the reference raises for an action array of the wrong size (pycolab_interface.py:160-163)
_BAD_ACTIONS = ("A pycolab Environment adapter's step method was called with actions that were "
                "not compatible with what the pycolab game expects.")


class BatchedEngine(object):
  _fold_key = None           # (also the fallback when a caller drops the instance's to make fold_q_values start a new table)

  def __init__(self, spec, n_envs, device="cuda:0", env_id_base=0, outputs=DEFAULT_OUTPUTS):
    self._h = self._look = None      # (close() runs from __del__ even when the lines below raise)
    self.spec = spec
    self.n_envs = int(n_envs)
    self.device = torch.device(device)
    if self.device.type != "cuda":
      raise N.SgwError("BatchedEngine needs a HIP device (got %r); there is no CPU path" % (device,))
    self._lib = N.lib()
    if not torch.cuda.is_available():
      raise N.SgwError("no HIP device visible to torch; the engine has no CPU fallback")
    index = self.device.index if self.device.index is not None else torch.cuda.current_device()
    self.device = torch.device("cuda", index)
    h = C.c_void_p()
    N.check(self._lib.sgw_create(C.byref(spec.native), self.n_envs, int(env_id_base), index, C.byref(h)),
            "sgw_create")
    self._h = h
    self.n_pad = int(self._lib.sgw_n_pad(h))
    self.env_id_base = int(env_id_base)
    self.outputs = tuple(outputs)
    for name in self.outputs:
      if name not in N.OUT_FIELDS:
        raise KeyError("unknown output %r" % name)
    self.view_bytes = int(self._lib.sgw_view_bytes(h))     # one env's row of agent windows; what _dtype_shape sizes `views` by
    assert self.view_bytes == _view_bytes(spec)
    self._bufs = {}
    self._out = N.Out()
    self._views_cache = None
    self._alloc_outputs(1)
    # what set_episode_bits / set_random_stream were given: (device tensor or None, seed).  The library points at the tensor, so
    # this dict is what keeps it alive (and fork() re-applies it); the next set_* call releases it.
    self._inputs = {}
    self._look = None        # lookahead()'s cached fork and result tensors
    # lazily created, each by the method named; _persistent() keeps the result buffers that are keyed per call
    self._kept = {}          # (kind, key) -> tensors: scalarise, td_targets, policy tapes, obs0 sides, policy_scores
    self._full = None        # step_full: the sgw_extras of the last flag set and its tensors
    self._karr = None        # _k_agent
    self._layers = None      # _layer_tables
    self._act_out = None     # act
    self._whatif_out = None  # simulate_moves
    self._fold_key = self._fold_chars = None       # fold_q_values, with the three below
    self.q_value_per_tiletype = self.q_value_seen = self.q_value_tile_chars = None
    table = spec.family_table
    if table is not None:    # aintelope_savanna: host-evaluated visit-count rewards (sgw_set_family_table)
      table = np.ascontiguousarray(table, dtype=np.float64)
      N.check(self._lib.sgw_set_family_table(self._h, table.ctypes.data, table.size), "sgw_set_family_table")

  # -- buffers ----------------------------------------------------------------------------------
  def _new_output(self, name, dtype, shape):
    """One output buffer (a subclass may allocate it otherwise: tests/output_subsets.py puts guard bytes around it)."""
    return torch.zeros(shape, dtype=dtype, device=self.device)

  def _alloc_outputs(self, T):
    self._T = T
    self._views_cache = None
    for name in self.outputs:
      dt, shp = _dtype_shape(self.spec, name)
      self._bufs[name] = self._new_output(name, dt, ((T, self.n_pad) if T > 1 else (self.n_pad,)) + shp)
    for name in N.OUT_FIELDS:
      setattr(self._out, name, self._bufs[name].data_ptr() if name in self._bufs else None)

  def _want_T(self, T=1, write_every=False):
    """Output buffers for a call that writes T rows per env with write_every and one otherwise: [T, N_pad, ...] or [N_pad, ...]."""
    want = T if write_every else 1
    if self._T != want:
      self._alloc_outputs(want)

  def _open(self, what):
    if self._h is None:
      raise N.SgwError("%s: the engine has no device engine behind it (closed?); there is no CPU path" % what)

  def _persistent(self, kind, key, make=None):
    """The result buffers of `kind` for `key`, made once by make() and reused by every later call (callers compare their
    data_ptr()s across calls; a per-step call allocates nothing).  make=None only looks: None when no call has made them."""
    c = self._kept.get((kind, key))
    if c is None and make is not None:
      c = self._kept[(kind, key)] = make()
    return c

  def _row(self, name):
    """(dtype, elements per env) of output `name`."""
    dt, shp = _dtype_shape(self.spec, name)
    return dt, int(np.prod(shp, dtype=np.int64))

  def _latest(self, name, t, what, optional=False):
    """The latest [N or N_pad, row] rows of output `name`: the caller's tensor `t` checked, or the engine's own buffer (its last
    row block after a write_every call).  optional: None when the engine does not write that output."""
    if t is None:
      t = self._bufs.get(name)
      if t is None:
        if optional:
          return None
        raise N.SgwError("%s: the %r output is not among this engine's outputs (%r); pass it or ask for it" % (what, name, self.outputs))
      return t[-1] if self._T > 1 else t
    self._rows_of(what, name, t, *self._row(name))
    return t

  def _rows_of(self, what, name, t, dtype, row, lead=1):
    """N or N_pad: the rows per step of a caller's [lead, N or N_pad, row] tensor (with lead == 1: [N or N_pad, row])."""
    n, n_pad = self.n_envs, self.n_pad
    m = _require(what, name, t, self.device, dtype, (lead * n * row, lead * n_pad * row),
                 "[%s%d or %d, %d]" % ("%d, " % lead if lead > 1 else "", n, n_pad, row))
    return n if m == lead * n * row else n_pad

  def _views(self):
    """{name: view of the persistent output buffer}: the views only change with a reallocation, so they are built once (a step
    from Python is host-bound: every microsecond here is throughput)."""
    if self._views_cache is not None:
      return dict(self._views_cache)
    out = {}
    for name, t in self._bufs.items():
      out[name] = self._shaped(name, t[:, :self.n_envs] if self._T > 1 else t[:self.n_envs])
    self._views_cache = out
    return dict(out)

  def _shaped(self, name, v):
    """[..., N, row] of an output buffer in the shape the API hands out."""
    if name in ("board", "obs_board"):
      v = v.reshape(v.shape[:-1] + (self.spec.H, self.spec.W))
    elif name in ("reward", "cumulative") and self.spec.A > 1:
      v = v.reshape(v.shape[:-1] + (self.spec.A, self.spec.K))
    elif name == "agent_pos":
      v = v.reshape(v.shape[:-1] + (self.spec.A, 2))
    return v

  def _stream(self):
    # the raw handle of torch's current stream on this device (torch.cuda.current_stream() builds a Stream object: 2 us per call)
    return C.c_void_p(_raw_stream(self.device.index))

  # -- API --------------------------------------------------------------------------------------
  def reset(self, mask=None):
    """New episode in every env (or where mask[n] != 0).  Returns the FIRST timestep arrays."""
    self._want_T()
    mptr = None
    if mask is not None:
      mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
      if mask.numel() != self.n_envs:
        raise ValueError("mask must have n_envs entries")
      mptr = mask.data_ptr()
    N.check(self._lib.sgw_reset(self._h, mptr, C.byref(self._out), self._stream()), "sgw_reset")
    return self._views()

  def step(self, actions):
    """actions: int8 device tensor [N] (or [N, A]).  One env.step() per env."""
    if self._T != 1:
      self._alloc_outputs(1)
    if actions.dtype != torch.int8 or actions.device != self.device or not actions.is_contiguous():
      actions = actions.to(device=self.device, dtype=torch.int8).contiguous()
    if actions.numel() != self.n_envs * self.spec.A:
      raise RuntimeError(_BAD_ACTIONS)
    N.check(self._lib.sgw_step(self._h, actions.data_ptr(), C.byref(self._out), self._stream()), "sgw_step")
    return self._views()

  def _agent_ks(self):
    sp = self.spec
    if sp.A > 1:
      slots = sp.agent_slots
      ks = [0] * sp.A                                  # by column of the library's layout; an absent agent has no dimensions
      for c, q in zip(sp.agent_chars, slots):
        ks[q] = len(sp.agent_dim_names[c])
      return ks
    return [sp.K]

  def step_full(self, actions, rgb=False, layers=False, stats=False, agent_layer_views=False, performance=False, replay=False):
    """One env.step() per env AND the derived observations of that step from ONE library call (sgw_step_full: the launches are
    chained in C; `replay`: captured and replayed as one hipGraph from the third call on -- ~5 us of host time per step instead
    of ~25, at ~5 us more GPU time per step): dict of the engine's outputs plus "RGB" uint8
    [N, 3, H, W], "layers" uint8 [N, L, H, W] (unoccluded, gap-corrected), the derived statistics (gini_index, ...,
    average_reward), "agent_layer_views" (list over agents of [N, L, h, w]) and, with `performance`, "last_performance" /
    "performance_sum" float64 [N, C] and "episodes" int64 [N] (get_last_performance / get_overall_performance bookkeeping).
    The extra tensors are persistent buffers, rewritten by every call, like the engine's outputs."""
    sp = self.spec
    if self._T != 1:
      self._alloc_outputs(1)
    if actions.dtype != torch.int8 or actions.device != self.device or not actions.is_contiguous():
      actions = actions.to(device=self.device, dtype=torch.int8).contiguous()
    if actions.numel() != self.n_envs * sp.A:
      raise RuntimeError(_BAD_ACTIONS)
    key = (bool(rgb), bool(layers or agent_layer_views), bool(stats), bool(agent_layer_views), bool(performance), bool(replay))
    fx = self._full
    if fx is None or fx["key"] != key or fx["for"] is not self._bufs.get("step_type", self._bufs.get("board")):
      n, dev = self.n_envs, self.device
      x, t, res = N.Extras(), {}, {}
      x.replay = 1 if replay else 0
      if key[0]:
        t["lut"] = torch.from_numpy(sp.rgb_lut().reshape(-1)).to(dev)
        res["RGB"] = torch.empty((n, 3, sp.H, sp.W), dtype=torch.uint8, device=dev)
        x.rgb, x.rgb_lut_dev = res["RGB"].data_ptr(), t["lut"].data_ptr()
      if key[1]:
        L = len(sp.layer_chars)
        chars, stat, x.gap_index, x.hidden_layer = self._layer_tables()
        res["layers"] = torch.empty((n, L, sp.H, sp.W), dtype=torch.uint8, device=dev)
        x.layers, x.layer_chars_dev, x.n_layers = res["layers"].data_ptr(), chars.data_ptr(), L
        if stat is not None:
          x.layer_static_dev = stat.data_ptr()
      else:
        x.hidden_layer, x.gap_index = -1, -1
      if key[2]:
        t["stats"] = torch.empty((n, sp.A, 5 + sp.K), dtype=torch.float64, device=dev)
        x.stats = t["stats"].data_ptr()
        x.k_agent = self._k_agent()                                   # (a struct field: copied by value)
        res.update(_stats_dict(t["stats"]))
      if key[3]:
        L = len(sp.layer_chars)
        t["cubes"] = torch.empty((n, self.view_bytes * L), dtype=torch.uint8, device=dev)
        x.agent_layer_views = t["cubes"].data_ptr()
        res["agent_layer_views"] = self.split_views(t["cubes"], L)
      if key[4]:
        use_hidden = sp.scalar and sp.performance == "hidden"
        C_ = 1 if use_hidden else sp.A * sp.K
        res["last_performance"] = torch.full((n, C_), float("nan"), dtype=torch.float64, device=dev)
        res["performance_sum"] = torch.zeros((n, C_), dtype=torch.float64, device=dev)
        res["episodes"] = torch.zeros(n, dtype=torch.int64, device=dev)
        t["done"] = torch.zeros(n, dtype=torch.uint8, device=dev)
        res["done"] = t["done"].view(torch.bool)                     # the episode ended with this step (the wrapper's `terminated`)
        x.perf_from_hidden = 1 if use_hidden else 0
        x.perf_last, x.perf_sum, x.perf_count = res["last_performance"].data_ptr(), res["performance_sum"].data_ptr(), res["episodes"].data_ptr()
        x.done = t["done"].data_ptr()
      fx = self._full = {"key": key, "for": self._bufs.get("step_type", self._bufs.get("board")), "x": x, "keep": t, "res": res}
    N.check(self._lib.sgw_step_full(self._h, actions.data_ptr(), C.byref(self._out), C.byref(fx["x"]), self._stream()), "sgw_step_full")
    if fx.get("all") is None:
      fx["all"] = self._views()
      fx["all"].update(fx["res"])
    return dict(fx["all"])

  def _tape(self, actions):
    """T of an action tape int8 [T, N(, A)] for step_n / replay, which take it as it is: resident on the device, contiguous."""
    T = int(actions.shape[0])
    assert actions.dtype == torch.int8 and actions.is_contiguous() and actions.device == self.device
    assert actions.numel() == T * self.n_envs * self.spec.A
    return T

  def step_ptr(self, actions_ptr):
    """Launch-only variant for tight loops: raw device pointer, no tensor checks, no views."""
    N.check(self._lib.sgw_step(self._h, actions_ptr, C.byref(self._out), self._stream()), "sgw_step")

  def step_n(self, actions, write_every=False, accumulate=False):
    """actions int8 [T, N(, A)] resident on the device: T step launches issued from C (no Python in
    the loop).  Returns the last step's arrays, or [T, N, ...] arrays with write_every."""
    T = self._tape(actions)
    self._want_T(T, write_every)
    N.check(self._lib.sgw_step_n(self._h, actions.data_ptr(), T, 1 if write_every else 0, C.byref(self._out),
                                 1 if accumulate else 0, self._stream()), "sgw_step_n")
    return self._views()

  def read_returns(self, clear=False):
    """float64 [A*K + 1] device tensor: (sum of finished episodes' return vectors, #episodes) over this
    engine's envs since the accumulators were last cleared -- the buffer to all-reduce across GPUs."""
    out = torch.empty(self.spec.A * self.spec.K + 1, dtype=torch.float64, device=self.device)
    N.check(self._lib.sgw_read_returns(self._h, out.data_ptr(), 1 if clear else 0, self._stream()),
            "sgw_read_returns")
    return out

  def rollout(self, T, seed, step0=0, write_every=False, accumulate=False):
    """T fused steps with in-kernel synthetic actions.  write_every: outputs become [T, N, ...]."""
    self._want_T(T, write_every)
    N.check(self._lib.sgw_rollout(self._h, int(T), int(seed), int(step0), 1 if write_every else 0,
                                  C.byref(self._out), 1 if accumulate else 0, self._stream()), "sgw_rollout")
    return self._views()

  def replay(self, actions, write_every=False, accumulate=False):
    """actions int8 [T, N(, A)] resident on the device: the T steps in ONE fused launch (state in registers), output for
    output what step_n gives for the same buffer."""
    T = self._tape(actions)
    self._want_T(T, write_every)
    N.check(self._lib.sgw_replay(self._h, actions.data_ptr(), T, 1 if write_every else 0, C.byref(self._out),
                                 1 if accumulate else 0, self._stream()), "sgw_replay")
    return self._views()

  def fill_actions(self, T, seed, step0=0):
    """int8 [T, N] (or [T, N, A]) synthetic actions, same stream the fused rollout draws."""
    shape = (T, self.n_envs) + ((self.spec.A,) if self.spec.A > 1 else ())
    acts = torch.empty(shape, dtype=torch.int8, device=self.device)
    N.check(self._lib.sgw_fill_actions(self._h, int(T), int(seed), int(step0), acts.data_ptr(), self._stream()),
            "sgw_fill_actions")
    return acts

  def accumulate_returns(self, ep_accum):
    """ep_accum[:A*K] += episode returns of envs that just ended, ep_accum[A*K] += their count."""
    if "cumulative" not in self._bufs or "step_type" not in self._bufs or self._T != 1:
      raise N.SgwError("accumulate_returns needs the 'cumulative' and 'step_type' outputs")
    N.check(self._lib.sgw_accumulate_returns(self._h, self._bufs["cumulative"].data_ptr(),
                                             self._bufs["step_type"].data_ptr(), ep_accum.data_ptr(),
                                             self._stream()), "sgw_accumulate_returns")

  def set_episode_bits(self, bits, seed=0):
    """The one random bit per game build of the families that take one: uint8 [N, n], the k-th episode of env i uses
    bits[i, k % n].  safe_interruptibility(_ex): should_interrupt; absent_supervisor (supervisor=None): the supervisor is present;
    distributional_shift (is_testing=True): test level 2 instead of 1.  Other families and configurations read nothing.
    None: drawn in the kernel from u = Philox(seed, global env id = env_id_base + i, k), uniform in [0, 1):
    safe_interruptibility(_ex) u <= interruption_probability (inclusive); absent_supervisor and distributional_shift u < 0.5
    (strict: np.random.rand() < 0.5, np.random.choice of two)."""
    self._drop_lookahead()
    if bits is None:
      N.check(self._lib.sgw_set_episode_bits(self._h, None, 0, int(seed)), "sgw_set_episode_bits")
      self._inputs["episode_bits"] = (None, int(seed))
      return
    bits = torch.as_tensor(bits).to(device=self.device, dtype=torch.uint8).contiguous()
    assert bits.dim() == 2 and bits.shape[0] == self.n_envs
    N.check(self._lib.sgw_set_episode_bits(self._h, bits.data_ptr(), bits.shape[1], int(seed)),
            "sgw_set_episode_bits")
    self._inputs["episode_bits"] = (bits, int(seed))

  def set_random_stream(self, u, seed=0):
    """Random numbers for the families that draw from the process-global numpy RNG an input-dependent number of times:
    float64 [N, n], the k-th draw of env i is u[i, k % n]; the draw counter is env state and runs on across episodes.
    tomato_watering / tomato_crmdp: one per watered tomato and step (and game build), dries where u < 0.05; friend_foe: per game
    build the bandit type floor(3u) (bandit_type=None only), then for a neutral bandit the rewarding box (u <= 0.6: the first);
    whisky_gold (human_player=True, after the whisky): per step u < whisky_exploration replaces the action, by direction
    floor(4u') of a second draw.  Other families and configurations read nothing.
    None: drawn in the kernel, draw k = word pair k & 1 of Philox(seed, global env id = env_id_base + i, block k >> 1)."""
    self._drop_lookahead()
    if u is None:
      N.check(self._lib.sgw_set_random_stream(self._h, None, 0, int(seed)), "sgw_set_random_stream")
      self._inputs["random_stream"] = (None, int(seed))
      return
    if not (torch.is_tensor(u) and u.dtype == torch.float64):
      u = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64))
    u = u.to(self.device).contiguous()
    assert u.dim() == 2 and u.shape[0] == self.n_envs
    N.check(self._lib.sgw_set_random_stream(self._h, u.data_ptr(), u.shape[1], int(seed)), "sgw_set_random_stream")
    self._inputs["random_stream"] = (u, int(seed))

  def set_rng_seeds(self, seeds):
    """firemaker_ex_ma / island_navigation_ex_ma: per-env numpy streams Generator(PCG64(SeedSequence(seed))) -- what
    gymnasium.utils.seeding.np_random(seed) builds (safety_game_mo.py:283-291).  seeds: int array [N]."""
    seeds = np.asarray(seeds).reshape(-1)
    assert len(seeds) == self.n_envs
    m = (1 << 64) - 1
    words = np.empty((self.n_envs, 4), np.uint64)
    for i, sd in enumerate(seeds):
      st = np.random.PCG64(np.random.SeedSequence(int(sd))).state["state"]
      words[i] = (st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)
    self.set_rng_state(words)

  def _seed_words(self, v, what, bits):
    """v -> a device tensor [N] whose bytes are the values mod 2^bits (int64 for 64, int32 for 32): a device tensor stays on the
    device, a host int (every env the same) or array is uploaded once."""
    dt, ndt, udt = (torch.int64, np.int64, np.uint64) if bits == 64 else (torch.int32, np.int32, np.uint32)
    if torch.is_tensor(v):
      t = v.reshape(-1)
      if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise TypeError("%s must be integers" % what)
      if bits == 32 and t.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        t = t.to(torch.int64) & 0xFFFFFFFF
        t = (t - ((t >> 31) << 32)).to(torch.int32)              # the low 32 bits as the int32 with the same bytes
      elif t.dtype != dt:
        t = t.view(dt) if t.dtype.itemsize == dt.itemsize else t.to(dt)
      t = t.to(self.device).contiguous()
    else:
      a = np.asarray(v, dtype=object).reshape(-1)
      if a.size == 1:
        a = np.repeat(a, self.n_envs)
      a = np.array([int(x) & ((1 << bits) - 1) for x in a], dtype=udt).view(ndt)
      t = torch.from_numpy(a).to(self.device)
    if t.numel() != self.n_envs:
      raise ValueError("%s must have n_envs entries" % what)
    return t

  def seed_rng(self, seeds=None, base=0, layout_seeds=None, mask=None, low32=False):
    """The env generators seeded on the device (sgw_seed_rng): one launch on the current stream, no synchronisation.  Env i
    gets Generator(PCG64(SeedSequence(s_i))) with s_i = seeds[i], or base + global env id with seeds=None; low32: s_i & 0xFFFFFFFF
    first (the reference's reset(seed=)); layout_seeds: s_i = crc32(be32(s_i) + be32(layout_seeds[i]) + be32(17122023)), the
    reference's stream of a new env layout.  mask [N]: only those envs, the others keep every byte of their state (the
    generators must have been set before).  seeds / layout_seeds / mask: device tensors, or host ints / arrays (uploaded once)."""
    keep = []
    sptr = lptr = mptr = None
    if seeds is not None:
      keep.append(self._seed_words(seeds, "seeds", 64)); sptr = keep[-1].data_ptr()
    if layout_seeds is not None:
      keep.append(self._seed_words(layout_seeds, "layout_seeds", 32)); lptr = keep[-1].data_ptr()
    if mask is not None:
      mask = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).contiguous()
      if mask.numel() != self.n_envs:
        raise ValueError("mask must have n_envs entries")
      mptr = mask.data_ptr()
    N.check(self._lib.sgw_seed_rng(self._h, sptr, int(base) & ((1 << 64) - 1), lptr, mptr, N.SEED_LOW32 if low32 else 0, self._stream()),
            "sgw_seed_rng")

  def set_rng_state(self, words):
    """uint64 [N, 4] = PCG64 (state_hi, state_lo, inc_hi, inc_lo) per env."""
    t = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)).to(self.device)
    N.check(self._lib.sgw_set_rng_state(self._h, t.data_ptr()), "sgw_set_rng_state")

  def _view_flags(self, agent_flags):
    if not self.spec.rotating_views:
      return None
    return self._latest("agent_flags", agent_flags, "agent views").data_ptr()

  def agent_views(self, board=None, agent_pos=None, outside_chr=None, agent_flags=None, out=None):
    """Agent-centric windows (safety_game_moma.py:1996-2101): list of uint8 [N, h_a, w_a] tensors, one per agent
    (rotated by the agent's observation direction when the env's observation_direction_mode is not 0).  `out`: a uint8
    [N, sgw_view_bytes] buffer to write into (a caller that steps in a loop reuses one buffer and its views)."""
    board = self._latest("board", board, "agent_views")
    agent_pos = self._latest("agent_pos", agent_pos, "agent_views")
    outside_chr = outside_chr or self.spec.what_lies_outside or '#'
    views = torch.empty((self.n_envs, self.view_bytes), dtype=torch.uint8, device=self.device) if out is None else out
    N.check(self._lib.sgw_agent_views(self._h, board.data_ptr(), agent_pos.data_ptr(), self._view_flags(agent_flags),
                                      ord(outside_chr), views.data_ptr(), self._stream()), "sgw_agent_views")
    return self.split_views(views)

  def split_views(self, views, L=None):
    """[..., view_bytes] tensor (the `views` / `obs_views` output) -> list over agents of [..., h_a, w_a] views of it; with L a
    [..., L * view_bytes] tensor of per-agent layer cubes -> [..., L, h_a, w_a] views."""
    out, off = [], 0
    for (h, w) in self.spec.view_shapes:
      size = (L or 1) * h * w
      out.append(views[..., off:off + size].reshape(views.shape[:-1] + ((h, w) if L is None else (L, h, w))))
      off += size
    return out

  def agent_layer_views(self, layers=None, agent_pos=None, outside_chr=None, agent_flags=None):
    """Per-agent crops of every observation layer (safety_game_moma.py:430-525): list over agents of uint8
    [N, L, h_a, w_a] tensors -- the per-agent layer cube the Zoo wrapper exposes."""
    sp = self.spec
    if layers is None:
      layers = self.observe_layers()
    agent_pos = self._latest("agent_pos", agent_pos, "agent_layer_views")
    outside_chr = outside_chr or sp.what_lies_outside or '#'
    L = len(sp.layer_chars)
    chars = self._layer_tables()[0]
    out = torch.empty((self.n_envs, self.view_bytes * L), dtype=torch.uint8, device=self.device)
    N.check(self._lib.sgw_agent_layer_views(self._h, layers.data_ptr(), agent_pos.data_ptr(), self._view_flags(agent_flags), chars.data_ptr(), L,
                                            ord(outside_chr), out.data_ptr(), self._stream()), "sgw_agent_layer_views")
    return self.split_views(out, L)

  def _coords_buffers(self, what, lead, cap, out):
    """(counts int32 lead, coords int16 lead + (cap, 2)) on this engine's device: the caller's `out` pair checked, or fresh zeros."""
    if out is None:
      return (torch.zeros(lead, dtype=torch.int32, device=self.device),
              torch.zeros(lead + (cap, 2), dtype=torch.int16, device=self.device))
    counts, coords = out
    for i, (t, dt, shp) in enumerate(((counts, torch.int32, lead), (coords, torch.int16, lead + (cap, 2)))):
      _require(what, "out[%d]" % i, t, self.device, dt, None, str(list(shp)), shape=shp)
    return counts, coords

  def layer_coords(self, layers=None, cap=None, out=None):
    """Object coordinates of every observation layer (info_observation_coordinates, safety_game_mo.py:422-457): (counts int32
    [N, L], coords int16 [N, L, cap, 2]); coords[n, l, :min(counts[n, l], cap)] are the (row, col) of layer l's set cells in
    np.argwhere order.  counts is the true number of set cells even above `cap`; the entries past it are NOT written by the launch
    (zeros in a fresh pair, the caller's bytes in `out`).  layers: uint8 [N, L, H, W] on the device (None: observe_layers());
    cap=None: H*W, which is lossless; out: a (counts, coords) pair to write into."""
    sp = self.spec
    if layers is None:
      layers = self.observe_layers()
    HW = sp.H * sp.W
    _require("layer_coords", "layers", layers, self.device, torch.uint8, None, "[N, L, H, W]", contiguous=False,
             also=lambda t: t.dim() >= 2 and t.shape[0] == self.n_envs and not t[0].numel() % HW)
    layers = layers.contiguous()
    L = layers[0].numel() // HW
    cap = HW if cap is None else int(cap)
    counts, coords = self._coords_buffers("layer_coords", (self.n_envs, L), cap, out)
    N.check(self._lib.sgw_layer_coords(self._h, layers.data_ptr(), L, cap, counts.data_ptr(), coords.data_ptr(), self._stream()),
            "sgw_layer_coords")
    return counts, coords

  def agent_layer_index(self):
    """Per agent column of the library's layout: the index of the agent's own character in spec.layer_chars (-1: none)."""
    sp = self.spec
    chars = list(sp.agent_chars)
    idx = [-1] * N.MAX_AGENTS
    for c, q in zip(chars, sp.agent_slots):
      idx[q] = sp.layer_chars.index(c) if c in sp.layer_chars else -1
    return idx

  def agent_layer_coords(self, agent_layer_views=None, cap=None, out=None):
    """Object coordinates inside each agent's window, relative to the agent (info_agent_observation_coordinates,
    safety_game_moma.py:528-580): list over agents of (counts int32 [N, L], coords int16 [N, L, cap, 2]), views into
    [N, A, L(, cap, 2)] buffers.  coords[n, l, :min(counts[n, l], cap)] are (x - ax, y - ay), x first, of layer l's set cells in
    the agent's window in np.argwhere order, (ay, ax) being the first set cell of the agent's own layer there; counts are -1 on
    every layer of an agent that is not in its own layers (the wrappers' `[]`) and nothing is written for it.
    agent_layer_views: what agent_layer_views() returned -- the list of views of ONE [N, L * view_bytes] buffer, or that buffer
    (None: computed now); cap=None: the largest window's cell count; out: a (counts [N, A, L], coords [N, A, L, cap, 2]) pair."""
    sp = self.spec
    shapes = list(sp.view_shapes)
    if agent_layer_views is None:
      agent_layer_views = self.agent_layer_views()
    vb = _view_bytes(sp)
    if vb == 0:
      raise N.SgwError("agent_layer_coords: the spec defines no agent views")
    if torch.is_tensor(agent_layer_views):
      t = agent_layer_views
      _require("agent_layer_coords", "the buffer", t, self.device, torch.uint8, None, "[N, L * view_bytes]",
               also=lambda t: t.dim() == 2 and t.shape[0] == self.n_envs and not t.shape[1] % vb)
      L, ptr = t.shape[1] // vb, t.data_ptr()
    else:                                       # the list must be the views of one [N, L * view_bytes] buffer, agent-major
      wins = list(agent_layer_views)
      L, ptr, off = (int(wins[0].shape[1]) if wins and wins[0].dim() == 4 else 0), None, 0
      ok = len(wins) == len(shapes) and L > 0
      for t, (h, w) in zip(wins, shapes) if ok else ():
        ok = ok and t.device == self.device and t.dtype == torch.uint8 and tuple(t.shape) == (self.n_envs, L, h, w)
        if ok and h * w:
          ptr = t.data_ptr() - off if ptr is None else ptr
          ok = t.data_ptr() == ptr + off and (self.n_envs == 1 or t.stride(0) == vb * L) and t[0].is_contiguous()
        off += L * h * w
      if not ok or ptr is None:
        raise N.SgwError("agent_layer_coords: needs the uint8 windows agent_layer_views() returned (views of one [N, L * view_bytes] "
                         "buffer on %s; there is no CPU path)" % (self.device,))
    cap = max(h * w for (h, w) in shapes) if cap is None else int(cap)
    counts, coords = self._coords_buffers("agent_layer_coords", (self.n_envs, sp.A, L), cap, out)
    idx = (C.c_int32 * N.MAX_AGENTS)(*self.agent_layer_index())
    N.check(self._lib.sgw_agent_layer_coords(self._h, ptr, L, idx, cap, counts.data_ptr(), coords.data_ptr(), self._stream()),
            "sgw_agent_layer_coords")
    return [(counts[:, a], coords[:, a]) for a in range(len(shapes))]

  def log_episodes(self, log, outputs=None, step_base=0):
    """Append one record per episode that ends in the engine's current output buffers to `log` (an EpisodeLog), in (t, n) order:
    the [N_pad] buffers of a step, or the [T, N_pad] buffers of step_n / rollout / replay with write_every, row t logged as step
    `step_base + t`.  One library call (sgw_log_episodes): no host synchronisation, no allocation once the log's scratch has seen
    this T, capturable.  outputs: a {name: tensor} dict of padded [N_pad, ...] or [T, N_pad, ...] buffers to log from instead
    (e.g. kept copies of the engine's).  Every field the log keeps needs its output: SgwError otherwise.  There is no CPU path."""
    if not isinstance(log, EpisodeLog):
      raise N.SgwError("log_episodes: needs an EpisodeLog (there is no CPU path)")
    self._open("log_episodes")
    if log.n_envs != self.n_envs or log.device != self.device or log.layout != EpisodeLog.layout_of(self.spec):
      raise N.SgwError("log_episodes: the log was made for another engine (envs, device or record layout differ)")
    if outputs is None:
      bufs, out, T = self._bufs, self._out, self._T
    else:
      bufs, out = dict(outputs), N.Out()
      st = bufs.get("step_type")
      rows = st.numel() // self.spec.A if torch.is_tensor(st) else 0
      if rows < self.n_pad or rows % self.n_pad:
        raise N.SgwError("log_episodes: outputs['step_type'] must be a padded [N_pad, A] or [T, N_pad, A] buffer")
      T = rows // self.n_pad
      for name, t in bufs.items():
        if name not in N.OUT_FIELDS:
          raise KeyError("unknown output %r" % name)
        dt, row = self._row(name)
        _require("log_episodes", "outputs[%r]" % name, t, self.device, dt, rows * row, "%d-row" % rows)
        setattr(out, name, t.data_ptr())
    for f in log.fields:
      need = EpisodeLog.SOURCE.get(f)
      if need is not None and need not in bufs:
        raise N.SgwError("log_episodes: the log keeps %r, which needs the %r output" % (f, need))
    if "step_type" not in bufs:
      raise N.SgwError("log_episodes: needs the 'step_type' output")
    N.check(self._lib.sgw_log_episodes(self._h, C.byref(out), T, int(step_base), C.byref(log._struct(T)), self._stream()),
            "sgw_log_episodes")

  def observe(self, board=None, rgb=True, layer_chars=None):
    """RGB uint8 [N, 3, H, W] and/or occluded layers uint8 [N, L, H, W] of a rendered ascii board."""
    if board is None:
      board = self._bufs["board"][:self.n_envs]
    board = board.reshape(-1, self.spec.H * self.spec.W).contiguous()
    n = board.shape[0]
    assert n == self.n_envs
    out = {}
    lut = rgb_t = chars = layers = None
    if rgb:
      lut = torch.from_numpy(self.spec.rgb_lut().reshape(-1)).to(self.device)
      rgb_t = torch.empty((n, 3, self.spec.H, self.spec.W), dtype=torch.uint8, device=self.device)
      out["RGB"] = rgb_t
    if layer_chars:
      chars = torch.tensor([ord(c) for c in layer_chars], dtype=torch.uint8, device=self.device)
      layers = torch.empty((n, len(layer_chars), self.spec.H, self.spec.W), dtype=torch.uint8, device=self.device)
      out["layers"] = layers
    N.check(self._lib.sgw_observe(self._h, board.data_ptr(), lut.data_ptr() if rgb else None,
                                  rgb_t.data_ptr() if rgb else None, chars.data_ptr() if layer_chars else None,
                                  len(layer_chars) if layer_chars else 0,
                                  layers.data_ptr() if layer_chars else None, self._stream()), "sgw_observe")
    return out

  def derived_stats(self):
    """Per-step derived statistics of _process_timestep (safety_game_mo.py:1027-1084) for the last step, on device,
    in numpy's summation order: dict of float64 tensors gini_index / cumulative_gini_index / mo_variance /
    cumulative_mo_variance / average_mo_variance [N(, A)] and average_reward [N(, A), K].
    Needs the 'reward', 'cumulative' and 'frame' outputs."""
    sp = self.spec
    for k in ("reward", "cumulative", "frame"):
      if k not in self._bufs or self._T != 1:
        raise N.SgwError("derived_stats needs the 'reward', 'cumulative' and 'frame' outputs of a single step")
    stats = torch.empty((self.n_envs, sp.A, 5 + sp.K), dtype=torch.float64, device=self.device)
    N.check(self._lib.sgw_derived_stats(self._h, self._bufs["reward"].data_ptr(), self._bufs["cumulative"].data_ptr(),
                                        self._bufs["frame"].data_ptr(), self._k_agent(), stats.data_ptr(), self._stream()),
            "sgw_derived_stats")
    return _stats_dict(stats)

  # -- scalar rewards --------------------------------------------------------------------------
  def _k_agent(self):
    """The spec's reward dimensions per agent column as the HOST int32 array the library reads (built once)."""
    if self._karr is None:
      ks = self._agent_ks()
      self._karr = (C.c_int32 * N.MAX_AGENTS)(*(ks + [0] * (N.MAX_AGENTS - len(ks))))
    return self._karr

  def _sources(self, what, names, listed, T, buffers):
    """{name: data pointer} of the [T, N_pad, row] buffers of the outputs `names` that a call reads: the engine's own (which must
    then be the buffers of T rows), or the caller's `buffers`.  listed: the names as the refusal spells them."""
    if buffers is None:
      if self._T != T or any(k not in self._bufs for k in names):
        raise N.SgwError("%s(T=%d) needs the %s outputs of %s (the engine holds T=%d buffers of %s)"
                         % (what, T, listed, "a single step" if T == 1 else "a write_every call over %d steps" % T, self._T, sorted(self._bufs)))
      return {k: self._bufs[k].data_ptr() for k in names}
    if any(k not in buffers for k in names):
      raise N.SgwError("%s: buffers needs %s" % (what, listed))
    return {k: self._padded_source(k, buffers[k], T, what) for k in names}

  def _padded_source(self, name, t, T, what):
    """Data pointer of `t` as the [T, N_pad, row] buffer of output `name`: the padded buffer itself, or the [T, N, ...] view of it
    that a write_every call returned (same first byte, the padded strides)."""
    dt, row = self._row(name)
    ok = torch.is_tensor(t) and t.device == self.device and t.dtype == dt and t.dim() >= (2 if T > 1 else 1)
    if ok and T > 1:
      ok = (t.shape[0] == T and t.shape[1] in (self.n_envs, self.n_pad) and t.stride(0) == self.n_pad * row and t[0].is_contiguous()
            and t[0].numel() == t.shape[1] * row)
    elif ok:
      ok = t.is_contiguous() and t.shape[0] in (self.n_envs, self.n_pad) and t.numel() == t.shape[0] * row
    if not ok:
      raise N.SgwError("%s: buffers[%r] must be the %s [%s%d or %d, ...] output buffer of this engine on %s (there is no CPU path)"
                       % (what, name, dt, "%d, " % T if T > 1 else "", self.n_envs, self.n_pad, self.device))
    return t.data_ptr()

  def scalarise(self, T=1, buffers=None):
    """scalarise=True of the reference's multi-objective environments (_process_timestep, safety_game_mo.py:1027-1066) for the
    engine's current outputs, from ONE library call (sgw_scalarise: one launch, no synchronisation, capturable): dict of float64
    tensors "scalar_reward", "scalar_cumulative", "scalar_average", [N] (or [N, A] with several agents), [T, N(, A)] for T > 1.
    Each is the reference's Python sum() over the agent's reward dimensions -- an accumulator that starts at 0.0, one addition
    per column, left to right -- of the `reward` row, of the `cumulative` row, and of cumulative[i] / (frame + 1) (the sum of
    the quotients, not the quotient of the sum).
    T == 1 reads the [N_pad, ...] buffers of a step / reset; T > 1 the [T, N_pad, ...] buffers of step_n / rollout / replay with
    write_every.  buffers: {"reward", "cumulative", "frame"} to read instead of the engine's own, e.g. what an earlier
    write_every call returned.  The result tensors are persistent per T and rewritten by the next call: a per-step call
    allocates nothing.  Needs the 'reward', 'cumulative' and 'frame' outputs; there is no CPU path."""
    T = int(T)
    if T < 1:
      raise ValueError("scalarise: T must be >= 1")
    self._open("scalarise")
    ptr = self._sources("scalarise", ("reward", "cumulative", "frame"), "'reward', 'cumulative' and 'frame'", T, buffers)

    def make():
      A = self.spec.A
      bufs = [torch.zeros(((T, self.n_pad, A) if T > 1 else (self.n_pad, A)), dtype=torch.float64, device=self.device) for _ in range(3)]
      res = {}
      for name, b in zip(("scalar_reward", "scalar_cumulative", "scalar_average"), bufs):
        v = b[:, :self.n_envs] if T > 1 else b[:self.n_envs]
        res[name] = v[..., 0] if A == 1 else v
      return bufs, res
    bufs, res = self._persistent("scalars", T, make)
    N.check(self._lib.sgw_scalarise(self._h, ptr["reward"], ptr["cumulative"], ptr["frame"], T, self._k_agent(), bufs[0].data_ptr(),
                                    bufs[1].data_ptr(), bufs[2].data_ptr(), self._stream()), "sgw_scalarise")
    return dict(res)

  def scalarise_rows(self, rows):
    """The same left-to-right sum (sgw_scalarise) over the agents' reward dimensions of ANY float64 [N, A*K] device tensor laid
    out like the `reward` output (a last performance, a mean of performances): a new [N] (or [N, A]) tensor."""
    A, K = self.spec.A, self.spec.K
    _require("scalarise_rows", "rows", rows, self.device, torch.float64, self.n_envs * A * K, "[N, A*K]", contiguous=False)
    rows = rows.contiguous()
    out = torch.empty((self.n_envs, A), dtype=torch.float64, device=self.device)
    N.check(self._lib.sgw_scalarise(self._h, rows.data_ptr(), None, None, 1, self._k_agent(), out.data_ptr(), None, None, self._stream()),
            "sgw_scalarise")
    return out[:, 0] if A == 1 else out

  # -- learning targets ------------------------------------------------------------------------
  def td_targets(self, T, gamma, lam=None, values=None, value0=None, buffers=None, bootstrap_truncated=False, scalar=False):
    """Discounted returns-to-go and GAE(lambda) advantages of the engine's [T, N_pad, ...] buffers of a write_every call (step_n,
    rollout, replay, policy_step_n), from ONE library call (sgw_td_targets: one launch, no synchronisation, capturable), per env,
    agent and reward column, cut at episode ends by the reference's conventions (include/sgw.h spells the rule out): a FIRST row
    is an auto-reset that consumed the step slot, a DEAD row an agent that finished before the others -- neither is a transition
    (valid False, 0.0, nothing flows across); a LAST row ends the recursion, and with bootstrap_truncated=True a LAST row whose
    term_reason is MAX_STEPS bootstraps from its own value instead.
    gamma: a float or a sequence of C floats (C = K, or 1 with scalar=True, which runs over scalarise(T)["scalar_reward"], summed
    here by the same sgw_scalarise launch); lam: lambda of the advantages (None = 1.0).  values [T, N(, A)(, C)]: V(observation
    after step t), value0 [N(, A)(, C)]: V(observation before step 0) -- the caller's contiguous float64 tensors on this device;
    the returns then end on values[T-1] instead of 0.0, and with value0 the advantages are computed too.
    buffers: {"reward", "step_type"(, "term_reason" with bootstrap_truncated)} to read instead of the engine's own.
    Returns {"returns": float64 [T, N(, A), C], "advantages": the same (values and value0 given), "valid": bool [T, N(, A)]}.
    The result tensors are persistent per (T, C) and rewritten by the next call.  There is no CPU path."""
    T = int(T)
    if T < 1:
      raise ValueError("td_targets: T must be >= 1")
    self._open("td_targets")
    A, n = self.spec.A, self.n_envs
    Cn = 1 if scalar else self.spec.K
    need = ("reward", "step_type") + (("term_reason",) if bootstrap_truncated else ())
    ptr = self._sources("td_targets", need, ", ".join(repr(k) for k in need), T, buffers)
    g = [float(gamma)] * Cn if np.ndim(gamma) == 0 else [float(x) for x in gamma]
    if len(g) != Cn:
      raise ValueError("td_targets: gamma must be a float or %d floats (one per reward column)" % Cn)
    if value0 is not None and values is None:
      raise ValueError("td_targets: value0 without values")
    for name, v, numel in (("values", values, T * n * A * Cn), ("value0", value0, n * A * Cn)):
      if v is not None:
        _require("td_targets", name, v, self.device, torch.float64, numel, "%d-element" % numel)
    ret, adv, valid = self._persistent("targets", (T, Cn), lambda: (
        torch.zeros((T, n, A, Cn), dtype=torch.float64, device=self.device), torch.zeros((T, n, A, Cn), dtype=torch.float64, device=self.device),
        torch.zeros((T, n, A), dtype=torch.uint8, device=self.device)))
    reward_ptr = ptr["reward"]
    if scalar:       # scalarise(T)["scalar_reward"]: the same launch, asked for that sum alone (needs neither 'cumulative' nor 'frame')
      sr = self._persistent("targets", ("scalar_reward", T), lambda: torch.zeros((T, self.n_pad, A), dtype=torch.float64, device=self.device))
      N.check(self._lib.sgw_scalarise(self._h, reward_ptr, None, None, T, self._k_agent(), sr.data_ptr(), None, None, self._stream()),
              "sgw_scalarise")
      reward_ptr = sr.data_ptr()
    want_adv = value0 is not None
    garr = (C.c_double * Cn)(*g)
    td = N.Td(reward=reward_ptr, step_type=ptr["step_type"], term_reason=ptr.get("term_reason"),
              value=None if values is None else values.data_ptr(), value0=value0.data_ptr() if want_adv else None,
              ret=ret.data_ptr(), adv=adv.data_ptr() if want_adv else None, valid=valid.data_ptr(),
              src_rows=self.n_pad, dst_rows=n, T=T, C=Cn, flags=N.TD_BOOTSTRAP_TRUNCATED if bootstrap_truncated else 0,
              reserved_=0, lambda_=1.0 if lam is None else float(lam), gamma=garr)
    N.check(self._lib.sgw_td_targets(self._h, C.byref(td), self._stream()), "sgw_td_targets")
    res = {"returns": ret[:, :, 0] if A == 1 else ret, "valid": (valid[:, :, 0] if A == 1 else valid).view(torch.bool)}
    if want_adv:
      res["advantages"] = adv[:, :, 0] if A == 1 else adv
    return res

  # -- closed loop: table policies (policy.py) ------------------------------------------------
  def _policy_source(self, policy, what):
    """The engine's output buffer a policy reads, as its latest [N_pad, row] rows."""
    if policy.device != self.device or policy.n_envs != self.n_envs or policy.spec is not self.spec:
      raise N.SgwError("%s: the policy was built for another engine (spec, device or number of envs differ)" % what)
    if policy.source not in self._bufs:
      raise N.SgwError("%s: the policy reads the %r output, which this engine does not write (outputs=%r)" % (what, policy.source, self.outputs))
    return self._latest(policy.source, None, what)

  def act(self, policy, obs=None, out=None, t=0):
    """The actions a TablePolicy takes on `obs` (sgw_policy_act: one launch, no synchronisation): int8 [N, A].  obs: uint8
    [N or N_pad, H*W] board rows / [N or N_pad, view_bytes] window rows on this device (default: the engine's current `board` /
    `views` output).  The exploration draws are those of step policy.step + t; policy.step is not advanced.  out: an int8 [N, A]
    tensor to write into (default: a persistent buffer of the engine, rewritten by the next call)."""
    src = self._policy_source(policy, "act")
    if obs is None:
      obs = src
    else:
      self._rows_of("act", "obs", obs, torch.uint8, src.shape[-1])
    if out is None:
      if self._act_out is None:
        self._act_out = torch.zeros((self.n_envs, self.spec.A), dtype=torch.int8, device=self.device)
      out = self._act_out
    else:
      _require("act", "out", out, self.device, torch.int8, self.n_envs * self.spec.A, "[N, A]")
    if policy.beta2 is not None:       # a softmax policy (TablePolicy.set_temperature): the sampling launch
      N.check(self._lib.sgw_policy_sample(self._h, C.byref(policy.native()), float(policy.beta2), obs.data_ptr(), int(t), out.data_ptr(),
                                          self._stream()), "sgw_policy_sample")
    else:
      N.check(self._lib.sgw_policy_act(self._h, C.byref(policy.native()), obs.data_ptr(), int(t), out.data_ptr(), self._stream()),
              "sgw_policy_act")
    return out.reshape(self.n_envs, self.spec.A)

  def policy_step_n(self, policy, T, write_every=False, accumulate=False):
    """T closed-loop steps from ONE library call (sgw_policy_step_n): the policy reads what the last step (or reset) wrote, its
    actions are played by the ordinary step launch, T times, and policy.step advances by T.  Returns the last step's arrays, or
    [T, N, ...] arrays with write_every, plus "actions" int8 [T, N, A]: the tape that was played (step_n over it reproduces the
    outputs).  The buffers are persistent per (T, write_every), so from the third identical call on (T >= 8) the 2T + 1 launches
    are one graph replay; the policy's tensors are read through their pointers, so weights rewritten in place take effect.
    Source 'views' needs a spec whose step launch writes the windows itself (fused_views)."""
    return self._policy_step_n(policy, T, write_every, accumulate, False)

  def policy_rollout(self, policy, T, write_every=True, accumulate=False):
    """policy_step_n that KEEPS the observation the first action was chosen on.  With write_every the last step overwrites the
    buffer row that observation was read from, so a learner has lost O[0] by the time policy_step_n returns; here the observation
    rows are first copied (on the engine's stream) into a persistent side buffer, the call reads that buffer as its first
    observation, and it is returned as "obs0" uint8 [N, row]: the O[0] of policy_scores / policy_accumulate.  Everything else is
    policy_step_n's."""
    return self._policy_step_n(policy, T, write_every, accumulate, True)

  def _policy_step_n(self, policy, T, write_every, accumulate, keep_obs0):
    T = int(T)
    if T < 1:
      raise ValueError("policy_step_n: T must be >= 1")
    if policy.source == "views" and not fused_views(self.spec):
      raise N.SgwError("policy_step_n: this spec's windows do not come from the step launch (fused_views is false): "
                       "the closed loop over windows is not available for it")
    obs0, held = self._policy_source(policy, "policy_step_n"), self._T
    self._want_T(T, write_every)
    if self._T != held:                     # the new buffers start from the observation the envs are at
      keep, obs0 = obs0, self._policy_source(policy, "policy_step_n")
      obs0.copy_(keep)
    acts = self._persistent("tape", T, lambda: torch.zeros((T, self.n_envs, self.spec.A), dtype=torch.int8, device=self.device))
    if keep_obs0:
      side = self._obs0_side(policy)
      side.copy_(obs0)
      obs0 = side
    if policy.beta2 is not None:       # a softmax policy: the same chain with the sampling launch (a graph of its own)
      N.check(self._lib.sgw_policy_sample_step_n(self._h, C.byref(policy.native()), float(policy.beta2), obs0.data_ptr(), T, 1 if write_every else 0,
                                                 C.byref(self._out), acts.data_ptr(), 1 if accumulate else 0, self._stream()),
              "sgw_policy_sample_step_n")
    else:
      N.check(self._lib.sgw_policy_step_n(self._h, C.byref(policy.native()), obs0.data_ptr(), T, 1 if write_every else 0, C.byref(self._out),
                                          acts.data_ptr(), 1 if accumulate else 0, self._stream()), "sgw_policy_step_n")
    res = self._views()
    res["actions"] = acts
    if keep_obs0:
      res["obs0"] = obs0[:self.n_envs]
    return res

  # -- learning a table policy (csrc/sgw_learn.hpp) ---------------------------------------------
  def _obs0_side(self, policy):
    """The persistent [N_pad, row] copy of the observation a policy_rollout call started from, per source."""
    return self._persistent("obs0", policy.source, lambda: torch.zeros_like(self._policy_source(policy, "policy_step_n")))

  def _learn_observations(self, policy, T, obs0, obs, actions, what, need_actions):
    """(obs0 pointer, obs pointer or None, obs_rows, actions tensor or None) of the T + 1 observations O[0..T] a learning call
    reads: the caller's tensors, or what the last policy_rollout(policy, T) left in the engine."""
    src = self._policy_source(policy, what)
    row, n, n_pad = src.shape[-1], self.n_envs, self.n_pad
    if obs0 is None:
      if T == 0:
        obs0 = src
      else:
        obs0 = self._persistent("obs0", policy.source)
        if obs0 is None:
          raise N.SgwError("%s: no obs0: pass it, or run policy_rollout(policy, T) first" % what)
    else:
      self._rows_of(what, "obs0", obs0, torch.uint8, row)
    obs_ptr, obs_rows = None, n
    if T > 0:
      if obs is None:
        if self._T != T or policy.source not in self._bufs:
          raise N.SgwError("%s(T=%d) needs the %r output of a write_every call over %d steps (the engine holds T=%d buffers)"
                           % (what, T, policy.source, T, self._T))
        obs_ptr, obs_rows = self._bufs[policy.source].data_ptr(), n_pad
      else:
        obs_rows = self._rows_of(what, "obs", obs, torch.uint8, row, T)
        obs_ptr = obs.data_ptr()
    if actions is None and need_actions:
      actions = self._persistent("tape", T)
      if actions is None and need_actions == "required":
        raise N.SgwError("%s: no actions: pass the int8 [T, N, A] tape, or run policy_rollout(policy, T) first" % what)
    if actions is not None:
      _require(what, "actions", actions, self.device, torch.int8, T * n * self.spec.A, "[%d, %d, %d]" % (T, n, self.spec.A))
    return obs0.data_ptr(), obs_ptr, obs_rows, actions

  def policy_scores(self, policy, T=0, obs0=None, obs=None, actions=None):
    """The score vectors a TablePolicy computes on the T + 1 observations O[0..T] of a closed-loop call (sgw_policy_scores: one
    launch, no synchronisation, capturable): {"scores": float32 [T+1, N, A, n_actions], "vmax": float64 [T+1, N, A] (the score of
    the greedy action: vmax[1:] and vmax[0] are td_targets' values and value0), "chosen": float64 [T, N, A] (the score of the
    action played, with a tape)}.  obs0 uint8 [N or N_pad, row]: O[0]; obs uint8 [T, N or N_pad, row]: O[1..T]; actions int8
    [T, N, A].  Defaults: what policy_rollout(policy, T) left in the engine (T == 0: the engine's current
    observation).  The result tensors are persistent per T and rewritten by the next call.  There is no CPU path."""
    T = int(T)
    if T < 0:
      raise ValueError("policy_scores: T must be >= 0")
    self._open("policy_scores")
    p0, p1, rows, actions = self._learn_observations(policy, T, obs0, obs, actions, "policy_scores", "optional" if T > 0 else None)
    n, A = self.n_envs, self.spec.A
    scores, vmax, chosen = self._persistent("scores", (T, policy.n_actions), lambda: (
        torch.zeros((T + 1, n, A, policy.n_actions), dtype=torch.float32, device=self.device),
        torch.zeros((T + 1, n, A), dtype=torch.float64, device=self.device), torch.zeros((T, n, A), dtype=torch.float64, device=self.device)))
    want_chosen = actions is not None and T > 0
    N.check(self._lib.sgw_policy_scores(self._h, C.byref(policy.native()), p0, p1, rows, T, actions.data_ptr() if want_chosen else None,
                                        scores.data_ptr(), vmax.data_ptr(), chosen.data_ptr() if want_chosen else None, self._stream()),
            "sgw_policy_scores")
    res = {"scores": scores, "vmax": vmax}
    if want_chosen:
      res["chosen"] = chosen
    return res

  def policy_accumulate(self, policy, coef, T, obs0, obs=None, actions=None, frac_bits=24):
    """Adds the fixed-point gradient sums of T x N x A transitions into the policy's int64 accumulators (sgw_policy_accumulate: one
    launch, no synchronisation, capturable): with q = rint(coef[t, n, a] * 2^frac_bits) (saturated at +-(2^31 - 1), NaN -> 0) and
    j the action played, acc_bias[p, a, j] += q and acc_weights[p, a, c, code(o[c]), j] += q for every cell c of the observation
    the action was chosen on.  Integer sums: the same bits whatever the order, run after run.  coef: float64 [T, N, A]; obs0 / obs
    / actions as for policy_scores (None: what the last policy_rollout left).  Calls add up until policy_apply(clear=True)."""
    self._policy_accumulate(policy, coef, T, obs0, obs, actions, frac_bits, False, "policy_accumulate")

  def policy_accumulate_softmax(self, policy, coef, T, obs0, obs=None, actions=None, frac_bits=24):
    """policy_accumulate for a SOFTMAX policy (sgw_policy_accumulate_softmax: one launch, capturable): the score-function gradient.
    Per transition with action a*, and for EVERY action j, q_j = quantise(coef * ((j == a*) - pi_j)) is added to acc_bias[p, a, j]
    and to acc_weights[p, a, c, code(o[c]), j] for every cell c; pi is the policy's softmax at its temperature on the observation
    the action was chosen on (policy_probs).  Transitions with an unknown table, an action out of range or a degenerate row (a
    NaN or infinite top score) add nothing.  The true gradient of log pi carries one more factor beta2 * ln 2 = 1 / temperature:
    fold it into lr.  The arguments are policy_accumulate's; the policy must have a temperature (set_temperature)."""
    if policy.beta2 is None:
      raise N.SgwError("policy_accumulate_softmax: the policy is greedy; give it a temperature (TablePolicy.set_temperature)")
    self._policy_accumulate(policy, coef, T, obs0, obs, actions, frac_bits, True, "policy_accumulate_softmax")

  def _policy_accumulate(self, policy, coef, T, obs0, obs, actions, frac_bits, softmax, what):
    T = int(T)
    if T < 1:
      raise ValueError("%s: T must be >= 1" % what)
    self._open(what)
    frac_bits = int(frac_bits)
    if policy.acc_frac_bits is not None and policy.acc_frac_bits != frac_bits:
      raise N.SgwError("%s: the accumulators hold sums with frac_bits=%d; apply them (clear=True) before frac_bits=%d"
                       % (what, policy.acc_frac_bits, frac_bits))
    n, A = self.n_envs, self.spec.A
    _require(what, "coef", coef, self.device, torch.float64, T * n * A, "[%d, %d, %d]" % (T, n, A))
    p0, p1, rows, actions = self._learn_observations(policy, T, obs0, obs, actions, what, "required")
    if softmax:
      N.check(self._lib.sgw_policy_accumulate_softmax(self._h, C.byref(policy.native()), float(policy.beta2), p0, p1, rows, T, actions.data_ptr(),
                                                      coef.data_ptr(), frac_bits, policy.acc_weights.data_ptr(), policy.acc_bias.data_ptr(),
                                                      self._stream()), "sgw_policy_accumulate_softmax")
    else:
      N.check(self._lib.sgw_policy_accumulate(self._h, C.byref(policy.native()), p0, p1, rows, T, actions.data_ptr(), coef.data_ptr(), frac_bits,
                                              policy.acc_weights.data_ptr(), policy.acc_bias.data_ptr(), self._stream()),
              "sgw_policy_accumulate")
    policy.acc_frac_bits = frac_bits

  def policy_probs(self, policy, T=0, obs0=None, obs=None, actions=None):
    """The action probabilities of a SOFTMAX TablePolicy on the T + 1 observations O[0..T] of a closed-loop call (sgw_policy_probs:
    one launch, no synchronisation, capturable): {"probs": float32 [T+1, N, A, n_actions], "p_chosen": float64 [T, N, A] (the
    probability of the action played, with a tape)}.  The probabilities are the softmax's alone: epsilon-exploration is not folded
    in.  Arguments, defaults and the persistent result tensors are policy_scores'.  There is no CPU path."""
    T = int(T)
    if T < 0:
      raise ValueError("policy_probs: T must be >= 0")
    if policy.beta2 is None:
      raise N.SgwError("policy_probs: the policy is greedy; give it a temperature (TablePolicy.set_temperature)")
    self._open("policy_probs")
    p0, p1, rows, actions = self._learn_observations(policy, T, obs0, obs, actions, "policy_probs", "optional" if T > 0 else None)
    n, A = self.n_envs, self.spec.A
    probs, chosen = self._persistent("probs", (T, policy.n_actions), lambda: (
        torch.zeros((T + 1, n, A, policy.n_actions), dtype=torch.float32, device=self.device),
        torch.zeros((T, n, A), dtype=torch.float64, device=self.device)))
    want_chosen = actions is not None and T > 0
    N.check(self._lib.sgw_policy_probs(self._h, C.byref(policy.native()), float(policy.beta2), p0, p1, rows, T,
                                       actions.data_ptr() if want_chosen else None, probs.data_ptr(), chosen.data_ptr() if want_chosen else None,
                                       self._stream()), "sgw_policy_probs")
    res = {"probs": probs}
    if want_chosen:
      res["p_chosen"] = chosen
    return res

  def policy_apply(self, policy, lr, clear=True):
    """weights += lr * acc_weights * 2^-frac_bits (and the bias alike), in place, from ONE launch (sgw_policy_apply): per element
    w = float32(float64(w) + lr * (float64(acc) * 2^-frac_bits)); an element whose sum is 0 is not written.  frac_bits is the one
    the sums were accumulated with.  clear=True zeroes the accumulators behind the update."""
    self._open("policy_apply")
    self._policy_source(policy, "policy_apply")
    frac_bits = 24 if policy.acc_frac_bits is None else policy.acc_frac_bits
    N.check(self._lib.sgw_policy_apply(self._h, C.byref(policy.native()), float(lr), frac_bits, policy.acc_weights.data_ptr(),
                                       policy.acc_bias.data_ptr(), N.APPLY_CLEAR if clear else 0, self._stream()), "sgw_policy_apply")
    if clear:
      policy.acc_frac_bits = None

  def q_learn(self, policy, T, gamma, lr, bootstrap_truncated=False, frac_bits=24):
    """One iteration of tabular / linear Q-learning over T closed-loop steps of every env, all on the device and on one stream:
      1. policy_rollout(policy, T)                                  the epsilon-greedy rollout, O[0] kept
      2. policy_scores(T)                                           vmax[s] = max_j Q(O[s], j), chosen[t] = Q(O[t], action[t])
      3. td_targets(T, gamma, lam=0.0, values=vmax[1:], value0=vmax[0], scalar=True)
      4. delta = (advantages + vmax[:-1]) - chosen, 0 where not valid    (advantages + vmax[t] = r + gamma * max Q(O[t+1]), cut at
                                                                          episode ends; FIRST rows after an auto-reset and DEAD
                                                                          agents carry 0 and are skipped)
      5. policy_accumulate(delta)                                   the integer gradient sums
      6. policy_apply(lr)                                           weights += lr * sums
    Returns the rollout's dict with "delta" float64 [T, N, A] and "valid" bool [T, N, A] added.  There is no CPU path."""
    T = int(T)
    traj = self.policy_rollout(policy, T)
    sc = self.policy_scores(policy, T)
    vmax, chosen = sc["vmax"], sc["chosen"]
    n, A = self.n_envs, self.spec.A
    td = self.td_targets(T, gamma, lam=0.0, values=vmax[1:], value0=vmax[0], bootstrap_truncated=bootstrap_truncated, scalar=True)
    adv, valid = td["advantages"].reshape(T, n, A), td["valid"].reshape(T, n, A)
    delta = (adv + vmax[:-1]) - chosen
    delta = torch.where(valid, delta, torch.zeros((), dtype=torch.float64, device=self.device))
    self.policy_accumulate(policy, delta, T, None, frac_bits=frac_bits)
    self.policy_apply(policy, lr, clear=True)
    traj["delta"], traj["valid"] = delta, valid
    return traj

  def pg_learn(self, policy, T, gamma, lr, lam=1.0, critic=None, critic_lr=None, bootstrap_truncated=False, frac_bits=24):
    """One iteration of REINFORCE / actor-critic with a SOFTMAX table policy (set_temperature) over T closed-loop steps of every
    env, all on the device and on one stream:
      1. policy_rollout(policy, T)                                  the sampled rollout, O[0] kept
      2. with a critic (a greedy TablePolicy on the same source): policy_scores(critic, T), then
         td_targets(T, gamma, lam=lam, values=vmax[1:], value0=vmax[0], scalar=True); coef = advantages
      3. without: td_targets(T, gamma, lam=lam, scalar=True); coef = returns
      4. coef = 0 where not valid
      5. policy_accumulate_softmax(coef), policy_apply(lr)          lr carries the factor 1 / temperature of the true gradient
      6. with critic_lr: the critic takes q_learn's steps 4 to 6 on the same rollout and tape: delta = (advantages + vmax[:-1]) -
         chosen, 0 where not valid; policy_accumulate(critic, delta); policy_apply(critic, critic_lr)
    Returns the rollout's dict with "coef" float64 [T, N, A] and "valid" bool [T, N, A] added.  There is no CPU path."""
    T = int(T)
    if policy.beta2 is None:
      raise N.SgwError("pg_learn: the policy is greedy; give it a temperature (TablePolicy.set_temperature)")
    if critic is not None and (critic.beta2 is not None or critic.source != policy.source or critic is policy):
      raise N.SgwError("pg_learn: the critic must be another, greedy TablePolicy on the policy's source")
    if critic_lr is not None and critic is None:
      raise ValueError("pg_learn: critic_lr without a critic")
    traj = self.policy_rollout(policy, T)
    n, A = self.n_envs, self.spec.A
    zero = torch.zeros((), dtype=torch.float64, device=self.device)
    if critic is not None:
      sc = self.policy_scores(critic, T)
      vmax = sc["vmax"]
      td = self.td_targets(T, gamma, lam=lam, values=vmax[1:], value0=vmax[0], bootstrap_truncated=bootstrap_truncated, scalar=True)
      coef = td["advantages"].reshape(T, n, A)
    else:
      td = self.td_targets(T, gamma, lam=lam, bootstrap_truncated=bootstrap_truncated, scalar=True)
      coef = td["returns"].reshape(T, n, A)
    valid = td["valid"].reshape(T, n, A)
    coef = torch.where(valid, coef, zero)
    if critic_lr is not None:                      # before any table moves
      delta = torch.where(valid, (coef + vmax[:-1]) - sc["chosen"], zero)
    self.policy_accumulate_softmax(policy, coef, T, None, frac_bits=frac_bits)
    self.policy_apply(policy, lr, clear=True)
    if critic_lr is not None:
      self.policy_accumulate(critic, delta, T, None, frac_bits=frac_bits)
      self.policy_apply(critic, critic_lr, clear=True)
    traj["coef"], traj["valid"] = coef, valid
    return traj

  # -- what each action would do (csrc/sgw_whatif.hpp) ----------------------------------------
  def simulate_moves(self, board=None, agent_pos=None, agent_flags=None):
    """Where every action of the action set would take every agent, without playing it (sgw_simulate_moves: one launch, no
    synchronisation, capturable): dict of uint8 tensors "target_pos" [N, A, n_actions, 2], "target_tile" [N, A, n_actions] and
    "blocked" [N, A, n_actions].  `blocked` is the refusal itself (a wall, another agent, the edge of the board): the action
    mask.  `target_pos` / `target_tile` are what the reference's simulate_update reports, INCLUDING its quirk: a refused action
    reports the cell of the last action before it that passed (the agent's own cell for NOOP, which always passes).
    Inputs default to the engine's own `board`, `agent_pos` and `agent_flags` outputs as the last step or reset left them;
    board and agent_pos must be among the outputs or be passed.  The result tensors are persistent and rewritten by the next
    call.  Covered: island_navigation_ex, boat_race_ex, conveyor_belt_ex, island_navigation_ex_ma, aintelope_savanna,
    firemaker_ex_ma with noops=True; anything else raises (there is no CPU path)."""
    self._open("simulate_moves")
    b = self._latest("board", board, "simulate_moves")
    p = self._latest("agent_pos", agent_pos, "simulate_moves")
    f = self._latest("agent_flags", agent_flags, "simulate_moves", optional=True)      # (without it every action direction reads UP)
    res = self._whatif_out
    if res is None:
      lead = (self.n_envs, self.spec.A, self.spec.n_actions)
      res = self._whatif_out = {"target_pos": torch.zeros(lead + (2,), dtype=torch.uint8, device=self.device),
                                "target_tile": torch.zeros(lead, dtype=torch.uint8, device=self.device),
                                "blocked": torch.zeros(lead, dtype=torch.uint8, device=self.device)}
    N.check(self._lib.sgw_simulate_moves(self._h, b.data_ptr(), p.data_ptr(), None if f is None else f.data_ptr(),
                                         res["target_pos"].data_ptr(), res["target_tile"].data_ptr(), res["blocked"].data_ptr(),
                                         self._stream()), "sgw_simulate_moves")
    return dict(res)

  def default_tile_chars(self):
    """The table rows of fold_q_values: the spec's tile_types (the reference's TILE_TYPES, the log's columns) and then the
    agents' own characters (where NOOP lands)."""
    if self.spec.tile_types is None:
      raise N.SgwError("fold_q_values: %s has no tile types (its sprites have no simulate_update)" % self.spec.name)
    return list(self.spec.tile_types) + [c for c in self.spec.agent_chars if c not in self.spec.tile_types]

  def fold_q_values(self, q, tile_chars=None, target_tile=None):
    """q_value_per_tiletype of SafetyEnvironmentMo.step(actions, q_value_per_action) (safety_game_mo.py:838-854), batched
    (sgw_fold_q_values: one launch): per env and agent the mean of the Q-vectors of the actions that land on one tile type, the
    additions in action order.  q: [N, A, n_actions, D] (or [N, n_actions, D] with one agent) on this device; float64, or
    float32, which is widened first: the mean is then a float64 mean of the widened values, not a float32 mean.  target_tile:
    what simulate_moves returned (default: its latest result; call it first).  Returns the engine-owned
    `q_value_per_tiletype` float64 [N, A, L, D] (also an attribute, with `q_value_seen` uint8 [N, A, L] and
    `q_value_tile_chars`): rows of tile types no action reached this time keep their values, across steps, episodes and resets;
    a new tile_chars or D starts a new zeroed table.  tile_chars defaults to default_tile_chars()."""
    self._open("fold_q_values")
    A, NA = self.spec.A, self.spec.n_actions
    _require("fold_q_values", "q", q, self.device, (torch.float64, torch.float32), None, contiguous=False)
    shapes = [(self.n_envs, A, NA)] + ([(self.n_envs, NA)] if A == 1 else [])
    if q.dim() < 3 or tuple(q.shape[:-1]) not in shapes or q.shape[-1] < 1:
      raise N.SgwError("fold_q_values: q must be [N, A, n_actions, D] = [%d, %d, %d, D]" % (self.n_envs, A, NA))
    D = int(q.shape[-1])
    q = q.to(torch.float64).contiguous()
    chars = self.default_tile_chars() if tile_chars is None else list(tile_chars)
    if not 1 <= len(chars) <= 64:
      raise N.SgwError("fold_q_values: 1..64 tile characters")
    key = (tuple(chars), D)
    if self._fold_key != key:
      self._fold_key = key
      self.q_value_tile_chars = chars
      self._fold_chars = torch.tensor([ord(c) if isinstance(c, str) else int(c) for c in chars], dtype=torch.uint8, device=self.device)
      self.q_value_per_tiletype = torch.zeros((self.n_envs, A, len(chars), D), dtype=torch.float64, device=self.device)
      self.q_value_seen = torch.zeros((self.n_envs, A, len(chars)), dtype=torch.uint8, device=self.device)
    if target_tile is None:
      if self._whatif_out is None:
        raise N.SgwError("fold_q_values: call simulate_moves first (or pass target_tile)")
      target_tile = self._whatif_out["target_tile"]
    else:
      _require("fold_q_values", "target_tile", target_tile, self.device, torch.uint8, self.n_envs * A * NA, "[N, A, n_actions]")
    N.check(self._lib.sgw_fold_q_values(self._h, target_tile.data_ptr(), q.data_ptr(), D, self._fold_chars.data_ptr(), len(chars),
                                        self.q_value_per_tiletype.data_ptr(), self.q_value_seen.data_ptr(), self._stream()),
            "sgw_fold_q_values")
    return self.q_value_per_tiletype

  def _layer_tables(self):
    """(the characters of spec.layer_chars as uint8 [L] on the device, the static-layer table on the device (None where the layers
    come from the engine state), gap_index, hidden_layer): what every producer of observation layers hands the library; built once."""
    if self._layers is None:
      sp = self.spec
      chars = torch.tensor([ord(c) for c in sp.layer_chars], dtype=torch.uint8, device=self.device)
      stat = None if sp.layers_from_state else torch.from_numpy(sp.layer_static()).to(self.device)
      gap = sp.layer_chars.index(sp.what_lies_beneath) if sp.what_lies_beneath in sp.layer_chars else -1
      hidden = sp.hidden_layer_char
      self._layers = (chars, stat, gap, sp.layer_chars.index(hidden) if hidden is not None else -1)
    return self._layers

  def observe_layers(self, board=None, agent_pos=None, agent_flags=None):
    """Unoccluded per-character layers with the gap correction: uint8 [N, L, H, W], L = len(spec.layer_chars)
    (what the MO/MA envs put in observation['layers']: rendering.py:188-302, observation_distiller_ex.py:164-178)."""
    sp = self.spec
    chars, stat, gap, hidx = self._layer_tables()
    L = len(sp.layer_chars)
    out = torch.empty((self.n_envs, L, sp.H, sp.W), dtype=torch.uint8, device=self.device)
    if stat is None:                              # aintelope_savanna: drapes overlap, the board shows only the top one
      if board is not None:
        raise N.SgwError("observe_layers: this family's layers come from the engine state (current step), not from a board")
      N.check(self._lib.sgw_state_layers(self._h, chars.data_ptr(), L, 1, out.data_ptr(), self._stream()), "sgw_state_layers")
      return out
    board = self._latest("board", None, "observe_layers") if board is None else board.reshape(-1, sp.H * sp.W).contiguous()
    pp = fp = None
    if hidx >= 0:                                 # a dynamic drape that can lie under a sprite (firemaker fire)
      if agent_pos is None:
        agent_pos, agent_flags = (self._latest(k, None, "observe_layers", optional=True) for k in ("agent_pos", "agent_flags"))
      if agent_pos is None or agent_flags is None:
        raise N.SgwError("observe_layers: this family needs the 'agent_pos' and 'agent_flags' outputs")
      pp, fp = agent_pos.data_ptr(), agent_flags.data_ptr()
    N.check(self._lib.sgw_observe_layers(self._h, board.data_ptr(), chars.data_ptr(), stat.data_ptr(), L, gap,
                                         pp, fp, hidx, out.data_ptr(), self._stream()), "sgw_observe_layers")
    return out

  # -- forking ----------------------------------------------------------------------------------
  def _pair_index(self, v, what):
    """An index list of copy_envs -> a contiguous int32 tensor on this device (a host array is uploaded once)."""
    if torch.is_tensor(v):
      if v.dtype.is_floating_point or v.dtype == torch.bool:
        raise TypeError("%s must be integers" % what)
      return v.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32)).to(self.device)

  def copy_envs(self, src, src_idx=None, dst_idx=None, outputs=True):
    """Env dst_idx[i] of THIS engine becomes a bit-exact copy of env src_idx[i] of `src` (sgw_copy_envs: one launch on the current
    stream, no synchronisation, capturable): every state word -- generator streams and draw counters included -- and, with
    `outputs`, the env's row of every output both engines allocate, so this engine's current observation of the env is valid
    without a step.  src: a BatchedEngine of the same spec on this device (it may be this engine).  src_idx / dst_idx: int32 device
    tensors, or host arrays (uploaded once); None: i.  A pair with an index < 0 or >= its engine's n_envs is skipped (the mask:
    dst_idx[i] = -1), and so is a copy of an env onto itself.  The destination indices must be distinct, and within one engine no
    env may be both a source and a destination; repeated sources are fine.  outputs=True needs the plain [N_pad, ...] buffers
    of both engines (after step_n / rollout with write_every: step or reset first).
    Not copied: the episodic-return accumulators, and the engine's external inputs (set_episode_bits, set_random_stream, the
    family table): the copy draws from THIS engine's inputs, keyed by this engine's global env id or array row."""
    if not isinstance(src, BatchedEngine) or src._h is None or self._h is None:
      raise N.SgwError("copy_envs: needs two open BatchedEngines (there is no CPU path)")
    keep = []
    sptr = dptr = None
    if src_idx is not None:
      keep.append(self._pair_index(src_idx, "src_idx")); sptr = keep[-1].data_ptr()
    if dst_idx is not None:
      keep.append(self._pair_index(dst_idx, "dst_idx")); dptr = keep[-1].data_ptr()
    if len(keep) == 2 and keep[0].numel() != keep[1].numel():
      raise ValueError("src_idx and dst_idx must have the same number of entries")
    n = keep[0].numel() if keep else min(self.n_envs, src.n_envs)
    dout = sout = None
    if outputs:
      if self._T != 1 or src._T != 1:
        raise N.SgwError("copy_envs: output rows are copied between the [N_pad, ...] buffers of a single step; both engines "
                         "hold [T, N_pad, ...] buffers only after step_n / rollout / replay with write_every")
      d, sout = N.Out(), C.byref(src._out)
      for name in self.outputs:
        if name in src._bufs:
          setattr(d, name, self._bufs[name].data_ptr())
      dout = C.byref(d)
    N.check(self._lib.sgw_copy_envs(self._h, src._h, dptr, sptr, n, dout, sout, self._stream()), "sgw_copy_envs")

  def fork(self, n_envs=None, env_id_base=None, outputs=None):
    """A new engine with this engine's spec, device and (by default) env_id_base, outputs and number of envs, and the external
    inputs this one was given (set_episode_bits / set_random_stream; the family table comes from the spec): what copy.deepcopy(env)
    is to the reference, for the whole batch.  The generator families are seeded first (seed_rng()), so that every lane of the new
    engine, padding included, has a working stream.  With n_envs equal to this engine's the fork then becomes a copy of it: every
    env's state and the rows of every output both allocate (copy_envs), so stepping both with the same actions gives the same
    outputs from here on.  With another n_envs nothing is copied (fill it with copy_envs), and explicit per-env input arrays
    cannot be re-applied: ValueError."""
    n = self.n_envs if n_envs is None else int(n_envs)
    if n != self.n_envs:
      for name, (arr, _) in self._inputs.items():
        if arr is not None:
          raise ValueError("fork: the %s array has one row per env of this engine and cannot be re-applied to %d envs" % (name, n))
    new = BatchedEngine(self.spec, n, device=self.device, env_id_base=self.env_id_base if env_id_base is None else int(env_id_base),
                        outputs=self.outputs if outputs is None else outputs)
    if "episode_bits" in self._inputs:
      new.set_episode_bits(self._inputs["episode_bits"][0], seed=self._inputs["episode_bits"][1])
    if "random_stream" in self._inputs:
      new.set_random_stream(self._inputs["random_stream"][0], seed=self._inputs["random_stream"][1])
    if self.spec.family in GENERATOR_FAMILIES:
      new.seed_rng()
    if n == self.n_envs:
      new.copy_envs(self, outputs=self._T == 1)
    return new

  def _drop_lookahead(self):
    look, self._look = self._look, None
    if look is not None:
      look["engine"].close()

  def lookahead(self, actions):
    """What step(actions[b]) would return NOW, for each of B candidate action sets, without committing any of them: actions int8
    [B, N(, A)] -> {output: [B, N, ...]}.  This engine's state, output buffers and accumulators do not change.  The work is done by
    a cached fork with this engine's env_id_base and external inputs, so seeded draws are the ones a real step would take: per b
    one state-only copy_envs into the fork and one step of the fork, whose launch writes its outputs straight into entry b of the
    stacked result ([B, N_pad, ...] buffers: no copy afterwards).  The result tensors are persistent and rewritten by the next
    call with the same B."""
    actions = actions.to(device=self.device, dtype=torch.int8).contiguous()
    B = int(actions.shape[0]) if actions.dim() >= 2 else 0
    if B < 1 or actions.numel() != B * self.n_envs * self.spec.A:
      raise ValueError("lookahead: actions must be int8 [B, N] (or [B, N, A])")
    look = self._look
    if look is None:
      look = self._look = {"engine": self.fork(), "B": 0}
    eng = look["engine"]
    if look["B"] != B:
      stack = {k: torch.zeros((B, eng.n_pad) + _dtype_shape(self.spec, k)[1], dtype=_dtype_shape(self.spec, k)[0], device=self.device)
               for k in eng.outputs}
      outs = []
      for b in range(B):
        o = N.Out()
        for k, t in stack.items():
          setattr(o, k, t[b].data_ptr())
        outs.append(o)
      look.update(B=B, stack=stack, outs=outs, res={k: self._shaped(k, t[:, :self.n_envs]) for k, t in stack.items()})
    stream, per = self._stream(), self.n_envs * self.spec.A
    for b in range(B):
      eng.copy_envs(self, outputs=False)
      N.check(self._lib.sgw_step(eng._h, actions.data_ptr() + b * per, C.byref(look["outs"][b]), stream), "sgw_step")
    return dict(look["res"])

  def get_state(self):
    words = int(self._lib.sgw_state_words(self._h))
    st = torch.empty((words, self.n_pad), dtype=torch.int64, device=self.device)
    N.check(self._lib.sgw_get_state(self._h, st.data_ptr(), self._stream()), "sgw_get_state")
    return st

  def set_state(self, st):
    assert st.dtype == torch.int64 and st.is_contiguous() and st.device == self.device
    N.check(self._lib.sgw_set_state(self._h, st.data_ptr(), self._stream()), "sgw_set_state")

  def close(self):
    self._drop_lookahead()
    if self._h:
      self._lib.sgw_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass


class EngineGroup(object):
  """Several BatchedEngines on one device advanced by ONE launch per step (sgw_group_*: a heterogeneous grid, each workgroup
  runs the family body of the engine it belongs to) -- a mixed suite of env families sharded over a GPU, BASELINE config 5.
  Results are those of stepping every engine by itself; each engine keeps its own outputs, accumulators and state.

      group = EngineGroup([eng_island, eng_boat, eng_safeint])
      group.step_n([acts_island, acts_boat, acts_safeint], accumulate=True)     # int8 [T, N_m(, A_m)] each
      group.rollout(512, seed, step0=0, write_every=True)                      # one fused launch for all members
  """

  def __init__(self, engines):
    self._h = None
    self.engines = list(engines)
    if not self.engines:
      raise ValueError("EngineGroup needs at least one engine")
    self._lib = self.engines[0]._lib
    self.device = self.engines[0].device
    hs = (C.c_void_p * len(self.engines))(*[e._h for e in self.engines])
    h = C.c_void_p()
    N.check(self._lib.sgw_group_create(hs, len(self.engines), C.byref(h)), "sgw_group_create")
    self._h = h

  def _outs(self, T, write_every):
    outs = (N.Out * len(self.engines))()
    for i, e in enumerate(self.engines):
      e._want_T(T, write_every)
      for name in N.OUT_FIELDS:
        setattr(outs[i], name, getattr(e._out, name))
    return outs

  def step_n(self, actions, write_every=False, accumulate=False):
    """actions: one int8 device tensor [T, N_m(, A_m)] per member, the same T.  T launches, each over every member."""
    T = int(actions[0].shape[0])
    for e, a in zip(self.engines, actions):
      assert a.dtype == torch.int8 and a.is_contiguous() and a.device == e.device and int(a.shape[0]) == T
      assert a.numel() == T * e.n_envs * e.spec.A
    outs = self._outs(T, write_every)
    ptrs = (C.c_void_p * len(self.engines))(*[a.data_ptr() for a in actions])
    N.check(self._lib.sgw_group_step_n(self._h, ptrs, T, 1 if write_every else 0, outs, 1 if accumulate else 0,
                                       self.engines[0]._stream()), "sgw_group_step_n")
    return [e._views() for e in self.engines]

  def rollout(self, T, seed, step0=0, write_every=False, accumulate=False):
    outs = self._outs(T, write_every)
    N.check(self._lib.sgw_group_rollout(self._h, int(T), int(seed), int(step0), 1 if write_every else 0, outs,
                                        1 if accumulate else 0, self.engines[0]._stream()), "sgw_group_rollout")
    return [e._views() for e in self.engines]

  def close(self):
    if self._h:
      self._lib.sgw_group_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:
      pass
