"""sgw_log_episodes (k_episode_count / k_episode_scan / k_episode_write) against the loop `for t: for n < N: if ended: append` over
the same synthetic arrays, on engines created through the C ABI for their geometry only and never stepped.  The payloads are random
BIT patterns (a record is a copy: bytes are compared, NaNs of every kind included); the rows >= N of every source hold LAST and
payloads of their own and must never be logged.  Every destination, the counter and the scratch sit in sentinel-filled allocations
with guard bytes on both sides: entries past min(count, cap), the guards and the sources must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.specs import make_spec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
BYTE = 0xA5
ERR_ARG = -1
FIRST, MID, LAST, DEAD = 0, 1, 2, 3
FIELDS = ("env", "step", "length", "term_reason", "ret", "hidden", "metrics")
SOURCE = {"length": "frame", "term_reason": "term_reason", "ret": "cumulative", "hidden": "hidden", "metrics": "metrics"}
# boat_race: A = 1, K = 1, no metrics; island_navigation_ex's spec with 12 reward columns and its 9 metrics; island_navigation_ex_ma:
# A = 2, agents finish one by one (per-agent step types and termination reasons); firemaker_ex_ma: A = 3, one shared step type
ENGINES = [("boat_race", None), ("island_navigation_ex", 12), ("island_navigation_ex_ma", None), ("firemaker_ex_ma", None)]
SHAPES = [(n, T) for n in (1, 63, 64, 65, 100, 257, 2000) for T in (1, 2, 9)] + [(20000, 4)]     # 20 000 x 4: 1 252 tiles


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class GeometryEngine(object):
  """An engine created for its GEOMETRY only (the spec's A, K, M, family; K optionally overridden).  NEVER stepped or reset."""

  def __init__(self, name, n, K=None):
    sp = N.Spec.from_buffer_copy(bytes(make_spec(name).native))
    if K is not None:
      sp.K = K
    self.lib = N.lib()
    h = C.c_void_p()
    N.check(self.lib.sgw_create(C.byref(sp), n, 0, 0, C.byref(h)), "sgw_create")
    self.h, self.n = h, n
    self.n_pad = int(self.lib.sgw_n_pad(h))
    self.A, self.K, self.M = sp.A, sp.K, sp.M
    self.per_agent = sp.family in (N.ISLAND_NAVIGATION_EX_MA, N.AINTELOPE_SAVANNA)
    self.R = self.A if self.per_agent else 1

  def close(self):
    if self.h:
      self.lib.sgw_destroy(self.h)
      self.h = None


def _step_types(g, rng, T, pattern):
  """uint8 [T, n_pad, A]; rows >= N are LAST in every pattern."""
  n, A = g.n, g.A
  if pattern == "mixed":                      # all four values, ~13 % LAST, every agent's byte drawn on its own
    st = rng.choice(np.array([FIRST, MID, LAST, DEAD], np.uint8), size=(T, g.n_pad, A), p=[0.29, 0.29, 0.13, 0.29])
  elif pattern == "none":
    st = np.full((T, g.n_pad, A), MID, np.uint8)
  elif pattern == "all":
    st = np.full((T, g.n_pad, A), LAST, np.uint8)
    if g.per_agent:
      st[:, 1::2, 1:] = DEAD                  # LAST or DEAD: still the end for the per-agent families
  elif pattern in ("env0", "envlast"):
    st = np.full((T, g.n_pad, A), MID, np.uint8)
    st[:, 0 if pattern == "env0" else n - 1, :] = LAST
  elif pattern == "combos":                   # every (agent 0, agent 1) pair of the four values, shifted per t
    st = np.zeros((T, g.n_pad, A), np.uint8)
    idx = np.arange(g.n_pad)[None, :] + 5 * np.arange(T)[:, None]
    st[:, :, 0], st[:, :, 1] = idx % 4, (idx // 4) % 4
  else:
    raise KeyError(pattern)
  st[:, n:, :] = LAST
  return np.ascontiguousarray(st)


def _bits(rng, shape):
  return rng.integers(0, 2 ** 64, size=shape, dtype=np.uint64).view(np.float64)


class Source(object):
  """The sgw_out of T rows: numpy originals, device copies, the struct."""

  def __init__(self, g, rng, T, pattern, without=()):
    rows = (T, g.n_pad)
    self.np = {"step_type": _step_types(g, rng, T, pattern),
               "frame": rng.integers(-2 ** 31, 2 ** 31, size=rows, dtype=np.int64).astype(np.int32),
               "term_reason": rng.integers(0, 256, size=rows + (g.R,), dtype=np.int64).astype(np.uint8),
               "cumulative": _bits(rng, rows + (g.A * g.K,)), "hidden": _bits(rng, rows)}
    if g.M > 0:
      self.np["metrics"] = _bits(rng, rows + (g.M,))
    for name in without:
      self.np.pop(name, None)
    self.dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.float64 else v).to(DEV) for k, v in self.np.items()}
    self.out = N.Out()
    for k, t in self.dev.items():
      setattr(self.out, k, t.data_ptr())

  def assert_untouched(self):
    for k, t in self.dev.items():
      want = self.np[k].view(np.int64) if self.np[k].dtype == np.float64 else self.np[k]
      assert np.array_equal(t.cpu().numpy(), want), "the source %r was written" % k


def _ended(g, st):
  """bool [T, N]: the predicate of sgw_track_performance."""
  live = st[:, :g.n]
  return (live >= LAST).all(axis=2) if g.per_agent else live[:, :, 0] == LAST


def _expect(g, src, T, step_base):
  """The loop: for t: for n < N: if ended: append.  {field: array [count, ...]}"""
  ended = _ended(g, src.np["step_type"])
  ts, ns = [], []
  for t in range(T):
    for n in range(g.n):
      if ended[t, n]:
        ts.append(t)
        ns.append(n)
  ts, ns = np.array(ts, dtype=np.int64), np.array(ns, dtype=np.int64)
  rec = {"env": ns.astype(np.int32), "step": step_base + ts}
  for f, s in SOURCE.items():
    if s in src.np:
      rec[f] = src.np[s][ts, ns]                # (a gather of the rows the loop visited: a byte copy, NaN payloads included)
  return rec


def _cat(a, b):
  return {f: np.concatenate([a[f], b[f]]) for f in a}


class Guarded(object):
  def __init__(self, nbytes):
    self.nbytes = nbytes
    self.t = torch.full((GUARD + nbytes + GUARD,), BYTE, dtype=torch.uint8, device=DEV)

  @property
  def ptr(self):
    return self.t.data_ptr() + GUARD

  def body(self):
    raw = self.t.cpu().numpy()
    assert (raw[:GUARD] == BYTE).all(), "write before the allocation"
    assert (raw[GUARD + self.nbytes:] == BYTE).all(), "write past the allocation"
    return raw[GUARD:GUARD + self.nbytes]


class Log(object):
  """A caller-owned sgw_episodes: the chosen fields, the counter and exactly sgw_episode_scratch_bytes of scratch, all guarded."""

  def __init__(self, g, cap, T, fields=FIELDS):
    self.g, self.cap, self.fields = g, cap, tuple(f for f in fields if not (f == "metrics" and g.M == 0))
    self.row = {"env": 4, "step": 8, "length": 4, "term_reason": g.R, "ret": 8 * g.A * g.K, "hidden": 8, "metrics": 8 * g.M}
    self.buf = {f: Guarded(cap * self.row[f]) for f in self.fields} if cap > 0 else {}
    self.count = Guarded(8)
    self.count.t[GUARD:GUARD + 8] = 0
    nbytes = int(g.lib.sgw_episode_scratch_bytes(g.n, T))
    assert nbytes > 0
    self.scratch = Guarded(nbytes)
    self.x = N.Episodes()
    self.x.cap, self.x.count, self.x.scratch = cap, self.count.ptr, self.scratch.ptr
    for f, b in self.buf.items():
      setattr(self.x, f, b.ptr)

  def append(self, src, T, step_base=0):
    return self.g.lib.sgw_log_episodes(self.g.h, C.byref(src.out), T, step_base, C.byref(self.x), _stream())

  def read(self):
    torch.cuda.synchronize()
    self.scratch.body()
    return int(self.count.body().view(np.int64)[0]), {f: b.body() for f, b in self.buf.items()}

  def check(self, want):
    """count is the true number; records 0 .. min(count, cap) - 1 are the loop's, byte for byte; everything after is the sentinel"""
    count, got = self.read()
    total = len(want["env"])
    assert count == total, "count is the true number of ended episodes"
    m = min(total, self.cap)
    for f in self.fields:
      if self.cap == 0:
        break
      used = m * self.row[f]
      assert got[f][:used].tobytes() == np.ascontiguousarray(want[f][:m]).tobytes(), "field %r" % f
      assert (got[f][used:] == BYTE).all(), "field %r: an entry past min(count, cap) was written" % f
    return count


def _patterns(g):
  return ("mixed", "none", "all", "env0", "envlast") + (("combos",) if g.per_agent and g.A == 2 else ())


@pytest.mark.parametrize("n,T", SHAPES)
@pytest.mark.parametrize("name,K", ENGINES)
def test_log_equals_the_loop(name, K, n, T):
  rng = np.random.default_rng(100003 * len(name) + 31 * n + T)
  g = GeometryEngine(name, n, K)
  try:
    for pattern in _patterns(g):
      src = Source(g, rng, T, pattern)
      want = _expect(g, src, T, 1000)
      caps = (T * n, 7, 0) if pattern == "mixed" else (T * n,)       # lossless; small: true count, records 7.. never stored; pure counter
      for cap in caps:
        log = Log(g, cap, T)
        assert log.append(src, T, 1000) == 0, g.lib.sgw_last_error()
        count = log.check(want)
      src.assert_untouched()
      ended = _ended(g, src.np["step_type"])
      assert count == int(ended.sum())
      if pattern == "none":
        assert count == 0
      if pattern == "all":
        assert count == T * n
      if pattern in ("env0", "envlast"):
        assert count == T and (want["env"] == (0 if pattern == "env0" else n - 1)).all()
      if pattern == "mixed" and T * n >= 500:
        assert 7 < count < T * n
  finally:
    g.close()


@pytest.mark.parametrize("name,K", ENGINES)
def test_three_appending_calls_one_crossing_cap(name, K):
  n, T = 257, 2
  rng = np.random.default_rng(11)
  g = GeometryEngine(name, n, K)
  try:
    srcs = [Source(g, rng, T, "mixed") for _ in range(3)]
    wants = [_expect(g, s, T, 100 + i * T) for i, s in enumerate(srcs)]
    counts = [len(w["env"]) for w in wants]
    assert min(counts) > 8
    cap = counts[0] + counts[1] // 2                                  # the second call crosses cap in the middle of its records
    log = Log(g, cap, T)
    for i, s in enumerate(srcs):
      assert log.append(s, T, 100 + i * T) == 0, g.lib.sgw_last_error()
    assert log.check(_cat(_cat(wants[0], wants[1]), wants[2])) == sum(counts) > cap
    roomy = Log(g, 3 * T * n, T)
    for i, s in enumerate(srcs):
      assert roomy.append(s, T, 100 + i * T) == 0
      roomy.check(wants[0] if i == 0 else _cat(wants[0], wants[1]) if i == 1 else _cat(_cat(wants[0], wants[1]), wants[2]))
    for s in srcs:
      s.assert_untouched()
  finally:
    g.close()


SUBSETS = [("env",), ("step", "length"), ("ret",), ("metrics", "hidden"), ("term_reason", "env", "ret"), FIELDS]


@pytest.mark.parametrize("name,K", ENGINES)
def test_field_subsets(name, K):
  n, T = 100, 2
  rng = np.random.default_rng(5)
  g = GeometryEngine(name, n, K)
  try:
    src = Source(g, rng, T, "mixed")
    want = _expect(g, src, T, 0)
    for fields in SUBSETS:
      for cap in (T * n, 7):
        log = Log(g, cap, T, fields)
        assert log.append(src, T, 0) == 0, (fields, g.lib.sgw_last_error())
        log.check(want)
    # only the sources of the kept fields are needed: a log of env and step reads step_type alone
    bare = Source(g, rng, T, "mixed", without=("frame", "term_reason", "cumulative", "hidden", "metrics"))
    log = Log(g, T * n, T, ("env", "step"))
    assert log.append(bare, T, 3) == 0, g.lib.sgw_last_error()
    log.check(_expect(g, bare, T, 3))
  finally:
    g.close()


def test_argument_errors_write_nothing():
  n, T = 100, 2
  rng = np.random.default_rng(9)
  g = GeometryEngine("island_navigation_ex", n, 12)
  try:
    src = Source(g, rng, T, "all")
    for f, s in SOURCE.items():                                      # a destination without its source
      bare = Source(g, rng, T, "all", without=(s,))
      log = Log(g, T * n, T, ("env", f))
      assert log.append(bare, T) == ERR_ARG, f
      assert b"sgw_log_episodes" in g.lib.sgw_last_error()
      assert log.check({"env": np.zeros(0, np.int32), f: np.zeros(0, np.uint8)}) == 0
    log = Log(g, T * n, T)
    for bad_T in (0, -1):
      assert log.append(src, bad_T) == ERR_ARG
    log.x.cap = -1
    assert log.append(src, T) == ERR_ARG
    log.x.cap = T * n
    for field in ("count", "scratch"):
      keep = getattr(log.x, field)
      setattr(log.x, field, None)
      assert log.append(src, T) == ERR_ARG, field
      setattr(log.x, field, keep)
    nost = Source(g, rng, T, "all", without=("step_type",))
    assert log.append(nost, T) == ERR_ARG
    count, got = log.read()
    assert count == 0 and all((b == BYTE).all() for b in got.values()), "a refused call wrote"
    assert log.append(src, T) == 0                                   # and the same log still works
    log.check(_expect(g, src, T, 0))
  finally:
    g.close()


@pytest.mark.parametrize("name,K", ENGINES)
def test_same_inputs_give_the_same_bytes(name, K):
  n, T = 2000, 2
  rng = np.random.default_rng(21)
  g = GeometryEngine(name, n, K)
  try:
    src = Source(g, rng, T, "mixed")
    logs = [Log(g, T * n // 16, T), Log(g, T * n // 16, T)]          # a cap that overflows: the unwritten tails are compared too
    for log in logs:
      for rep in range(2):
        assert log.append(src, T, rep) == 0
    (c0, a), (c1, b) = logs[0].read(), logs[1].read()
    assert c0 == c1 > logs[0].cap
    for f in a:
      assert a[f].tobytes() == b[f].tobytes(), f
  finally:
    g.close()


def test_log_under_graph_capture():
  """Plain launches on the caller's stream: one sgw_log_episodes captured by torch.cuda.graph on a side stream and replayed twice
  appends the batch twice."""
  n, T = 257, 2
  rng = np.random.default_rng(77)
  g = GeometryEngine("island_navigation_ex_ma", n)
  try:
    src = Source(g, rng, T, "mixed")
    want = _expect(g, src, T, 40)
    log = Log(g, 2 * T * n, T)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside the capture (loads the kernels' code object)
      assert log.append(src, T, 40) == 0
    side.synchronize()
    log.check(want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      assert log.append(src, T, 40) == 0
    for b in list(log.buf.values()) + [log.count]:
      b.t.fill_(BYTE)
    log.count.t[GUARD:GUARD + 8] = 0                                  # the caller clears the log by zeroing the counter
    torch.cuda.synchronize()
    graph.replay()
    log.check(want)
    graph.replay()
    assert log.check(_cat(want, want)) == 2 * len(want["env"]) > 0
  finally:
    g.close()
