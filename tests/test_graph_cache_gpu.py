"""The graph cache behind sgw_step_n, sgw_step_full(replay) and sgw_group_step_n (csrc/sgw_api.hip GraphCache) filled past its
entry bound: one more distinct actions buffer than the cache holds (257 / 17 / 65), three calls in a row on each -- direct
launches, capture, replay -- so that the last insertion evicts buffer 0's entry, then three more calls on buffer 0, which must
go direct, capture, replay again.  Every buffer is refilled before every call, and an engine that takes the same actions one
step at a time must agree bit for bit with the last call on every buffer, with the final state and with read_returns().
(What can go wrong here is bookkeeping -- a stale graph, a destroyed one, a wrong entry -- not arithmetic: 100 envs.  The
65 536-node bound of sgw_step_n would take hundreds of thousands of launches to reach and is checked by reading.)"""
import pytest
import torch

from ai_safety_gridworlds_amd.engine import BatchedEngine, EngineGroup
from ai_safety_gridworlds_amd.specs import make_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_ENVS = 100
OUTS = ("board", "reward", "step_type", "cumulative")
T_MIN = 8          # the smallest T that sgw_step_n / sgw_group_step_n cache


def engine(name="island_navigation_ex", **kw):
  e = BatchedEngine(make_spec(name, **kw), N_ENVS, device=DEV, outputs=OUTS)
  e.reset()
  return e


def visits(cap):
  """Buffer 0 .. cap (cap + 1 buffers: the last one evicts buffer 0's entry), then buffer 0 once more; three calls each."""
  return [b for b in list(range(cap + 1)) + [0] for _ in range(3)]


def snapshot(outs):
  return {k: outs[k].clone() for k in OUTS}


def same(got, want, what):
  for k in OUTS:
    assert torch.equal(got[k], want[k]), (what, k)


def test_step_full_cache_evicts_at_16():
  a, b = engine(), engine()
  order = visits(16)
  acts = a.fill_actions(len(order), 5).clone()                  # [calls, N]
  bufs = torch.empty((17, N_ENVS), dtype=torch.int8, device=DEV)
  last = {}
  for c, i in enumerate(order):
    bufs[i].copy_(acts[c])
    last[i] = (c, snapshot(a.step_full(bufs[i], replay=True)))
  want = [snapshot(b.step(acts[c])) for c in range(len(order))]
  torch.cuda.synchronize()
  for i, (c, got) in last.items():
    same(got, want[c], "buffer %d, call %d" % (i, c))
  assert torch.equal(a.get_state(), b.get_state())
  assert torch.equal(a.read_returns(), b.read_returns())
  a.close(); b.close()


def test_step_n_cache_evicts_at_256():
  a, b = engine(), engine()
  order = visits(256)
  acts = a.fill_actions(T_MIN * len(order), 6).clone().reshape(len(order), T_MIN, N_ENVS, 1)
  bufs = torch.empty((257, T_MIN, N_ENVS, 1), dtype=torch.int8, device=DEV)
  last = {}
  for c, i in enumerate(order):
    bufs[i].copy_(acts[c])
    last[i] = (c, snapshot(a.step_n(bufs[i], accumulate=True)))
  want = []
  for c in range(len(order)):
    for t in range(T_MIN):                                      # one step launch at a time (T = 1 is never cached), returns accumulated
      o = b.step_n(acts[c, t:t + 1], accumulate=True)
    want.append(snapshot(o))
  torch.cuda.synchronize()
  for i, (c, got) in last.items():
    same(got, want[c], "buffer %d, call %d" % (i, c))
  assert torch.equal(a.get_state(), b.get_state())
  ra, rb = a.read_returns(), b.read_returns()
  assert torch.equal(ra, rb) and float(rb[-1]) > 0
  a.close(); b.close()


def test_group_step_n_cache_evicts_at_64():
  members = [("boat_race", dict(level=0, max_iterations=10, noops=True)), ("island_navigation", dict(level=0, max_iterations=12))]
  ga, solo = [engine(n, **kw) for n, kw in members], [engine(n, **kw) for n, kw in members]
  grp = EngineGroup(ga)
  order = visits(64)
  acts = [e.fill_actions(T_MIN * len(order), 7 + m).clone().reshape(len(order), T_MIN, N_ENVS, 1) for m, e in enumerate(ga)]
  bufs = [torch.empty((65, T_MIN, N_ENVS, 1), dtype=torch.int8, device=DEV) for _ in ga]
  last = {}
  for c, i in enumerate(order):
    for m in range(2):
      bufs[m][i].copy_(acts[m][c])
    last[i] = (c, [snapshot(o) for o in grp.step_n([bufs[0][i], bufs[1][i]], accumulate=True)])
  want = []
  for c in range(len(order)):
    for t in range(T_MIN):
      o = [e.step_n(acts[m][c, t:t + 1], accumulate=True) for m, e in enumerate(solo)]
    want.append([snapshot(x) for x in o])
  torch.cuda.synchronize()
  for i, (c, got) in last.items():
    for m in range(2):
      same(got[m], want[c][m], "pair %d, call %d, member %d" % (i, c, m))
  for m in range(2):
    assert torch.equal(ga[m].get_state(), solo[m].get_state())
    ra, rb = ga[m].read_returns(), solo[m].read_returns()
    assert torch.equal(ra, rb) and float(rb[-1]) > 0
  grp.close()
  for e in ga + solo:
    e.close()
