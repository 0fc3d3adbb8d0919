"""sgw_layer_coords / sgw_agent_layer_coords (k_plane_coords) against np.argwhere per plane, on geometry-only engines created
through the C ABI and never stepped: boards of every H*W % 4 below, at and above 64 and 256 cells, windows from 3 x 3 to
33 x 33, empty / full / random planes with set bytes other than 1, a lossless cap and a small one, absent agents, argument
errors and a captured launch.  Both outputs are pre-filled with a sentinel inside poisoned allocations: every int16 past
min(count, cap), every row >= N and the guard bytes on both sides must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from tests.kernel_gpu_util import DEV, GUARD, S16, GeometryEngine, Guarded
from tests.kernel_gpu_util import agent_rows as _agent_rows, planes as _planes, stream as _stream, want_agents as _want_agents
from tests.kernel_gpu_util import want_global as _want_global

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _run_global(g, planes_dev_ptr, L, cap):
  counts = Guarded(g.n, g.n_pad, L, np.int32)
  coords = Guarded(g.n, g.n_pad, L * cap * 2, np.int16)
  rc = g.lib.sgw_layer_coords(g.h, planes_dev_ptr, L, cap, counts.ptr, coords.ptr, _stream())
  assert rc == 0, g.lib.sgw_last_error()
  return counts.get().reshape(g.n, L), coords.get().reshape(g.n, L, cap, 2)


# (H, W, L, N): H*W % 4 = 1 1 2 0 1 1 0 3; every L in {1, 9, 32} and N in {1, 63, 64, 65, 130}; 17 x 17 with L = 32 and N = 130
GLOBAL_CASES = [(3, 3, 1, 1), (3, 3, 9, 63), (5, 5, 32, 64), (5, 5, 9, 130), (6, 7, 9, 65), (6, 7, 1, 64), (8, 8, 9, 64), (8, 8, 32, 1),
                (5, 13, 9, 130), (5, 13, 32, 63), (17, 17, 32, 130), (17, 17, 1, 65), (16, 20, 9, 65), (16, 20, 32, 64), (3, 5, 9, 63),
                (3, 5, 1, 130)]


@pytest.mark.parametrize("H,W,L,n", GLOBAL_CASES)
def test_layer_coords_match_argwhere(H, W, L, n):
  rng = np.random.default_rng(1000 * H + 10 * W + L + n)
  planes = _planes(rng, (n, L, H * W))
  dev = torch.from_numpy(planes).to(DEV)
  g = GeometryEngine(H, W, n=n)
  try:
    for cap in (H * W, 4):
      counts, coords = _run_global(g, dev.data_ptr(), L, cap)
      want_counts, want = _want_global(planes, H, W, cap)
      assert np.array_equal(counts, want_counts), (cap, "counts are the true numbers of set cells")
      assert np.array_equal(coords, want), (cap, "lists in argwhere order, sentinel past min(count, cap)")
    assert L * n < 3 or (want_counts > 4).any(), "the small cap is exceeded somewhere"
  finally:
    g.close()


def test_layer_coords_from_an_unaligned_slice():
  """Planes that start one byte past a 16-byte boundary (a caller's slice): head and tail bytes of every plane load singly."""
  H, W, L, n = 5, 5, 3, 65
  rng = np.random.default_rng(5)
  planes = _planes(rng, (n, L, H * W))
  t = torch.zeros(planes.size + 16, dtype=torch.uint8, device=DEV)
  t[1:1 + planes.size] = torch.from_numpy(planes.reshape(-1)).to(DEV)
  g = GeometryEngine(H, W, n=n)
  try:
    counts, coords = _run_global(g, t.data_ptr() + 1, L, H * W)
    want_counts, want = _want_global(planes, H, W, H * W)
    assert np.array_equal(counts, want_counts) and np.array_equal(coords, want)
  finally:
    g.close()


# ---- the agent-relative form ---------------------------------------------------------------------------------------------------
R = lambda r: (r, r, r, r)
RECT = (1, 2, 3, 0)                                                   # up, down, left, right: a 4 x 4 window
# (radii per agent, L, N, agent_layer per agent)
AGENT_CASES = [([R(1)], 2, 65, [1]),
               ([R(2), RECT], 12, 63, [3, 0]),
               ([R(5), R(1), R(10)], 2, 64, [0, 1, -1]),
               ([R(16), R(2), RECT], 12, 7, [11, 5, 0]),
               ([R(10), R(16)], 2, 130, [1, 0])]


def _shapes(radii):
  return [(r[0] + r[1] + 1, r[2] + r[3] + 1) for r in radii]


def _run_agents(g, views_ptr, L, agent_layer, cap):
  A = g.A
  counts = Guarded(g.n, g.n_pad, A * L, np.int32)
  coords = Guarded(g.n, g.n_pad, A * L * cap * 2, np.int16)
  idx = (C.c_int32 * N.MAX_AGENTS)(*(list(agent_layer) + [-1] * (N.MAX_AGENTS - len(agent_layer))))
  rc = g.lib.sgw_agent_layer_coords(g.h, views_ptr, L, idx, cap, counts.ptr, coords.ptr, _stream())
  assert rc == 0, g.lib.sgw_last_error()
  return counts.get().reshape(g.n, A, L), coords.get().reshape(g.n, A, L, cap, 2)


@pytest.mark.parametrize("radii,L,n,agent_layer", AGENT_CASES)
def test_agent_layer_coords_match_the_facade_rule(radii, L, n, agent_layer):
  shapes = _shapes(radii)
  rng = np.random.default_rng(100 * len(radii) + L + n)
  rows = _agent_rows(rng, shapes, L, n, agent_layer)
  flat = np.concatenate([r.reshape(n, -1) for r in rows], axis=1)          # [N, L * view_bytes], agent-major
  dev = torch.from_numpy(np.ascontiguousarray(flat)).to(DEV)
  g = GeometryEngine(6, 7, A=len(radii), radii=radii, n=n)
  try:
    assert g.lib.sgw_view_bytes(g.h) * L == flat.shape[1]
    for cap in (max(h * w for h, w in shapes), 4):
      counts, coords = _run_agents(g, dev.data_ptr(), L, agent_layer, cap)
      want_counts, want = _want_agents(rows, shapes, L, n, agent_layer, cap)
      assert np.array_equal(counts, want_counts), cap
      assert np.array_equal(coords, want), cap
    for a in range(len(radii)):
      absent = (want_counts[:, a] == -1).all(axis=1)
      assert absent.all() if agent_layer[a] < 0 else (absent.any() == (n >= 4) and not absent.all())
  finally:
    g.close()


def test_agent_layer_coords_order_and_signs_by_hand():
  """One 3 x 3 window, agent in the first row / last column: (x - ax, y - ay), x first."""
  own = np.array([[0, 0, 7], [0, 0, 0], [0, 0, 0]], np.uint8)                  # the agent at row 0, column 2
  other = np.array([[1, 0, 0], [0, 9, 0], [0, 0, 255]], np.uint8)
  flat = np.stack([own, other]).reshape(1, -1)
  g = GeometryEngine(6, 7, A=1, radii=[R(1)], n=1)
  try:
    dev = torch.from_numpy(flat).to(DEV)
    counts, coords = _run_agents(g, dev.data_ptr(), 2, [0], 9)
    assert counts.tolist() == [[[1, 3]]]
    assert coords[0, 0, 0, :1].tolist() == [[0, 0]]
    assert coords[0, 0, 1, :3].tolist() == [[-2, 0], [-1, 1], [0, 2]]
    assert (coords[0, 0, 0, 1:] == S16).all() and (coords[0, 0, 1, 3:] == S16).all()
  finally:
    g.close()


def test_argument_errors():
  g = GeometryEngine(5, 5, n=64)
  gv = GeometryEngine(5, 5, A=1, radii=[R(1)], n=64)
  try:
    planes = torch.zeros(64 * 33 * 25, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(64 * 33, dtype=torch.int32, device=DEV)
    coords = torch.zeros(64 * 33 * 25 * 2, dtype=torch.int16, device=DEV)
    idx = (C.c_int32 * N.MAX_AGENTS)(0, -1, -1, -1)
    p, c, x = planes.data_ptr(), counts.data_ptr(), coords.data_ptr()
    for L, cap, pp, cc, xx in ((0, 25, p, c, x), (33, 25, p, c, x), (1, 0, p, c, x), (1, 25, None, c, x), (1, 25, p, None, x), (1, 25, p, c, None)):
      assert g.lib.sgw_layer_coords(g.h, pp, L, cap, cc, xx, _stream()) == ERR_ARG, (L, cap)
      assert gv.lib.sgw_agent_layer_coords(gv.h, pp, L, idx, cap, cc, xx, _stream()) == ERR_ARG, (L, cap)
    assert gv.lib.sgw_agent_layer_coords(gv.h, p, 1, None, 25, c, x, _stream()) == ERR_ARG
    assert g.lib.sgw_agent_layer_coords(g.h, p, 1, idx, 25, c, x, _stream()) == ERR_UNSUPPORTED      # no agent views in this spec
    torch.cuda.synchronize()
    assert int(counts.abs().sum()) == 0 and int(coords.abs().sum()) == 0, "a refused call wrote"
  finally:
    g.close(); gv.close()


def test_layer_coords_under_graph_capture():
  """A plain launch on the caller's stream: captured by torch.cuda.graph on a side stream (a single chain) and replayed twice
  over planes refilled in place."""
  H, W, L, n = 6, 7, 9, 65
  rng = np.random.default_rng(77)
  g = GeometryEngine(H, W, n=n)
  try:
    dev = torch.zeros((n, L, H * W), dtype=torch.uint8, device=DEV)
    counts = Guarded(n, g.n_pad, L, np.int32)
    coords = Guarded(n, g.n_pad, L * H * W * 2, np.int16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                    # warm-up outside the capture (loads the kernel's code object)
      assert g.lib.sgw_layer_coords(g.h, dev.data_ptr(), L, H * W, counts.ptr, coords.ptr, _stream()) == 0
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      assert g.lib.sgw_layer_coords(g.h, dev.data_ptr(), L, H * W, counts.ptr, coords.ptr, _stream()) == 0
    for rep in range(2):
      planes = _planes(rng, (n, L, H * W))
      dev.copy_(torch.from_numpy(planes).to(DEV))
      counts.fill(); coords.fill()
      graph.replay()
      want_counts, want = _want_global(planes, H, W, H * W)
      assert np.array_equal(counts.get().reshape(n, L), want_counts), rep
      assert np.array_equal(coords.get().reshape(n, L, H * W, 2), want), rep
  finally:
    g.close()
