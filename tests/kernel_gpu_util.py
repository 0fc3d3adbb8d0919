"""Shared by the GPU tests that call the observation kernels through the C ABI (tests/test_derived_kernels_gpu.py,
tests/test_coords_kernels_gpu.py, tests/test_grid_caps_gpu.py): geometry-only engines, poisoned outputs with guard bytes, the
position / direction mixes of the window tests, random byte planes and the np.argwhere statements of the coordinate lists."""
import ctypes as C

import numpy as np
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.specs import make_spec

DEV = "cuda:0"
GUARD = 64                   # poisoned bytes after (Out) or on both sides of (Guarded) every output
POISON = 0xA5
S16 = np.int16(-23131)       # 0xA5A5: what a poisoned int16 reads


class GeometryEngine(object):
  """An engine created through the C ABI for its GEOMETRY only: boat_race's spec with H, W, K, A, the view radii and
  start cells overridden.  The derived-observation entry points read nothing else of the engine, so these engines let the
  tests reach shapes no registered env has.  They are NEVER stepped or reset: the family's step kernel would read a board
  and tables that do not exist for that geometry."""

  def __init__(self, H, W, K=1, A=1, radii=None, n=64):
    sp = N.Spec.from_buffer_copy(bytes(make_spec("boat_race").native))
    sp.H, sp.W, sp.K, sp.A = H, W, K, A
    for a in range(N.MAX_AGENTS):
      sp.start_cell[a] = 0
      rad = radii[a] if radii is not None and a < len(radii) and radii[a] is not None else (-1, -1, -1, -1)
      for j in range(4):
        sp.view_radius[a][j] = rad[j]
      for u in range(N.MAX_K):
        sp.dim_slot[a][u] = -1
    self.H, self.W, self.K, self.A, self.n = H, W, K, A, n
    self.lib = N.lib()
    h = C.c_void_p()
    N.check(self.lib.sgw_create(C.byref(sp), n, 0, 0, C.byref(h)), "sgw_create")
    self.h = h
    self.n_pad = int(self.lib.sgw_n_pad(h))

  def close(self):
    if self.h:
      self.lib.sgw_destroy(self.h)
      self.h = None


def stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
  return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Out(object):
  """A device output of `rows` rows of `row_bytes` bytes (+ padding rows up to n_pad and GUARD bytes), all poisoned."""

  def __init__(self, rows, n_pad, row_bytes):
    self.rows, self.n_pad, self.row_bytes = rows, n_pad, row_bytes
    self.t = torch.full((n_pad * row_bytes + GUARD,), POISON, dtype=torch.uint8, device=DEV)

  @property
  def ptr(self):
    return self.t.data_ptr()

  def get(self, dtype=np.uint8, shape=None):
    """The first `rows` rows as `dtype`, after checking that nothing past them was written."""
    torch.cuda.synchronize()
    raw = self.t.cpu().numpy()
    tail = raw[self.rows * self.row_bytes:]
    assert (tail == POISON).all(), "write past the %d requested rows (first at byte %d of the tail)" % (
        self.rows, int(np.argmax(tail != POISON)))
    body = raw[:self.rows * self.row_bytes].view(dtype)
    return body.reshape(shape) if shape is not None else body


class Guarded(object):
  """`n_pad` rows of `row` elements of `dtype` between two guards, every byte the sentinel; rows >= `rows` are padding."""

  def __init__(self, rows, n_pad, row, dtype):
    self.rows, self.row, self.dtype = rows, row, np.dtype(dtype)
    self.body = n_pad * row * self.dtype.itemsize
    self.t = torch.empty(GUARD + self.body + GUARD, dtype=torch.uint8, device=DEV)
    self.fill()

  def fill(self):
    self.t.fill_(POISON)

  @property
  def ptr(self):
    return self.t.data_ptr() + GUARD

  def get(self):
    """The first `rows` rows, after checking the guards and the padding rows."""
    torch.cuda.synchronize()
    raw = self.t.cpu().numpy()
    used = self.rows * self.row * self.dtype.itemsize
    assert (raw[:GUARD] == POISON).all(), "write before the output"
    assert (raw[GUARD + used:] == POISON).all(), "write into rows >= N or past the output"
    return raw[GUARD:GUARD + used].view(self.dtype)


# ---- the window tests' inputs ----------------------------------------------------------------------------------------------------
def boards(rng, n, H, W, chars=None):
  b = rng.integers(0, 128, (n, H, W)).astype(np.uint8)
  if chars is not None:                                        # mostly the layer characters, so dynamic layers light up
    pick = np.asarray(chars, np.uint8)[rng.integers(0, len(chars), (n, H, W))]
    b = np.where(rng.random((n, H, W)) < 0.7, pick, b)
  return b


def positions(rng, n, A, H, W):
  spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H - 1, W // 2), (H // 2, W - 1),
           (H // 2, W // 2)]
  pos = np.stack([rng.integers(0, H, (n, A)), rng.integers(0, W, (n, A))], -1)
  for e in range(n):
    for a in range(A):
      if (e + a) % 3 != 2:
        pos[e, a] = spots[(e * A + a) % len(spots)]
  return pos.astype(np.uint8)


def flags(rng, n, A):
  """Every observation direction (bits 3-4) for every agent, the other bits random (they must not matter)."""
  d = (np.arange(n)[:, None] + np.arange(A)[None, :]) % 4
  return ((d << 3) | rng.integers(0, 8, (n, A)) | (rng.integers(0, 8, (n, A)) << 5)).astype(np.uint8)


# ---- the coordinate tests' inputs and their np.argwhere statements ---------------------------------------------------------------
def planes(rng, shape):
  """Random uint8 planes [..., cells]: per plane all-zero, all-set or ~0.3 dense; set bytes take values 1..255."""
  lead, cells = shape[:-1], shape[-1]
  kind = rng.integers(0, 4, lead)                                    # 0: empty, 1: full, 2-3: random
  kind.reshape(-1)[:2] = (0, 1)[:kind.size]
  dens = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, 0.3))[..., None]
  on = rng.random(lead + (cells,)) < dens
  return (on * rng.integers(1, 256, lead + (cells,))).astype(np.uint8)


def want_global(planes, H, W, cap):
  n, L = planes.shape[:2]
  counts = np.zeros((n, L), np.int32)
  coords = np.full((n, L, cap, 2), S16, np.int16)
  for i in range(n):
    for l in range(L):
      at = np.argwhere(planes[i, l].reshape(H, W))
      counts[i, l] = len(at)
      coords[i, l, :min(len(at), cap)] = at[:cap]
  return counts, coords


def agent_rows(rng, shapes, L, n, agent_layer):
  """Per env [agent][layer][h][w] rows; the agent's own plane by env: a single cell in the window's centre, in its first row /
  last column, several random cells (the first in row-major order is the centre), or empty (the agent is absent)."""
  rows = []
  for (h, w) in shapes:
    rows.append(planes(rng, (n, L, h * w)))
  for a, (h, w) in enumerate(shapes):
    own = agent_layer[a]
    if own < 0:
      continue
    for i in range(n):
      p = np.zeros(h * w, np.uint8)
      if i % 4 == 0:
        p[(h // 2) * w + w // 2] = 1
      elif i % 4 == 1:
        p[w - 1] = 200
      elif i % 4 == 2:
        p[:] = (rng.random(h * w) < 0.2) * rng.integers(1, 256, h * w)
      rows[a][i, own] = p
  return rows


def want_agents(rows, shapes, L, n, agent_layer, cap):
  A = len(shapes)
  counts = np.full((n, A, L), -1, np.int32)
  coords = np.full((n, A, L, cap, 2), S16, np.int16)
  for a, (h, w) in enumerate(shapes):
    for i in range(n):
      me = np.argwhere(rows[a][i, agent_layer[a]].reshape(h, w)) if agent_layer[a] >= 0 else []
      if len(me) == 0:
        continue                                                     # the facades' []: counts stay -1, nothing is written
      ay, ax = me[0]
      for l in range(L):
        at = np.argwhere(rows[a][i, l].reshape(h, w))
        counts[i, a, l] = len(at)
        rel = np.stack([at[:, 1] - ax, at[:, 0] - ay], axis=1) if len(at) else np.zeros((0, 2), np.int64)      # x first
        coords[i, a, l, :min(len(at), cap)] = rel[:cap]
  return counts, coords
