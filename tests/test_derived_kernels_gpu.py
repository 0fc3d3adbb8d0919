"""The derived-observation kernels against the numpy references of tests/derived_ref.py (pinned to the reference's outputs
by tests/test_derived_ref.py) over the domain include/sgw.h declares, not only at the shapes the fixtures happen to have:
sgw_derived_stats for every K <= 16 and A <= 4, sgw_observe / sgw_observe_layers for boards of every H*W % 4 up to 320
cells, the three dispatch branches of sgw_agent_views / sgw_agent_layer_views, sgw_track_performance, and sgw_step_full's
fused extras on real specs.  Every element is compared bit for bit (NaN for NaN); padding rows and trailing guard bytes of
every output are poisoned and must come back untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec
from tests import derived_ref as R
from tests.kernel_gpu_util import DEV, GUARD, POISON, GeometryEngine, Out
from tests.kernel_gpu_util import boards as _boards, dev as _dev, flags as _flags, positions as _positions, stream as _stream

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -3


def _unaligned(a):
  """A device copy of uint8 `a` starting one byte past a 16-byte boundary (a caller's unaligned slice); (tensor, ptr)."""
  flat = np.ascontiguousarray(a).reshape(-1)
  t = torch.zeros(flat.size + 16, dtype=torch.uint8, device=DEV)
  t[1:1 + flat.size] = _dev(flat)
  return t, t.data_ptr() + 1


# ---- sgw_derived_stats ----------------------------------------------------------------------------------------------------
def _values(rng, cls, K):
  if cls == 0:
    return rng.integers(-50, 51, K).astype(np.float64)                      # integer-valued rewards (every real env)
  if cls == 1:
    return rng.normal(size=K) * 10.0 ** rng.uniform(-3, 6, K)
  if cls == 2:
    return np.full(K, rng.normal() * 7)                                     # all equal
  if cls == 3:
    v = np.zeros(K); v[rng.integers(K)] = rng.normal() * 100; return v      # a single nonzero
  if cls == 4:
    return -np.abs(rng.normal(size=K) * 1e3) - 1e-3                         # negative only
  if cls == 5:
    return np.where(rng.random(K) < 0.5, -0.0, 0.0)                         # signed zeros
  if cls == 6:
    return 3.0 + rng.integers(0, 2, K) * 4.440892098500626e-16              # nearly equal: mean of d ~ eps (the gini's + eps)
  if cls == 7:
    return rng.normal(size=K) * 1e160                                       # squares overflow in the variances
  return rng.normal(size=K) * 1e-3


def _stats_inputs(rng, n, A, K):
  reward = np.zeros((n, A, K))
  cumulative = np.zeros((n, A, K))
  for e in range(n):
    for a in range(A):
      reward[e, a] = _values(rng, (e + a) % 9, K)
      cumulative[e, a] = _values(rng, (e + 2 * a + 3) % 9, K)
  frame = rng.integers(0, 65536, n).astype(np.int32)
  frame[::7] = 0
  frame[1::11] = 65535
  return reward, cumulative, frame


def _run_stats(g, reward, cumulative, frame, ks, reward_ptr_offset=0):
  n, A, K = reward.shape
  r, c, f = _dev(reward), _dev(cumulative), _dev(frame)
  out = Out(n, g.n_pad, A * (5 + K) * 8)
  karr = (C.c_int32 * N.MAX_AGENTS)(*(list(ks) + [0] * (N.MAX_AGENTS - len(ks))))
  rc = g.lib.sgw_derived_stats(g.h, r.data_ptr() + reward_ptr_offset, c.data_ptr(), f.data_ptr(), karr, out.ptr, _stream())
  return rc, out


def _k_patterns(K, A):
  mixed = [K, max(1, K // 2), 1, max(1, K - 1)][:A]
  hole = [K, 0, K, K][:A] if A > 1 else [K]
  return [[K] * A, mixed, hole]


@pytest.mark.parametrize("A", [1, 2, 3, 4])
@pytest.mark.parametrize("K", list(range(1, 17)))
def test_derived_stats_every_K_and_A(K, A):
  """K * K > 128 (K >= 12) takes np_sum_c's split; A = 4 with K >= 13 needs more than 64 KiB of LDS (the cap is raised
  once per engine: the second and third calls reuse it); n = 65 leaves a ragged second wave."""
  rng = np.random.default_rng(1000 * K + A)
  n = 65
  g = GeometryEngine(6, 8, K=K, A=A, n=n)
  try:
    reward, cumulative, frame = _stats_inputs(rng, n, A, K)
    for ks in _k_patterns(K, A):
      rc, out = _run_stats(g, reward, cumulative, frame, ks)
      assert rc == 0, N.lib().sgw_last_error()
      R.assert_bits("stats K=%d A=%d k=%s" % (K, A, ks), out.get(np.float64, (n, A, 5 + K)),
                    R.stats_ref(reward, cumulative, frame, ks))
  finally:
    g.close()


@pytest.mark.parametrize("n", [1, 63, 64, 1000])
@pytest.mark.parametrize("K,A", [(16, 4), (13, 3), (12, 1), (3, 2)])
def test_derived_stats_env_counts(K, A, n):
  rng = np.random.default_rng(7 * n + K)
  g = GeometryEngine(5, 5, K=K, A=A, n=n)
  try:
    reward, cumulative, frame = _stats_inputs(rng, n, A, K)
    ks = _k_patterns(K, A)[n % 3]
    rc, out = _run_stats(g, reward, cumulative, frame, ks)
    assert rc == 0, N.lib().sgw_last_error()
    R.assert_bits("stats n=%d" % n, out.get(np.float64, (n, A, 5 + K)), R.stats_ref(reward, cumulative, frame, ks))
  finally:
    g.close()


def test_derived_stats_refuses_bad_arguments():
  """Rows move as 16-byte accesses: an 8-byte-misaligned pointer is refused; so is k_agent > K.  Nothing is written."""
  g = GeometryEngine(5, 5, K=4, A=2, n=10)
  try:
    reward, cumulative, frame = _stats_inputs(np.random.default_rng(3), 10, 2, 4)
    rc, out = _run_stats(g, reward, cumulative, frame, [4, 4], reward_ptr_offset=8)
    assert rc == ERR_ARG
    rc2, out2 = _run_stats(g, reward, cumulative, frame, [4, 5])
    assert rc2 == ERR_ARG
    for o in (out, out2):
      torch.cuda.synchronize()
      assert (o.t.cpu().numpy() == POISON).all()
  finally:
    g.close()


# ---- sgw_observe / sgw_observe_layers -------------------------------------------------------------------------------------
PLANE_SHAPES = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (3, 5), (5, 5), (6, 7), (6, 8), (7, 9), (10, 10),
                (1, 255), (255, 1), (13, 13), (17, 17), (16, 20)]


@pytest.mark.parametrize("H,W", PLANE_SHAPES)
def test_observe_rgb_and_occluded_layers(H, W):
  """RGB planes and board == char layers; n = 65 reads the boards through a pointer one byte past a 16-byte boundary.  No
  board is refused up to 32 layers (17 x 17 with 32 layers once was: plane_geom checked a reciprocal no kernel uses)."""
  HW = H * W
  rng = np.random.default_rng(H * 1000 + W)
  lut = rng.integers(0, 256, (128, 3)).astype(np.uint8)
  for n in (1, 65, 1000):
    g = GeometryEngine(H, W, n=n)
    try:
      board = _boards(rng, n, H, W)
      bt, bptr = _unaligned(board) if n == 65 else (None, None)
      if bt is None:
        bt = _dev(board); bptr = bt.data_ptr()
      lt = _dev(lut.reshape(-1))
      for L in (1, 32, 128):
        chars = rng.permutation(128)[:L].astype(np.uint8)
        ct = _dev(chars)
        rgb, lay = Out(n, g.n_pad, 3 * HW), Out(n, g.n_pad, L * HW)
        rc = g.lib.sgw_observe(g.h, bptr, lt.data_ptr(), rgb.ptr, ct.data_ptr(), L, lay.ptr, _stream())
        if rc == ERR_UNSUPPORTED:
          assert L > 32, "sgw_observe refused H*W=%d with %d layers" % (HW, L)
          continue
        assert rc == 0, N.lib().sgw_last_error()
        where = "%dx%d n=%d L=%d" % (H, W, n, L)
        R.assert_bits("rgb " + where, rgb.get(shape=(n, 3, HW)), R.rgb_ref(board.reshape(n, HW), lut))
        R.assert_bits("layers " + where, lay.get(shape=(n, L, HW)), R.occluded_layers_ref(board.reshape(n, HW), chars))
    finally:
      g.close()


@pytest.mark.parametrize("H,W", PLANE_SHAPES)
def test_observe_unoccluded_layers(H, W):
  """Static curtains, dynamic layers, the gap correction on and off, a hidden drape under agents (agent_pos / agent_flags):
  64 envs per workgroup, or 16 when H*W > 128."""
  HW = H * W
  rng = np.random.default_rng(H * 7 + W * 13)
  A = 2
  for n in (1, 65, 1000):
    g = GeometryEngine(H, W, A=A, n=n)
    try:
      for L in (1, 5, 32):
        chars = rng.permutation(128)[:L].astype(np.uint8)
        gap = int(rng.integers(L)) if L > 1 else -1
        static = rng.integers(0, 3, (L, HW)).astype(np.uint8)
        if gap >= 0:
          static[gap] = rng.integers(0, 2, HW)                    # the what_lies_beneath curtain is a static one
        board = _boards(rng, n, H, W, chars)
        pos = np.stack([rng.integers(0, H, (n, A)), rng.integers(0, W, (n, A))], -1).astype(np.uint8)
        flags = rng.integers(0, 256, (n, A)).astype(np.uint8)
        hidden = (gap + 1) % L if L > 1 else -1
        bt, bptr = _unaligned(board) if n == 65 else (None, None)
        if bt is None:
          bt = _dev(board); bptr = bt.data_ptr()
        ct, st, pt, ft = _dev(chars), _dev(static), _dev(pos), _dev(flags)
        for with_gap, with_hidden in ((True, hidden >= 0), (False, False)):
          gi = gap if with_gap else -1
          hi = hidden if with_hidden else -1
          out = Out(n, g.n_pad, L * HW)
          rc = g.lib.sgw_observe_layers(g.h, bptr, ct.data_ptr(), st.data_ptr(), L, gi, pt.data_ptr() if with_hidden else None,
                                        ft.data_ptr() if with_hidden else None, hi, out.ptr, _stream())
          assert rc == 0, N.lib().sgw_last_error()
          want = R.unoccluded_layers_ref(board, chars, static, gi, pos if with_hidden else None, flags, hi)
          R.assert_bits("layers %dx%d n=%d L=%d gap=%d hidden=%d" % (H, W, n, L, gi, hi), out.get(shape=(n, L, HW)), want)
    finally:
      g.close()


# ---- sgw_agent_views / sgw_agent_layer_views ------------------------------------------------------------------------------
SQ, ASYM = True, False
WINDOW_CASES = [
    # (H, W, radii per agent, square windows, n, layers)                      branch (sgw_agent_views / _layer_views)
    (6, 8, [(2, 2, 2, 2), (2, 2, 2, 2)], SQ, 65, (1, 9)),                       # every window <= 64 cells
    (6, 8, [(1, 3, 0, 2), (0, 4, 5, 1)], ASYM, 65, (3,)),
    (5, 5, [(2, 2, 2, 2), None, (1, 0, 3, 2), (0, 0, 0, 0)], ASYM, 65, (2,)),   # A = 4, the second agent without a view
    (3, 4, [(3, 3, 3, 3)], SQ, 1, (1,)),                                        # window (7 x 7) larger than the board
    (17, 17, [(2, 2, 2, 2), (2, 2, 2, 2), (16, 16, 16, 16)], SQ, 65, (1, 9)),   # windows > 64 cells: the LDS kernels
    (13, 13, [(10, 10, 10, 10), None], SQ, 65, (1, 4)),
    (5, 10, [(3, 6, 12, 1), (0, 0, 5, 4)], ASYM, 65, (3,)),
    (1, 255, [(2, 3, 40, 30)], ASYM, 65, (2,)),
    (17, 17, [(45, 45, 45, 45), (45, 45, 45, 45)], SQ, 20, (1,)),               # rows too large for LDS: a wave per window
    (13, 13, [(16, 16, 16, 16), (16, 16, 16, 16)], SQ, 20, (32,)),
]


@pytest.mark.parametrize("case", range(len(WINDOW_CASES)))
def test_agent_views_and_layer_cubes(case):
  H, W, radii, square, n, Ls = WINDOW_CASES[case]
  A = len(radii)
  rng = np.random.default_rng(case + 50)
  g = GeometryEngine(H, W, A=A, radii=radii, n=n)
  try:
    vb = int(g.lib.sgw_view_bytes(g.h))
    assert vb == sum((r[0] + r[1] + 1) * (r[2] + r[3] + 1) for r in radii if r is not None)
    pos = _positions(rng, n, A, H, W)
    flags = _flags(rng, n, A)
    pt, ft = _dev(pos), _dev(flags)
    for outside in (ord('#'), ord('W')):
      board = _boards(rng, n, H, W)
      board[rng.random((n, H, W)) < 0.2] = outside
      bt = _dev(board)
      for rotate in ((False, True) if square else (False,)):
        out = Out(n, g.n_pad, vb)
        rc = g.lib.sgw_agent_views(g.h, bt.data_ptr(), pt.data_ptr(), ft.data_ptr() if rotate else None, outside, out.ptr,
                                   _stream())
        assert rc == 0, N.lib().sgw_last_error()
        R.assert_bits("views case %d rotate=%d outside=%d" % (case, rotate, outside), out.get(shape=(n, vb)),
                      R.views_ref(board, pos, flags if rotate else None, radii, outside))
      for L in Ls:
        chars = rng.permutation(128)[:L].astype(np.uint8)
        chars[rng.integers(L)] = outside                        # the outside character's own layer reads 1 beyond the board
        layers = (rng.random((n, L, H, W)) < 0.4).astype(np.uint8)
        lt, ct = _dev(layers), _dev(chars)
        rotate = square
        out = Out(n, g.n_pad, L * vb)
        rc = g.lib.sgw_agent_layer_views(g.h, lt.data_ptr(), pt.data_ptr(), ft.data_ptr() if rotate else None, ct.data_ptr(), L,
                                         outside, out.ptr, _stream())
        assert rc == 0, N.lib().sgw_last_error()
        R.assert_bits("layer cubes case %d L=%d outside=%d" % (case, L, outside), out.get(shape=(n, L * vb)),
                      R.layer_views_ref(layers, pos, flags if rotate else None, radii, chars, outside))
    if not square:                                              # rotation needs square windows
      views = Out(n, g.n_pad, vb)
      assert g.lib.sgw_agent_views(g.h, bt.data_ptr(), pt.data_ptr(), ft.data_ptr(), 35, views.ptr, _stream()) == ERR_UNSUPPORTED
      lt, ct = _dev(np.zeros((n, 1, H, W), np.uint8)), _dev(np.array([35], np.uint8))
      assert g.lib.sgw_agent_layer_views(g.h, lt.data_ptr(), pt.data_ptr(), ft.data_ptr(), ct.data_ptr(), 1, 35, views.ptr,
                                         _stream()) == ERR_UNSUPPORTED
      torch.cuda.synchronize()
      assert (views.t.cpu().numpy() == POISON).all()
  finally:
    g.close()


# ---- sgw_track_performance ------------------------------------------------------------------------------------------------
PERF_SPECS = [("boat_race_ex", dict(level=3), False), ("island_navigation_ex_ma", dict(max_iterations=30), True),
              ("aintelope_savanna", dict(amount_agents=2, max_iterations=25), True)]


@pytest.mark.parametrize("env_name,kw,per_agent", PERF_SPECS)
def test_track_performance(env_name, kw, per_agent):
  """Several calls in a row (sum and count accumulate), n_cols 1 and A * K, each output pointer NULL in turn."""
  spec = make_spec(env_name, **kw)
  n, A = 77, spec.A
  eng = BatchedEngine(spec, n)
  lib = N.lib()
  rng = np.random.default_rng(len(env_name))
  try:
    for ncols in (1, A * spec.K):
      calls = [(rng.normal(size=(n, ncols)) * 10 ** rng.uniform(-2, 3), rng.integers(0, 4, (n, A)).astype(np.uint8))
               for _ in range(4)]
      for skip in (None, 0, 1, 2, 3):
        outs = [Out(n, eng.n_pad, ncols * 8), Out(n, eng.n_pad, ncols * 8), Out(n, eng.n_pad, 8), Out(n, eng.n_pad, 1)]
        init = [np.full((n, ncols), np.nan), np.zeros((n, ncols)), np.zeros(n, np.int64), None]
        for o, v in zip(outs[:3], init[:3]):
          o.t[:n * o.row_bytes] = _dev(v.reshape(-1).view(np.uint8))
        last, tot, cnt = init[0], init[1], init[2]
        for perf, st in calls:
          ptrs = [None if k == skip else outs[k].ptr for k in range(4)]
          pf, stt = _dev(perf), _dev(st)
          rc = lib.sgw_track_performance(eng._h, pf.data_ptr(), ncols, stt.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], _stream())
          assert rc == 0, lib.sgw_last_error()
          last, tot, cnt, done = R.track_performance_ref(perf, st, per_agent, last, tot, cnt)
          where = "%s cols=%d skip=%s" % (env_name, ncols, skip)
          if skip != 3:
            R.assert_bits("done " + where, outs[3].get(np.uint8, (n,)), done)
        if skip != 0:
          R.assert_bits("last " + where, outs[0].get(np.float64, (n, ncols)), last)
        if skip != 1:
          R.assert_bits("sum " + where, outs[1].get(np.float64, (n, ncols)), tot)
        if skip != 2:
          R.assert_bits("count " + where, outs[2].get(np.int64, (n,)), cnt)
        if skip is not None:
          torch.cuda.synchronize()
          o = outs[skip].t.cpu().numpy()
          assert (o[n * outs[skip].row_bytes:] == POISON).all()
  finally:
    eng.close()


# ---- sgw_step_full: k_step_extras + the chained launches on real specs --------------------------------------------------
FULL_SPECS = [
    ("island_navigation_ex", dict(level=9, max_iterations=15)),                 # 6 x 8
    ("boat_race_ex", dict(level=3, max_iterations=15)),                         # 7 x 7: H*W % 4 = 1
    ("firemaker_ex_ma", dict(amount_agents=3, max_iterations=15)),              # 17 x 17: 16 envs per workgroup, hidden fire
    ("island_navigation", dict()),                                              # the tile family (scalar, hidden performance)
    ("island_navigation_ex_ma", dict(max_iterations=15)),                       # agents finish one by one
]


@pytest.mark.parametrize("env_name,kw", FULL_SPECS)
def test_step_full_extras_match_references(env_name, kw):
  spec = make_spec(env_name, **kw)
  n, T = 100, 40
  outs = ("board", "reward", "cumulative", "frame", "step_type", "agent_pos", "agent_flags", "hidden")
  eng = BatchedEngine(spec, n, outputs=outs)
  if getattr(spec, "needs_rng", False) or spec.family == N.FIREMAKER_EX_MA:
    eng.set_rng_seeds(np.arange(n) + 11)
  eng.reset()
  views = bool(spec.view_shapes)
  acts = eng.fill_actions(T, 0xD17)
  A, K, H, W = spec.A, spec.K, spec.H, spec.W
  L = len(spec.layer_chars)
  gap = spec.layer_chars.index(spec.what_lies_beneath) if spec.what_lies_beneath in spec.layer_chars else -1
  hid = spec.layer_chars.index(spec.hidden_layer_char) if getattr(spec, "hidden_layer_char", None) else -1
  lut, static = spec.rgb_lut(), spec.layer_static()
  ks = eng._agent_ks()
  use_hidden = spec.scalar and getattr(spec, "performance", "hidden") == "hidden"
  per_agent = spec.family in (N.ISLAND_NAVIGATION_EX_MA, N.AINTELOPE_SAVANNA)
  C_ = 1 if use_hidden else A * K
  last, tot, cnt = np.full((n, C_), np.nan), np.zeros((n, C_)), np.zeros(n, np.int64)
  radii = [tuple(spec.native.view_radius[a]) if spec.native.view_radius[a][0] >= 0 else None for a in range(A)]
  rotate = spec.family != N.FIREMAKER_EX_MA or spec.rotating_views
  outside = spec.native.view_outside or ord('#')
  ended = 0
  try:
    for t in range(T):
      o = eng.step_full(acts[t], rgb=True, layers=True, stats=True, agent_layer_views=views, performance=True)
      torch.cuda.synchronize()
      g = {k: v.cpu().numpy() for k, v in o.items() if torch.is_tensor(v)}
      board = g["board"].reshape(n, H, W)
      pos, flags = g["agent_pos"].reshape(n, A, 2), g["agent_flags"].reshape(n, A)
      st = g["step_type"].reshape(n, A)
      where = "%s step %d" % (env_name, t)
      R.assert_bits("rgb " + where, g["RGB"].reshape(n, 3, H * W), R.rgb_ref(board.reshape(n, H * W), lut))
      want_layers = R.unoccluded_layers_ref(board, spec.layer_chars, static, gap, pos, flags, hid)
      R.assert_bits("layers " + where, g["layers"].reshape(n, L, H * W), want_layers)
      got_stats = np.concatenate([g[k].reshape(n, A, 1) for k in R.STATS_NAMES] + [g["average_reward"].reshape(n, A, K)], -1)
      R.assert_bits("stats " + where, got_stats, R.stats_ref(g["reward"].reshape(n, A, K), g["cumulative"].reshape(n, A, K),
                                                            g["frame"], ks))
      perf = g["hidden"].reshape(n, 1) if use_hidden else g["cumulative"].reshape(n, A * K)
      last, tot, cnt, done = R.track_performance_ref(perf, st, per_agent, last, tot, cnt)
      ended += int(done.sum())
      R.assert_bits("done " + where, g["done"].astype(np.uint8), done)
      R.assert_bits("last_performance " + where, g["last_performance"], last)
      R.assert_bits("performance_sum " + where, g["performance_sum"], tot)
      R.assert_bits("episodes " + where, g["episodes"], cnt)
      if views:
        got = np.concatenate([c.cpu().numpy().reshape(n, -1) for c in o["agent_layer_views"]], 1)
        R.assert_bits("agent layer cubes " + where, got,
                      R.layer_views_ref(want_layers.reshape(n, L, H, W), pos, flags if rotate else None, radii,
                                        spec.layer_chars, outside))
    assert ended > 0, "no episode ended: the performance bookkeeping was not exercised"
  finally:
    eng.close()
