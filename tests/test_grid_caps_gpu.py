"""Every capped launch of csrc/sgw_api.hip past its first trip: one test per covered row of tests/grid_caps.py, at the row's large
shape (every stride loop runs two or three times, the last trip ragged), through the C ABI, against the same numpy statements the
one-trip tests use.  Every output is poisoned with guard bytes behind (or around) it and compared whole, bit for bit: a trip that was
skipped shows as poison, a trip that ran twice or out of place as a wrong byte or a write past the rows.

The per-env kernels (windows, coordinates) get B = 131 distinct envs repeated: the reference is computed for those and tiled.  B is
prime and no stride of these launches is a multiple of B envs (tests/test_grid_caps.py), so the env one stride earlier always holds
other content, and a trip that read or wrote another trip's env shows.  The sums of sgw_policy_accumulate mix all envs: their
reference runs on the full input."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd import philox
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec
from tests import derived_ref
from tests import grid_caps as GC
from tests import kernel_gpu_util as K
from tests import learn_ref
from tests import policy_gpu_util as U
from tests import policy_ref
from tests.test_learn_gpu import FRAC, _observations, _transition_inputs

pytestmark = pytest.mark.gpu

B = GC.B_ENVS
SENT32, SENT64 = np.float32(-777.25), np.int64(-0x5A5A5A5A5A5A5A5B)
TAIL = 16                    # sentinel elements behind every table and accumulator


def _tile(a, n):
  """The B envs of `a` repeated to n envs."""
  a = np.ascontiguousarray(a)
  return np.ascontiguousarray(np.tile(a, (-(-n // B),) + (1,) * (a.ndim - 1))[:n])


def _distinct(rows):
  rows = np.ascontiguousarray(rows).reshape(len(rows), -1)
  assert len({r.tobytes() for r in rows}) == len(rows), "two of the %d envs have the same reference row" % len(rows)


def _same(what, got, want):
  got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
  assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
  if not np.array_equal(got, want):
    bad = np.flatnonzero(got != want)
    poison = np.frombuffer(bytes([K.POISON]) * got.dtype.itemsize, got.dtype)[0]
    raise AssertionError("%s: %d of %d elements differ, first at %d (got %r, want %r); %d of them still hold the poison" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]], int((got[bad] == poison).sum())))


def _trips(id):
  r = GC.BY_ID[id]
  t = r["fn"](**r["large"])
  assert r["covered"] and t.max_trips >= 3 and t.min_trips < t.max_trips, (id, t)
  return r, t


# ---- windows ----------------------------------------------------------------------------------------------------------------------
def _window_engine(id, seed):
  r, _ = _trips(id)
  s = r["large"]
  n, H, W, radii = s["n"], s["H"], s["W"], s["radii"]
  A = len(radii)
  rng = np.random.default_rng(seed)
  g = K.GeometryEngine(H, W, A=A, radii=radii, n=n)
  assert int(g.lib.sgw_view_bytes(g.h)) == GC.view_total(radii)
  pos, fl = K.positions(rng, B, A, H, W), K.flags(rng, B, A)           # corners, edges, the centre; every direction
  assert all(rad is None or rad[0] + rad[1] == rad[2] + rad[3] for rad in radii), "square windows: rotation is on"
  return s, g, rng, pos, fl


@pytest.mark.parametrize("id", ["views_small", "views_lds"])
def test_agent_views_past_the_first_trip(id):
  s, g, rng, pos, fl = _window_engine(id, 11)
  n, H, W, radii = s["n"], s["H"], s["W"], s["radii"]
  vb = GC.view_total(radii)
  try:
    pt, ft = K.dev(_tile(pos, n)), K.dev(_tile(fl, n))
    for outside in (ord('#'), ord('W')):
      board = K.boards(rng, B, H, W)
      board[rng.random((B, H, W)) < 0.2] = outside
      want = derived_ref.views_ref(board, pos, fl, radii, outside)
      _distinct(want)
      bt = K.dev(_tile(board, n))
      out = K.Out(n, g.n_pad, vb)
      rc = g.lib.sgw_agent_views(g.h, bt.data_ptr(), pt.data_ptr(), ft.data_ptr(), outside, out.ptr, K.stream())
      assert rc == 0, g.lib.sgw_last_error()
      _same("%s outside=%d" % (id, outside), out.get(shape=(n, vb)), _tile(want, n))
  finally:
    g.close()


# (the fallback's reference takes two seconds per run -- 33 536 windows cut in numpy --, so its two conventions are two cases)
@pytest.mark.parametrize("id,outsides", [("layer_views_small", "#W"), ("layer_views_lds", "#W"), ("layer_views_wave", "#"),
                                         ("layer_views_wave", "W")])
def test_agent_layer_views_past_the_first_trip(id, outsides):
  s, g, rng, pos, fl = _window_engine(id, 12 + len(outsides))
  n, H, W, radii, L = s["n"], s["H"], s["W"], s["radii"], s["L"]
  vb = GC.view_total(radii)
  try:
    pt, ft = K.dev(_tile(pos, n)), K.dev(_tile(fl, n))
    for outside in [ord(c) for c in outsides]:
      chars = rng.permutation(128)[:L].astype(np.uint8)
      if outside not in chars:
        chars[rng.integers(L)] = outside                        # the outside character's own layer reads 1 beyond the board
      layers = (rng.random((B, L, H, W)) < 0.4).astype(np.uint8)
      want = derived_ref.layer_views_ref(layers, pos, fl, radii, chars, outside)
      _distinct(want)
      lt, ct = K.dev(_tile(layers, n)), K.dev(chars)
      out = K.Out(n, g.n_pad, L * vb)
      rc = g.lib.sgw_agent_layer_views(g.h, lt.data_ptr(), pt.data_ptr(), ft.data_ptr(), ct.data_ptr(), L, outside, out.ptr, K.stream())
      assert rc == 0, g.lib.sgw_last_error()
      _same("%s outside=%d" % (id, outside), out.get(shape=(n, L * vb)), _tile(want, n))
      del out, lt
  finally:
    g.close()


# ---- coordinates ------------------------------------------------------------------------------------------------------------------
def test_layer_coords_past_the_first_trip():
  """5 x 5 planes: a segment of 8 lanes per plane, 8 planes per wave; the lossless cap and one that truncates."""
  r, t = _trips("plane_coords")
  H, W, L = 5, 5, 9
  n = r["large"]["items"] // L
  assert t.extra["per_wave"] == 8 and r["large"]["max_cells"] == H * W and n * L == r["large"]["items"]
  rng = np.random.default_rng(13)
  planes = K.planes(rng, (B, L, H * W))
  dev = K.dev(_tile(planes, n))
  g = K.GeometryEngine(H, W, n=n)
  try:
    for cap in (H * W, 4):
      want_counts, want = K.want_global(planes, H, W, cap)
      _distinct(np.concatenate([want_counts.reshape(B, -1).astype(np.int16), want.reshape(B, -1)], axis=1))
      counts = K.Guarded(n, g.n_pad, L, np.int32)
      coords = K.Guarded(n, g.n_pad, L * cap * 2, np.int16)
      rc = g.lib.sgw_layer_coords(g.h, dev.data_ptr(), L, cap, counts.ptr, coords.ptr, K.stream())
      assert rc == 0, g.lib.sgw_last_error()
      _same("counts cap=%d" % cap, counts.get(), _tile(want_counts, n))
      _same("coords cap=%d" % cap, coords.get(), _tile(want, n))
      del coords
    assert (want_counts > 4).any(), "the small cap truncates"
  finally:
    g.close()


def test_agent_layer_coords_past_the_first_trip():
  """The agent-relative form: one 5 x 5 window, the agent's own plane in the middle of the nine; every fourth env's agent is absent."""
  r, t = _trips("plane_coords_rel")
  L, own, radii, shapes = 9, 4, [GC.R4(2)], [(5, 5)]
  n = r["large"]["items"] // L
  assert t.extra["per_wave"] == 8 and r["large"]["max_cells"] == 25 and n * L == r["large"]["items"]
  rng = np.random.default_rng(14)
  rows = K.agent_rows(rng, shapes, L, B, [own])
  flat = rows[0].reshape(B, -1)
  cap = 25
  want_counts, want = K.want_agents(rows, shapes, L, B, [own], cap)
  absent = (want_counts == -1).all(axis=(1, 2))                 # nothing is written for them: their rows are the poison, all alike
  assert absent.tolist() == [i % 4 == 3 for i in range(B)] and (want_counts[~absent] >= 0).all()
  _distinct(np.concatenate([want_counts.reshape(B, -1).astype(np.int16), want.reshape(B, -1)], axis=1)[~absent])
  dev = K.dev(_tile(flat, n))
  g = K.GeometryEngine(6, 7, A=1, radii=radii, n=n)
  try:
    assert g.lib.sgw_view_bytes(g.h) * L == flat.shape[1]
    counts = K.Guarded(n, g.n_pad, L, np.int32)
    coords = K.Guarded(n, g.n_pad, L * cap * 2, np.int16)
    idx = (C.c_int32 * N.MAX_AGENTS)(own, -1, -1, -1)
    rc = g.lib.sgw_agent_layer_coords(g.h, dev.data_ptr(), L, idx, cap, counts.ptr, coords.ptr, K.stream())
    assert rc == 0, g.lib.sgw_last_error()
    _same("relative counts", counts.get(), _tile(want_counts, n))
    _same("relative coords", coords.get(), _tile(want, n))
  finally:
    g.close()


# ---- the action tape --------------------------------------------------------------------------------------------------------------
def test_fill_actions_past_the_first_trip():
  r, _ = _trips("fill_actions")
  T, n, A = r["large"]["T"], r["large"]["n"], r["large"]["A"]
  spec = make_spec("island_navigation_ex_ma")
  assert spec.A == A
  eng = BatchedEngine(spec, n, device=K.DEV, outputs=("board", "step_type"))
  try:
    seed, step0, lo, nact = 0xC0FFEE, 1000, int(spec.action_lo), int(spec.n_actions)
    total = T * n * A
    buf = torch.full((total + K.GUARD,), K.POISON, dtype=torch.uint8, device=K.DEV)
    rc = eng._lib.sgw_fill_actions(eng._h, T, seed, step0, buf.data_ptr(), K.stream())
    assert rc == 0, eng._lib.sgw_last_error()
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[total:] == K.POISON).all(), "write past the tape"
    want = np.stack([philox.actions(seed, np.arange(n), step0 + np.arange(T), lo, nact, agent=a) for a in range(A)], axis=-1)
    assert want.shape == (T, n, A) and not (want == np.int8(K.POISON - 256)).any()
    _same("the tape", raw[:total].view(np.int8), want)
  finally:
    eng.close()


# ---- tables -----------------------------------------------------------------------------------------------------------------------
def _policy(geo, n, P, seed, mixed):
  name, kw, source = U.GEOMETRIES[geo]
  spec = make_spec(name, **kw)
  eng = BatchedEngine(spec, n, device=K.DEV, outputs=U.outputs_for(spec, source))
  pol = TablePolicy(eng, source=source, chars=list(spec.layer_chars) + [U.WIN], n_policies=P, seed=5)
  rng = np.random.default_rng(seed)
  w, b, idx = U.fill_policy(pol, rng, mixed, with_index=P > 1)
  return spec, eng, pol, rng, w, b, idx


def _guarded(host, sentinel):
  """A device copy of `host` with TAIL sentinel elements behind it: (the flat tensor, the view of the array's shape)."""
  flat = torch.full((host.size + TAIL,), sentinel.item(), dtype=torch.from_numpy(host[:0].reshape(-1)).dtype, device=K.DEV)
  flat[:host.size] = K.dev(host.reshape(-1))
  return flat, flat[:host.size].view(host.shape)


def _tail_intact(flat, size, sentinel):
  return bool((flat[size:].cpu().numpy() == sentinel).all())


def test_policy_apply_past_the_first_trip():
  r, t = _trips("policy_apply")
  g = r["large"]
  spec, eng, pol, rng, w, b, _ = _policy("firemaker_views", 1, g["P"], 15, True)
  try:
    assert w.size + b.size == t.extra["elements"] and (pol.n_codes, pol.n_actions, pol.cells) == (g["G"], g["NA"], g["C"])
    w.reshape(-1)[:4] = [-0.0, 0.0, np.inf, 1.0]
    b.reshape(-1)[:2] = [-0.0, 1.0]
    for clear, lr in ((False, 0.1), (True, -0.37)):
      acc_w = rng.integers(-2 ** 36, 2 ** 36, size=w.shape).astype(np.int64)
      acc_w[rng.random(w.shape) < 0.4] = 0
      acc_b = rng.integers(-2 ** 36, 2 ** 36, size=b.shape).astype(np.int64)
      acc_b[rng.random(b.shape) < 0.4] = 0
      acc_w.reshape(-1)[:4] = [0, 0, 7, 2 ** 53 + 1]
      acc_b.reshape(-1)[:2] = [0, -(2 ** 62)]
      acc_w.reshape(-1)[-1] = 3                                 # the last element of the last trip is live
      fw, pol.weights = _guarded(w, SENT32)
      fb, pol.bias = _guarded(b, SENT32)
      faw, aw = _guarded(acc_w, SENT64)
      fab, ab = _guarded(acc_b, SENT64)
      rc = eng._lib.sgw_policy_apply(eng._h, C.byref(pol.native()), lr, FRAC, aw.data_ptr(), ab.data_ptr(), N.APPLY_CLEAR if clear else 0, None)
      assert rc == 0, eng._lib.sgw_last_error()
      torch.cuda.synchronize()
      got_w, got_b = pol.weights.cpu().numpy(), pol.bias.cpu().numpy()
      what = "clear=%r lr=%r" % (clear, lr)
      assert learn_ref.same_f32(got_w, learn_ref.apply(w, acc_w, lr, FRAC)), what
      assert learn_ref.same_f32(got_b, learn_ref.apply(b, acc_b, lr, FRAC)), what
      still = acc_w == 0
      assert np.array_equal(got_w.view(np.uint32)[still], w.view(np.uint32)[still]), "untouched elements keep their bytes"
      assert np.array_equal(aw.cpu().numpy(), np.zeros_like(acc_w) if clear else acc_w), what
      assert np.array_equal(ab.cpu().numpy(), np.zeros_like(acc_b) if clear else acc_b), what
      assert _tail_intact(fw, w.size, SENT32) and _tail_intact(fb, b.size, SENT32), "write past a table"
      assert _tail_intact(faw, w.size, SENT64) and _tail_intact(fab, b.size, SENT64), "write past an accumulator"
  finally:
    eng.close()


@pytest.mark.parametrize("id", ["accumulate_lds_one_slice", "accumulate_lds_sliced_window", "accumulate_global_atomics"])
def test_policy_accumulate_past_the_first_trip(id):
  """Two calls into the same non-zero accumulators: padded rows with the bias, then plain rows (where sgw.h takes them: row blocks
  of a multiple of 16 bytes) without it.  The out-of-range actions and the special coefficients of the one-trip test are in."""
  r, t = _trips(id)
  g = r["large"]
  n, T, P = g["n"], g["T"], g["P"]
  spec, eng, pol, rng, w, b, idx = _policy(r["geo"], n, P, 16 + P, False)
  try:
    c_a, off_a, row = policy_ref.geometry(spec, pol.source)
    assert (row, list(c_a), pol.n_codes, pol.n_actions) == (g["row_bytes"], list(g["c_a"]), g["G"], g["NA"])
    A, NA, n_pad, lo = spec.A, pol.n_actions, eng.n_pad, pol.action_lo
    code_of = pol.code_of.cpu().numpy()
    want_w = rng.integers(-2 ** 40, 2 ** 40, size=w.shape).astype(np.int64)          # the accumulators start non-zero
    want_b = rng.integers(-2 ** 40, 2 ** 40, size=b.shape).astype(np.int64)
    faw, acc_w = _guarded(want_w, SENT64)
    fab, acc_b = _guarded(want_b, SENT64)
    drawn, layouts = 0, []
    for with_bias in (True, False):
      plain = not with_bias and (n * row) % 16 == 0
      rows = n if plain else n_pad
      O = _observations(rng, spec, T + 1, rows, n, row)
      actions, coef = _transition_inputs(rng, drawn, T, n, A, NA, lo)
      drawn += actions.size
      obs0, obs, acts, cf = K.dev(O[0]), K.dev(O[1:]), K.dev(actions), K.dev(coef)
      rc = eng._lib.sgw_policy_accumulate(eng._h, C.byref(pol.native()), obs0.data_ptr(), obs.data_ptr(), rows, T, acts.data_ptr(),
                                          cf.data_ptr(), FRAC, acc_w.data_ptr(), acc_b.data_ptr() if with_bias else None, None)
      assert rc == 0, eng._lib.sgw_last_error()
      live = learn_ref.accumulate(want_w, want_b if with_bias else None, O[:, :n], code_of, idx, c_a, off_a, actions, coef, FRAC, lo)
      last_tile = n % t.extra["E"] or t.extra["E"]              # the envs of the ragged last tile, at the last step
      assert live.any() and not live.all() and live[-1, -last_tile:].any(), "the last tile adds something"
      what = "%s bias=%r %s rows" % (id, with_bias, "plain" if plain else "padded")
      _same(what + ": acc_weights", acc_w.cpu().numpy(), want_w)
      _same(what + ": acc_bias", acc_b.cpu().numpy(), want_b)
      assert _tail_intact(faw, want_w.size, SENT64) and _tail_intact(fab, want_b.size, SENT64), what + ": write past an accumulator"
      layouts.append(plain)
    assert layouts == [False, (n * row) % 16 == 0]
    assert t.extra["in_lds"] == (P == 1)
  finally:
    eng.close()
