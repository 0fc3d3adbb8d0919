"""sgw_copy_envs on the GPU, and what engine.py builds on it (BatchedEngine.copy_envs / fork / lookahead): the row-size table
against engine._dtype_shape, a fork that stays equal to its original across episode ends, gather / scatter between engines of 130
and 70 envs against torch indexing of sgw_get_state and of the output buffers (padding rows and columns included), one engine onto
itself, the refused calls, one-step lookahead against a third engine restored from a snapshot, and the launch under graph capture.
Every comparison is of bytes (NaNs included)."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine, _dtype_shape, _view_bytes
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP

pytestmark = pytest.mark.gpu

DEV = LP.DEV
ERR_ARG = -1
LAST = 2


def same(a, b):
  """Equal byte for byte (a NaN equals itself)."""
  a, b = a.contiguous(), b.contiguous()
  return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def engine_of(row_id, n=None, seed=None):
  """(row, spec, inp, engine) of a launch_paths row, with `n` envs and the inputs of `seed` instead of the row's; not reset."""
  row = dict(LP.BY_ID[row_id])
  if n is not None:
    row["n"] = n
  spec = make_spec(row["name"], **row["kw"])
  inp = LP.inputs(row, spec, LP.ROWS.index(LP.BY_ID[row_id]) if seed is None else seed)
  return row, spec, inp, LP.make_engine(row, spec, inp)


def bufs_of(eng):
  return {k: v.clone() for k, v in eng._bufs.items()}


# ---- 1. the row-size table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", LP.ROWS, ids=[r["id"] for r in LP.ROWS])
def test_out_row_bytes_is_the_buffer_row(row):
  spec = make_spec(row["name"], **row["kw"])
  eng = BatchedEngine(spec, 64, device=DEV, outputs=("board",))
  try:
    L = eng._lib
    assert len(N.OUT_FIELDS) == 20
    for field, name in enumerate(N.OUT_FIELDS):
      dt, shp = _dtype_shape(spec, name)
      lacks = ((name == "metrics" and spec.M == 0) or (name == "safety2" and spec.family != N.AINTELOPE_SAVANNA)
               or (name in ("views", "obs_views") and _view_bytes(spec) == 0))
      want = 0 if lacks else dt.itemsize * int(np.prod(shp, dtype=np.int64))
      assert int(L.sgw_out_row_bytes(eng._h, field)) == want, (row["id"], name)
    assert L.sgw_out_row_bytes(eng._h, 20) < 0 and L.sgw_out_row_bytes(eng._h, -1) < 0
  finally:
    eng.close()


# ---- 2. a fork equals the original ------------------------------------------------------------------------------------------------
FORK_ROWS = ("island_ex_packed", "island_ex_plain", "boat_race_ex", "safe_interruptibility_ex", "tomato_crmdp", "tomato_watering",
             "firemaker_ex_ma", "island_ex_ma", "aintelope_savanna")
# tomato_watering / tomato_crmdp take no max_iterations: their episodes last 100 steps, so no episode could end inside 32 steps
# from a reset.  One fused rollout puts these two engines 80 steps into their episodes first; the 16 + 16 steps of the test are
# then steps 81 .. 112, and every env's episode ends at step 100, in the second half.
PRE_STEPS = {"tomato_watering": 80, "tomato_crmdp": 80}


FORK_SEED, FORK_AT, FORK_STEPS = 0xF0, 16, 32


def fork_stays_equal(row, eng, pre_steps=0):
  """A fresh engine of `row`: FORK_AT steps of its sgw_fill_actions stream (seed FORK_SEED), fork(), and both engines side by side to
  step FORK_STEPS, across episode ends.  Closes both; returns the fork's outputs of steps FORK_AT .. FORK_STEPS - 1 as
  {field: [steps, N, ...]}."""
  row_id = row["id"]
  fork = None
  try:
    n = row["n"]
    LP.start(eng, row)
    if pre_steps:
      eng.rollout(pre_steps, 11)
    acts = eng.fill_actions(FORK_STEPS, FORK_SEED)
    for t in range(FORK_AT):
      o = eng.step(acts[t])
    fork = eng.fork()
    assert fork.n_envs == n and fork.env_id_base == eng.env_id_base and fork.outputs == eng.outputs
    fo = fork._views()
    for k in row["outs"]:
      assert same(fo[k], o[k]), "%s: the fork's %s differs right after fork()" % (row_id, k)
    ended = False
    rec = {k: [] for k in row["outs"]}
    for t in range(FORK_AT, FORK_STEPS):
      o, fo = eng.step(acts[t]), fork.step(acts[t])
      for k in row["outs"]:
        assert same(fo[k], o[k]), "%s step %d: %s" % (row_id, t, k)
        rec[k].append(fo[k].clone())
      ended = ended or bool((o["step_type"] == LAST).any())
    assert ended, "%s: no episode ends in the second half" % row_id
    assert same(fork.get_state()[:, :n], eng.get_state()[:, :n])
    return {k: torch.stack(v) for k, v in rec.items()}
  finally:
    if fork is not None:
      fork.close()
    eng.close()


@pytest.mark.parametrize("row_id", FORK_ROWS)
def test_fork_equals_the_original(row_id):
  row, spec, inp, eng = engine_of(row_id)
  fork_stays_equal(row, eng, PRE_STEPS.get(row_id, 0))


def test_fork_to_another_size_refuses_explicit_arrays():
  row, spec, inp, eng = engine_of("tomato_watering", n=70)            # an explicit random-stream array
  row2, spec2, inp2, eng2 = engine_of("island_ex_packed", n=70)
  small = None
  try:
    with pytest.raises(ValueError):
      eng.fork(n_envs=40)
    small = eng2.fork(n_envs=40, env_id_base=5)
    assert small.n_envs == 40 and small.env_id_base == 5 and small.spec is eng2.spec
  finally:
    if small is not None:
      small.close()
    eng.close()
    eng2.close()


# ---- 3. gather / scatter against torch --------------------------------------------------------------------------------------------
N_SRC, N_DST = 130, 70


def pair_lists():
  """60 pairs: distinct destinations on both sides of the 64-env boundary, 10 sources used twice or more, 12 skipped pairs
  (-1 and >= n_envs, on either side)."""
  rs = np.random.default_rng(5)
  dst = rs.permutation(N_DST)[:60].astype(np.int32)
  src = rs.integers(0, N_SRC, 60).astype(np.int32)
  src[:10] = src[10:20]                                               # fan-out
  src[20:24] = (-1, N_SRC, N_SRC + 61, 1 << 20)                        # (N_SRC + 61 = 191: a padding row of the source)
  dst[24:32] = (-1, -5, N_DST, N_DST + 57, 128, 1 << 20, -1, N_DST + 1)   # (N_DST + 57 = 127: a padding row of the destination)
  valid = (src >= 0) & (src < N_SRC) & (dst >= 0) & (dst < N_DST)
  assert (~valid).sum() >= 8 and len(set(dst[valid])) == valid.sum()
  assert (np.bincount(src[valid], minlength=N_SRC) >= 2).sum() >= 8, "repeated sources"
  assert (dst[valid] < 64).any() and (dst[valid] >= 64).any() and (src[valid] < 64).any() and (src[valid] >= 64).any()
  return src, dst, valid


def stepped(row_id, n, seed, steps):
  row, spec, inp, eng = engine_of(row_id, n=n, seed=seed)
  LP.start(eng, row)
  eng.step_n(eng.fill_actions(steps, seed), accumulate=True)          # (one launch per step; the accumulators are not empty)
  return row, eng


@pytest.mark.parametrize("row_id", ("island_ex_packed", "firemaker_ex_ma"))
def test_gather_scatter_equals_torch_indexing(row_id):
  rs_, src = stepped(row_id, N_SRC, 41, 27)                           # (episodes of 12 / 14 steps: some have finished)
  rd_, dst = stepped(row_id, N_DST, 42, 19)
  try:
    words = int(src._lib.sgw_state_words(src._h))
    assert words == int(dst._lib.sgw_state_words(dst._h))
    if row_id == "island_ex_packed":
      assert words == 10
    else:
      assert words % 2 == 1, "the row picked for an odd number of state words has %d" % words
    si, di, valid = pair_lists()
    s0, d0 = src.get_state().clone(), dst.get_state().clone()
    sb0, db0 = bufs_of(src), bufs_of(dst)
    sr0, dr0 = src.read_returns().clone(), dst.read_returns().clone()
    assert sr0[-1] > 0 and dr0[-1] > 0, "episodes have finished: the accumulators hold something"
    sv, dv = torch.from_numpy(si[valid]).long().to(DEV), torch.from_numpy(di[valid]).long().to(DEV)
    differ = (s0[:, sv] != d0[:, dv]).any(dim=0)
    assert int(differ.sum()) * 2 > len(sv), "the engines must differ before the copy"
    dst.copy_envs(src, src_idx=si, dst_idx=di)                         # host arrays: uploaded once
    want = d0.clone()
    want[:, dv] = s0[:, sv]
    assert same(dst.get_state(), want), "state, all [words, n_pad] columns"
    assert set(dst._bufs) == set(rd_["outs"])
    for k in dst._bufs:
      wb = db0[k].clone()
      wb[dv] = sb0[k][sv]
      assert same(dst._bufs[k], wb), "output %s over all n_pad rows" % k
    assert same(src.get_state(), s0), "the source's state is not written"
    for k in src._bufs:
      assert same(src._bufs[k], sb0[k]), "the source's %s is not written" % k
    assert same(src.read_returns(), sr0) and same(dst.read_returns(), dr0), "the accumulators do not travel"
    # the same pairs as device tensors, state only, into a fresh copy of the destination's old state
    dst.set_state(d0)
    for k in dst._bufs:
      dst._bufs[k].copy_(db0[k])
    dst.copy_envs(src, src_idx=torch.from_numpy(si).to(DEV), dst_idx=torch.from_numpy(di).to(DEV), outputs=False)
    assert same(dst.get_state(), want)
    for k in dst._bufs:
      assert same(dst._bufs[k], db0[k]), "outputs=False leaves %s alone" % k
  finally:
    src.close()
    dst.close()


# ---- 4. one engine, disjoint sets -------------------------------------------------------------------------------------------------
def test_same_engine_disjoint_sets():
  row, eng = stepped("island_ex_packed", N_SRC, 43, 9)
  try:
    s0, b0 = eng.get_state().clone(), bufs_of(eng)
    r0 = eng.read_returns().clone()
    si = torch.arange(40, 72, dtype=torch.int32, device=DEV)
    di = torch.arange(96, 128, dtype=torch.int32, device=DEV)
    assert bool((s0[:, 40:72] != s0[:, 96:128]).any())
    eng.copy_envs(eng, src_idx=si, dst_idx=di)
    want = s0.clone()
    want[:, 96:128] = s0[:, 40:72]
    assert same(eng.get_state(), want)
    for k, v in eng._bufs.items():
      wb = b0[k].clone()
      wb[96:128] = b0[k][40:72]
      assert same(v, wb), k
    eng.copy_envs(eng)                                                  # every env onto itself: every pair is skipped
    assert same(eng.get_state(), want) and same(eng.read_returns(), r0)
  finally:
    eng.close()


# ---- 5. refused calls -------------------------------------------------------------------------------------------------------------
def raw_copy(dst, src, n, dst_out=None, src_out=None):
  return dst._lib.sgw_copy_envs(dst._h, src._h, None, None, n, C.byref(dst_out) if dst_out is not None else None,
                                C.byref(src_out) if src_out is not None else None, dst._stream())


def test_refused_calls_launch_nothing():
  ra, a = stepped("island_ex_packed", N_DST, 44, 5)
  spec_b = make_spec("island_navigation_ex", level=5, max_iterations=13)          # one field away from a's spec
  b = BatchedEngine(spec_b, N_DST, device=DEV, outputs=ra["outs"])
  rf, spec_f, inp_f, f_src = engine_of("firemaker_ex_ma", n=N_DST)
  f_dst = BatchedEngine(spec_f, N_DST, device=DEV, outputs=rf["outs"])              # its generators are never set
  try:
    b.reset()
    s0 = b.get_state().clone()
    assert raw_copy(b, a, N_DST) == ERR_ARG and b"spec" in a._lib.sgw_last_error()
    with pytest.raises(N.SgwError):
      b.copy_envs(a)
    assert same(b.get_state(), s0)
    # an output set in dst_out and NULL in src_out
    s0 = a.get_state().clone()
    d_out, s_out = N.Out(), N.Out()
    d_out.board, d_out.reward = a._bufs["board"].data_ptr(), a._bufs["reward"].data_ptr()
    s_out.board = a._bufs["board"].data_ptr()
    si = torch.arange(0, 8, dtype=torch.int32, device=DEV)
    di = torch.arange(32, 40, dtype=torch.int32, device=DEV)
    rc = a._lib.sgw_copy_envs(a._h, a._h, di.data_ptr(), si.data_ptr(), 8, C.byref(d_out), C.byref(s_out), a._stream())
    assert rc == ERR_ARG and b"src_out" in a._lib.sgw_last_error()
    rc = a._lib.sgw_copy_envs(a._h, a._h, di.data_ptr(), si.data_ptr(), 8, C.byref(d_out), None, a._stream())
    assert rc == ERR_ARG
    assert same(a.get_state(), s0)
    # a generator family whose destination was never seeded
    LP.start(f_src, rf)
    s0 = f_dst.get_state().clone()
    assert raw_copy(f_dst, f_src, N_DST) == ERR_ARG and b"generators" in a._lib.sgw_last_error()
    assert same(f_dst.get_state(), s0)
    f_dst.seed_rng()
    assert raw_copy(f_dst, f_src, N_DST) == 0, "seeded by its own setter: accepted"
    assert same(f_dst.get_state()[:, :N_DST], f_src.get_state()[:, :N_DST])
  finally:
    for e in (a, b, f_src, f_dst):
      e.close()


# ---- 6. lookahead -----------------------------------------------------------------------------------------------------------------
LOOK_B, LOOK_AT, LOOK_SEED, LOOK_CAND_SEED = 4, 10, 0xA1, 0xB2


def lookahead_is_the_step_not_taken(row, eng, third):
  """Two fresh engines of `row`: LOOK_AT steps of the sgw_fill_actions stream (seed LOOK_SEED), then LOOK_B candidate action sets
  (seed LOOK_CAND_SEED) through lookahead() against `third` restored from a snapshot; entry 2 is then taken.  Closes both; returns
  lookahead()'s stacked result {field: [LOOK_B, N, ...]} as it was before the step."""
  B, row_id = LOOK_B, row["id"]
  try:
    LP.start(eng, row)
    LP.start(third, row)
    acts = eng.fill_actions(LOOK_AT, LOOK_SEED)
    for t in range(LOOK_AT):
      eng.step(acts[t])
    cand = eng.fill_actions(B, LOOK_CAND_SEED)                          # int8 [B, N(, A)]: four different action sets
    snap, b0, r0 = eng.get_state().clone(), bufs_of(eng), eng.read_returns().clone()
    res = eng.lookahead(cand)
    assert set(res) == set(row["outs"])
    for b in range(B):
      third.set_state(snap)
      o = third.step(cand[b])
      for k in row["outs"]:
        assert tuple(res[k].shape) == (B,) + tuple(o[k].shape)
        assert same(res[k][b], o[k]), "%s candidate %d: %s" % (row_id, b, k)
    boards = res["board"].reshape(B, row["n"], -1)
    assert bool((boards[1:] != boards[:1]).any()), "the candidates must lead to different boards somewhere"
    assert same(eng.get_state(), snap), "lookahead does not move the engine"
    for k, v in eng._bufs.items():
      assert same(v, b0[k]), "lookahead does not write the engine's %s" % k
    assert same(eng.read_returns(), r0)
    kept = {k: v[2].clone() for k, v in res.items()}
    whole = {k: v.clone() for k, v in res.items()}
    o = eng.step(cand[2])
    for k in row["outs"]:
      assert same(o[k], kept[k]), "%s: step(actions[2]) differs from entry 2 in %s" % (row_id, k)
    assert eng.lookahead(cand)["board"].data_ptr() == res["board"].data_ptr(), "persistent result tensors"
    return whole
  finally:
    eng.close()
    third.close()


@pytest.mark.parametrize("row_id", ("island_ex_packed", "safe_interruptibility_ex", "firemaker_ex_ma"))
def test_lookahead_is_the_step_not_taken(row_id):
  row, spec, inp, eng = engine_of(row_id)
  lookahead_is_the_step_not_taken(row, eng, LP.make_engine(row, spec, inp))


# ---- 7. under graph capture -------------------------------------------------------------------------------------------------------
def test_copy_and_step_under_graph_capture():
  """Plain launches on the caller's stream: a state + outputs copy and a step of the fork, captured by torch.cuda.graph on a side
  stream after a warm-up outside the capture; replayed twice, the source and the action buffer refilled in between, it leaves the
  bytes the direct calls leave in a second fork."""
  row, spec, inp, src = engine_of("island_ex_packed")
  n = row["n"]
  dst = dst2 = None
  try:
    LP.start(src, row)
    feed = src.fill_actions(12, 0xC3)
    for t in range(6):
      src.step(feed[t])
    dst, dst2 = src.fork(), src.fork()
    rs = np.random.default_rng(9)
    perm = rs.permutation(n).astype(np.int32)
    didx = np.arange(n, dtype=np.int32)
    didx[::37] = -1                                                      # some envs of the fork keep going on their own
    si, di = torch.from_numpy(perm).to(DEV), torch.from_numpy(didx).to(DEV)
    abuf = feed[6].clone()

    def both(e):
      e.copy_envs(src, src_idx=si, dst_idx=di)
      return e.step(abuf)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # warm-up outside the capture
      both(dst)
    side.synchronize()
    both(dst2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
      both(dst)
    for r in (1, 2):
      src.step(feed[6 + r])                                             # refill the source ...
      abuf.copy_(feed[8 + r])                                           # ... and the actions, in place
      torch.cuda.synchronize()
      graph.replay()
      both(dst2)
      torch.cuda.synchronize()
      assert same(dst.get_state(), dst2.get_state()), "replay %d: state" % r
      for k in dst._bufs:
        assert same(dst._bufs[k], dst2._bufs[k]), "replay %d: %s" % (r, k)
    assert not same(dst.get_state()[:, :n], src.get_state()[:, :n])
  finally:
    for e in (src, dst, dst2):
      if e is not None:
        e.close()
