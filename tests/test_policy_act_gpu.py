"""sgw_policy_act through the C ABI on synthetic observation bytes against tests/policy_ref.py: the ragged ends of a wave and of a
four-wave workgroup, boards of several sizes, windows of different sizes per agent, several tables with an index out of range,
exploration never / sometimes / always, nonzero t and *step_dev, guard bytes around the actions, and rows n >= N full of a byte
whose code would win."""
import ctypes as C

import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import BatchedEngine, fused_views
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec
from tests import policy_gpu_util as U
from tests import policy_ref

pytestmark = pytest.mark.gpu

BASE = (1 << 32) + 5             # global env ids with a high word
GUARD = 64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("geo", sorted(U.GEOMETRIES))
def test_act_matches_the_numpy_statement(geo, n):
  name, kw, source = U.GEOMETRIES[geo]
  spec = make_spec(name, **kw)
  eng = BatchedEngine(spec, n, device=U.DEV, env_id_base=BASE, outputs=U.outputs_for(spec, source))
  L = N.lib()
  rng = np.random.default_rng(n * 7 + len(geo))
  chars = list(spec.layer_chars) + [U.WIN]
  c_a, off_a, row = policy_ref.geometry(spec, source)
  assert row == (spec.H * spec.W if source == "board" else int(L.sgw_view_bytes(eng._h)))
  # observation rows: the spec's characters and a few bytes outside them (code 0); rows n >= N hold the winning byte
  alphabet = np.array([ord(c) for c in spec.layer_chars] + [0, 7, 200, 255], np.uint8)
  obs = np.full((eng.n_pad, row), ord(U.WIN), np.uint8)
  obs[:n] = alphabet[rng.integers(0, len(alphabet), size=(n, row))]
  obs_dev = torch.from_numpy(obs).to(U.DEV)
  for P, below, mixed in ((1, 0, False), (3, 1 << 30, True), (3, 1 << 32, False), (1, 1 << 30, True)):
    pol = TablePolicy(eng, source=source, chars=chars, n_policies=P, seed=99 + P)
    pol.explore_below = below
    w, b, idx = U.fill_policy(pol, rng, mixed, with_index=P > 1)
    pol.step.fill_(1000)
    buf = torch.full((n * spec.A + 2 * GUARD,), 0x55, dtype=torch.int8, device=U.DEV)
    rc = L.sgw_policy_act(eng._h, C.byref(pol.native()), obs_dev.data_ptr(), 5, buf.data_ptr() + GUARD, None)
    assert rc == 0, L.sgw_last_error()
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0x55).all() and (got[GUARD + n * spec.A:] == 0x55).all(), "bytes outside [N, A] were written"
    want = U.ref_actions(pol, obs[:n], w, b, idx, BASE, 1005)
    assert (got[GUARD:GUARD + n * spec.A].reshape(n, spec.A) == want).all(), "P=%d explore_below=%d" % (P, below)
    assert int(pol.step.item()) == 1000, "sgw_policy_act does not advance the step"
    if idx is not None and n > 1:
      assert (want[0] == 0).all()                                            # the env whose table index is out of range
  # the inputs do their work: the winning byte is in every row n >= N and in no row n < N, and its code decides a row that holds it
  assert not (obs[:n] == ord(U.WIN)).any() and (obs[n:] == ord(U.WIN)).all()
  poisoned = policy_ref.act(np.full((1, row), ord(U.WIN), np.uint8), pol.code_of.cpu().numpy(), w, b, None, c_a, off_a, pol.n_actions,
                            pol.action_lo, 0, 0, [BASE], 0)
  assert (poisoned[:, [a for a in range(spec.A) if c_a[a] > 0]] == pol.action_lo + pol.n_actions - 1).all()
  eng.close()


def test_engine_act_reads_the_current_output_and_takes_explicit_rows():
  spec = make_spec("island_navigation_ex", level=9)
  eng = BatchedEngine(spec, 65, device=U.DEV, outputs=("board", "reward", "step_type"))
  eng.reset()
  pol = TablePolicy(eng, n_policies=2, seed=3, epsilon=0.25)
  w, b, idx = U.fill_policy(pol, np.random.default_rng(5), True)
  board = eng._bufs["board"].cpu().numpy()[:65]
  got = eng.act(pol, t=3)
  assert got.shape == (65, 1) and got.dtype == torch.int8
  assert (got.cpu().numpy() == U.ref_actions(pol, board, w, b, idx, 0, 3)).all()
  rows = torch.from_numpy(np.ascontiguousarray(board[::-1].copy())).to(U.DEV)    # [N, H*W]: rows >= N are never read
  out = torch.zeros((65, 1), dtype=torch.int8, device=U.DEV)
  assert eng.act(pol, obs=rows, out=out).data_ptr() == out.data_ptr()
  assert (out.cpu().numpy() == U.ref_actions(pol, board[::-1], w, b, idx, 0, 0)).all()
  eng.close()


def test_refusals():
  L = N.lib()
  spec = make_spec("island_navigation_ex", level=9)
  eng = BatchedEngine(spec, 65, device=U.DEV, outputs=("reward", "step_type"))           # no board output
  full = BatchedEngine(spec, 65, device=U.DEV, outputs=("board", "reward", "step_type"))
  with pytest.raises(N.SgwError, match="windows"):
    TablePolicy(full, source="views")
  full.reset()
  pol = TablePolicy(full)
  acts = torch.zeros((8, 65, 1), dtype=torch.int8, device=U.DEV)
  obs = full._bufs["board"]

  def step_n(engine, p, out):
    return L.sgw_policy_step_n(engine._h, C.byref(p), obs.data_ptr(), 8, 0, C.byref(out), acts.data_ptr(), 0, None)

  def variant(**kw):
    p = N.Policy.from_buffer_copy(pol.native())
    for k, v in kw.items():
      setattr(p, k, v)
    return p

  assert step_n(full, pol.native(), full._out) == 0
  assert step_n(eng, pol.native(), eng._out) == -1 and b"board" in L.sgw_last_error()           # missing board output
  assert step_n(full, variant(source=N.POLICY_VIEWS), full._out) == -1 and b"windows" in L.sgw_last_error()
  assert step_n(full, variant(n_codes=65), full._out) == -1 and b"n_codes" in L.sgw_last_error()
  assert step_n(full, variant(explore_below=(1 << 32) + 1), full._out) == -1 and b"explore_below" in L.sgw_last_error()
  assert step_n(full, variant(cells=47), full._out) == -1 and b"cells" in L.sgw_last_error()
  assert step_n(full, variant(step_dev=None), full._out) == -1
  assert L.sgw_policy_step_n(full._h, C.byref(pol.native()), obs.data_ptr(), 0, 0, C.byref(full._out), acts.data_ptr(), 0, None) == -1
  assert L.sgw_policy_act(full._h, C.byref(variant(n_codes=0)), obs.data_ptr(), 0, acts.data_ptr(), None) == -1
  with pytest.raises(N.SgwError, match="board"):
    eng.policy_step_n(pol, 8)
  # windows that do not come from the step launch: refused at the Python level
  wide = make_spec("island_navigation_ex_ma", observation_radius=[4, 4, 4, 4])           # 9 x 9 windows on a 6 x 8 board
  assert not fused_views(wide)
  ima = BatchedEngine(wide, 65, device=U.DEV, outputs=("board", "views", "step_type"))
  with pytest.raises(N.SgwError, match="fused_views"):
    ima.policy_step_n(TablePolicy(ima, source="views"), 8)
  eng.close(); full.close(); ima.close()
