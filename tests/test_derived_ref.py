"""The numpy references of tests/derived_ref.py against the reference's own outputs in the committed fixtures (no GPU): the
derived statistics, RGB planes, unoccluded layers, agent windows and per-layer agent cubes they compute from a fixture's
inputs must equal the arrays the reference recorded, bit for bit.  tests/test_derived_kernels_gpu.py then holds the kernels
to these references over the whole domain include/sgw.h declares."""
import numpy as np
import pytest

from ai_safety_gridworlds_amd.specs import make_spec
from tests import derived_ref as R
from tests import golden_util as G

MAX_ENVS = 32             # envs per fixture (the statistics' reference is a Python loop per env and step)


def _spec(meta):
  return make_spec(meta["family_name"], **meta["kwargs"])


STATS_FIXTURES = [n for n in G.fixture_names() if "gini_index" in np.load(G.GOLDEN + "/" + n + ".npz").files
                  and "reward" in np.load(G.GOLDEN + "/" + n + ".npz").files]
RGB_FIXTURES = [n for n in G.fixture_names() if "rgb" in np.load(G.GOLDEN + "/" + n + ".npz").files]
# aintelope_savanna's layers come from its state (sgw_state_layers), not from the board.  conveyor_belt_ex (the belt under the
# object) and safe_interruptibility_ex (the interruption tile under the agent, the button row) have drapes whose curtains the
# board does not show: the layer tables of their specs do not model those yet, so their fixture layers are not a check of
# the board-derived contract
LAYERS_NOT_FROM_BOARD = ("sav_", "conveyorex_", "safeintex_")
LAYER_FIXTURES = [n for n in G.fixture_names() if "layers" in np.load(G.GOLDEN + "/" + n + ".npz").files
                  and not n.startswith(LAYERS_NOT_FROM_BOARD)]
VIEW_FIXTURES = [n for n in G.fixture_names(["firemaker_", "ima_"])]


def test_fixture_lists_are_complete():
  # 8 of them the `_quit` / `_quitlate` tapes of the four multi-objective families, 5 the `island_num_*` tapes of tests/flag_fixtures.py
  assert len(STATS_FIXTURES) == 45
  assert len(RGB_FIXTURES) >= 65 and len(LAYER_FIXTURES) >= 34
  # 8 of them the `_quit` / `_quitlate` tapes of firemaker_ex_ma and island_navigation_ex_ma, 7 the `*_num_*` / `*_asym*` tapes
  assert len(VIEW_FIXTURES) == 46


@pytest.mark.parametrize("name", STATS_FIXTURES)
def test_stats_ref_reproduces_fixture(name):
  """gini_index ... average_reward (safety_game_mo.py:1027-1084) from the recorded reward, cumulative reward and frame."""
  fx, meta = G.load(name)
  E = min(MAX_ENVS, fx["reward"].shape[0])
  reward, cumulative, frame = fx["reward"][:E], fx["cumulative"][:E], fx["frame"][:E]
  T, K = reward.shape[1], reward.shape[2]
  got = R.stats_ref(reward.reshape(E * T, 1, K), cumulative.reshape(E * T, 1, K), frame.reshape(-1), [K])[:, 0]
  for i, key in enumerate(R.STATS_NAMES):
    R.assert_bits(name + "." + key, got[:, i], fx[key][:E].reshape(-1))
  R.assert_bits(name + ".average_reward", got[:, 5:], fx["average_reward"][:E].reshape(E * T, K))


def test_stats_ref_absent_agent_and_empty_columns():
  """An agent without reward dimensions: gini 0, variances NaN (np.var of an empty list); columns past k stay 0."""
  reward = np.array([[[1.0, 2.0, 0.0], [0.0, 0.0, 0.0]]])
  got = R.stats_ref(reward, reward * 3, np.array([4]), [2, 0])
  assert got.shape == (1, 2, 8)
  assert got[0, 1, 0] == 0.0 and got[0, 1, 1] == 0.0 and np.isnan(got[0, 1, 2:5]).all() and (got[0, 1, 5:] == 0).all()
  assert got[0, 0, 7] == 0.0 and got[0, 0, 5] == 3.0 / 5 and got[0, 0, 6] == 6.0 / 5


@pytest.mark.parametrize("name", RGB_FIXTURES)
def test_rgb_ref_reproduces_fixture(name):
  fx, meta = G.load(name)
  spec = _spec(meta)
  rgb = fx["rgb"]                                                  # [e, T, 3, H, W] of the first envs
  e, T = rgb.shape[:2]
  board = fx["board"][:e].reshape(e * T, spec.H * spec.W)
  R.assert_bits(name + ".rgb", R.rgb_ref(board, spec.rgb_lut()), rgb.reshape(e * T, 3, spec.H * spec.W))


def _hidden_flags(spec, layers, pos):
  """firemaker: fire that spread under an agent is invisible in the board; the step reports it in agent_flags bit 0.  The
  fixture does not record the flags, so they are read off the fixture's own fire layer at the agent's cell (the rest of
  every layer is still checked against the board)."""
  Fi = spec.layer_chars.index(spec.hidden_layer_char)
  n, A = pos.shape[:2]
  return np.array([[layers[i, Fi, pos[i, a, 0], pos[i, a, 1]] for a in range(A)] for i in range(n)], np.uint8)


@pytest.mark.parametrize("name", LAYER_FIXTURES)
def test_unoccluded_layers_ref_reproduces_fixture(name):
  """observation['layers']: the spec's layer tables (layer_chars, layer_static) + the gap correction, from the board."""
  fx, meta = G.load(name)
  spec = _spec(meta)
  assert "".join(spec.layer_chars) == meta["layer_chars"]
  lay = fx["layers"]
  e, T, L = lay.shape[:3]
  board = fx["board"][:e].reshape(e * T, spec.H, spec.W)
  want = lay.reshape(e * T, L, spec.H, spec.W)
  gap = spec.layer_chars.index(spec.what_lies_beneath) if spec.what_lies_beneath in spec.layer_chars else -1
  pos = flags = None
  hidden = -1
  if getattr(spec, "hidden_layer_char", None):
    pos = fx["pos"][:e].reshape(e * T, spec.A, 2)
    flags = _hidden_flags(spec, want, pos)
    hidden = spec.layer_chars.index(spec.hidden_layer_char)
  got = R.unoccluded_layers_ref(board, spec.layer_chars, spec.layer_static(), gap, pos, flags, hidden)
  R.assert_bits(name + ".layers", got, want.reshape(e * T, L, spec.H * spec.W).astype(np.uint8))


def _agent_windows(name):
  """(spec, per-slot radius, per-slot agent char, positions [n, A, 2], directions [n, A] or None, boards [n, H, W], the
  fixture) for the first MAX_ENVS envs of a windowed multi-agent fixture."""
  fx, meta = G.load(name)
  spec = _spec(meta)
  E = min(MAX_ENVS, fx["board"].shape[0])
  T = fx["board"].shape[1]
  slots = getattr(spec, "agent_slots", list(range(len(spec.agent_chars))))
  chars = [None] * spec.A
  for c, q in zip(spec.agent_chars, slots):
    chars[q] = c
  radii = [tuple(spec.native.view_radius[a]) if spec.native.view_radius[a][0] >= 0 else None for a in range(spec.A)]
  pos = fx["pos"][:E].reshape(E * T, spec.A, 2).astype(np.int64)
  dirs = fx["observation_direction"][:E].reshape(E * T, spec.A) if spec.rotating_views else None
  board = fx["board"][:E].reshape(E * T, spec.H, spec.W)
  return spec, radii, chars, pos, dirs, board, fx, E


@pytest.mark.parametrize("name", VIEW_FIXTURES)
def test_views_ref_reproduces_fixture(name):
  """The agents' windows (get_agent_perspective) from the board, the recorded positions and observation directions.  A
  window is checked wherever its agent is on the board (an agent that left the game has no meaningful window)."""
  spec, radii, chars, pos, dirs, board, fx, E = _agent_windows(name)
  outside = ord(spec.what_lies_outside) if spec.what_lies_outside else spec.native.view_outside
  if "view" in fx.files:
    want = [fx["view"][:E].reshape((len(board), -1) + fx["view"].shape[-2:])[:, a] for a in range(spec.A)]
  else:
    wk = fx["view_worker"][:E].reshape((len(board), 2) + fx["view_worker"].shape[-2:])
    want = [wk[:, 0], wk[:, 1], fx["view_supervisor"][:E].reshape((len(board),) + fx["view_supervisor"].shape[-2:])]
  checked = 0
  for a, rad in enumerate(radii):
    if rad is None:
      continue
    on = board[np.arange(len(board)), pos[:, a, 0].clip(0, spec.H - 1), pos[:, a, 1].clip(0, spec.W - 1)] == ord(chars[a])
    idx = np.nonzero(on)[0]
    only = [r if b == a else None for b, r in enumerate(radii)]
    got = R.views_ref(board[idx], pos[idx], None if dirs is None else (dirs[idx] << 3), only, outside)
    R.assert_bits("%s.view[%d]" % (name, a), got, want[a][idx].reshape(len(idx), -1))
    checked += len(idx)
  assert checked > 0


@pytest.mark.parametrize("name", [n for n in VIEW_FIXTURES if n.startswith("firemaker_")])
def test_layer_views_ref_reproduces_fixture(name):
  """The per-agent crops of every layer (agent_perspectives_with_layers) from the fixture's own layers."""
  spec, radii, chars, pos, dirs, board, fx, E = _agent_windows(name)
  lay = fx["layers"]
  e, T, L = lay.shape[:3]
  layers = lay.reshape(e * T, L, spec.H, spec.W).astype(np.uint8)
  outside = chr(spec.native.view_outside)
  want = [fx["agent_layers_worker"][:, :, 0], fx["agent_layers_worker"][:, :, 1], fx["agent_layers_supervisor"]]
  n = e * T
  for a, rad in enumerate(radii):
    if rad is None:
      continue
    on = board[:n][np.arange(n), pos[:n, a, 0], pos[:n, a, 1]] == ord(chars[a])
    idx = np.nonzero(on)[0]
    only = [r if b == a else None for b, r in enumerate(radii)]
    got = R.layer_views_ref(layers[idx], pos[:n][idx], None if dirs is None else (dirs[:n][idx] << 3), only, spec.layer_chars, outside)
    R.assert_bits("%s.agent_layers[%d]" % (name, a), got, want[a].reshape(n, -1)[idx].astype(np.uint8))


def test_track_performance_ref_rules():
  """LAST ends an episode of a single-agent env; per-agent families need every agent LAST or DEAD."""
  perf = np.array([[1.0], [2.0], [3.0]])
  st = np.array([[R.LAST, R.MID], [R.LAST, R.DEAD], [R.MID, R.LAST]], np.uint8)
  z = np.zeros((3, 1))
  c = np.zeros(3, np.int64)
  last, tot, cnt, done = R.track_performance_ref(perf, st, False, z, z, c)
  assert done.tolist() == [1, 1, 0] and cnt.tolist() == [1, 1, 0] and tot[:, 0].tolist() == [1.0, 2.0, 0.0]
  last, tot, cnt, done = R.track_performance_ref(perf, st, True, last, tot, cnt)
  assert done.tolist() == [0, 1, 0] and cnt.tolist() == [1, 2, 0] and tot[:, 0].tolist() == [1.0, 4.0, 0.0]
