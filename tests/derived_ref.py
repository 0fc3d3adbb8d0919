"""Plain numpy references of the derived-observation entry points (include/sgw.h: sgw_derived_stats, sgw_observe,
sgw_observe_layers, sgw_agent_views, sgw_agent_layer_views, sgw_track_performance), written from the reference's formulas.
They are test infrastructure: slow (a Python loop per env where numpy's own reduction order is the contract), exact, and
anchored to the committed fixtures by tests/test_derived_ref.py before the GPU tests compare the kernels with them."""
import warnings

import numpy as np

LEFT, RIGHT, UP, DOWN = 0, 1, 2, 3          # Directions (bits 3-4 of agent_flags)
FIRST, MID, LAST, DEAD = 0, 1, 2, 3          # sgw_step_type
STATS_NAMES = ("gini_index", "cumulative_gini_index", "mo_variance", "cumulative_mo_variance", "average_mo_variance")


def gini_coefficient(reward_dims):
  """gini_coefficient (safety_game_mo.py:1645-1681): Python min() of the list, np.subtract.outer, .mean(), + eps."""
  if len(reward_dims) == 0:
    return np.float64(0.0)
  d = np.array(reward_dims) - min(reward_dims)
  mad = np.abs(np.subtract.outer(d, d)).mean()
  rel_mad = mad / (np.mean(d) + np.finfo(float).eps)
  return 0.5 * rel_mad


def _var(dims):
  if len(dims) == 0:
    return np.float64(np.nan)                # np.var([]) (a RuntimeWarning in the reference, NaN all the same)
  return np.var(dims, ddof=0)


def agent_stats(reward_dims, cumulative_dims, frame, K):
  """One agent's row of sgw_derived_stats: _process_timestep (safety_game_mo.py:1027-1084) on Python float lists."""
  average_dims = [x / (frame + 1) for x in cumulative_dims]      # Python float division by the int frame + 1
  row = np.zeros(5 + K, np.float64)
  row[0] = gini_coefficient(reward_dims) * 100
  row[1] = gini_coefficient(cumulative_dims) * 100
  row[2] = _var(reward_dims)
  row[3] = _var(cumulative_dims)
  row[4] = _var(average_dims)
  row[5:5 + len(average_dims)] = average_dims
  return row


def stats_ref(reward, cumulative, frame, k_agent):
  """reward / cumulative float64 [N, A, K], frame int [N], k_agent[A] -> float64 [N, A, 5 + K] = (gini_index,
  cumulative_gini_index, mo_variance, cumulative_mo_variance, average_mo_variance, average_reward[K]).  Agent a uses its
  first k_agent[a] dimensions; k = 0 (an absent agent) gives 0, 0, NaN, NaN, NaN and zero averages."""
  reward = np.asarray(reward, np.float64)
  cumulative = np.asarray(cumulative, np.float64)
  N, A, K = reward.shape
  out = np.zeros((N, A, 5 + K), np.float64)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)            # overflow of squares near 1e160, as in the reference
    for n in range(N):
      f = int(frame[n])
      for a in range(A):
        k = int(k_agent[a])
        out[n, a] = agent_stats(reward[n, a, :k].tolist(), cumulative[n, a, :k].tolist(), f, K)
  return out


def rgb_ref(board, lut):
  """board uint8 [N, H*W] (codes < 128), lut uint8 [128, 3] -> uint8 [N, 3, H*W] (observation_distiller.py:88-90)."""
  board = np.asarray(board).reshape(len(board), -1)
  return np.ascontiguousarray(np.asarray(lut)[board].transpose(0, 2, 1))


def occluded_layers_ref(board, chars):
  """board uint8 [N, H*W], chars [L] -> uint8 [N, L, H*W]: board == char (rendering.py:69-185)."""
  board = np.asarray(board).reshape(len(board), -1)
  chars = np.asarray([ord(c) if isinstance(c, str) else c for c in chars], np.uint8)
  return (board[:, None, :] == chars[None, :, None]).astype(np.uint8)


def unoccluded_layers_ref(board, chars, static, gap_index, agent_pos=None, agent_flags=None, hidden_layer=-1):
  """The sgw_observe_layers contract.  board uint8 [N, H, W]; static uint8 [L, H*W]: 1 = the layer's static curtain is on
  there, 0 = off, 2 = a dynamic layer (on where the board shows its character); a dynamic drape hidden under an agent
  (agent_flags bit 0) is on at the agent's cell (agent_pos [N, A, 2]); then the what_lies_beneath layer `gap_index` keeps its
  curtain only where every other layer is blank (observation_distiller_ex.py:164-178).  The gap layer's curtain is static in
  every spec (the backdrop's what_lies_beneath cells).  -> uint8 [N, L, H*W]."""
  board = np.asarray(board)
  N, H, W = board.shape
  flat = board.reshape(N, H * W)
  chars = np.asarray([ord(c) if isinstance(c, str) else c for c in chars], np.uint8)
  static = np.asarray(static).reshape(len(chars), H * W)
  on = (static != 0) & (static != 2)
  dyn = static == 2
  lay = on[None] | (dyn[None] & (flat[:, None, :] == chars[None, :, None]))
  if agent_pos is not None and hidden_layer is not None and hidden_layer >= 0:
    pos = np.asarray(agent_pos).reshape(N, -1, 2)
    flags = np.asarray(agent_flags).reshape(N, -1)
    for a in range(pos.shape[1]):
      hid = (flags[:, a] & 1) != 0
      cell = pos[:, a, 0].astype(np.int64) * W + pos[:, a, 1]
      lay[np.nonzero(hid)[0], hidden_layer, cell[hid]] = True
  if gap_index is not None and gap_index >= 0:
    others = np.delete(lay, gap_index, axis=1).any(axis=1)
    lay[:, gap_index] &= ~others
  return lay.astype(np.uint8)


def window(plane, r, c, rad, direction, outside):
  """get_agent_perspective (safety_game_moma.py:1996-2101) of one 2-D plane: the (up + down + 1) x (left + right + 1) crop
  around (r, c), cells beyond the board = `outside`; then rot90 by the observation direction (2085-2096: UP none, DOWN k=2,
  LEFT k=-1, RIGHT k=1); direction None = no rotation (observation_direction_mode 0)."""
  up, down, left, right = rad
  padded = np.pad(plane, ((up, down), (left, right)), constant_values=outside)
  out = padded[r:r + up + down + 1, c:c + left + right + 1]
  if direction == DOWN:
    out = np.rot90(out, k=2)
  elif direction == LEFT:
    out = np.rot90(out, k=-1)
  elif direction == RIGHT:
    out = np.rot90(out, k=1)
  return out


def _directions(agent_flags, N, A):
  if agent_flags is None:
    return np.full((N, A), -1, np.int64)
  return (np.asarray(agent_flags).reshape(N, A).astype(np.int64) >> 3) & 3


def views_ref(board, pos, flags, radii, outside):
  """sgw_agent_views: board uint8 [N, H, W], pos [N, A, 2], flags [N, A] or None (no rotation), radii[A] = (up, down, left,
  right) or None (no view) -> uint8 [N, view_bytes], agent a's window at the sum of the previous agents' window sizes."""
  board = np.asarray(board)
  N = board.shape[0]
  A = len(radii)
  pos = np.asarray(pos).reshape(N, A, 2).astype(np.int64)
  dirs = _directions(flags, N, A)
  rows = []
  for n in range(N):
    parts = []
    for a, rad in enumerate(radii):
      if rad is None:
        continue
      d = dirs[n, a] if flags is not None else None
      parts.append(window(board[n], pos[n, a, 0], pos[n, a, 1], rad, d, outside).reshape(-1))
    rows.append(np.concatenate(parts))
  return np.stack(rows).astype(np.uint8)


def layer_views_ref(layers, pos, flags, radii, chars, outside):
  """sgw_agent_layer_views: layers uint8 [N, L, H, W] -> uint8 [N, L * view_bytes], per env agent-major
  [agent][layer][h][w]; cells beyond the board read (layer char == outside) (agent_perspectives_with_layers,
  safety_game_moma.py:430-525)."""
  layers = np.asarray(layers)
  N, L = layers.shape[:2]
  A = len(radii)
  chars = [ord(c) if isinstance(c, str) else int(c) for c in chars]
  outside = ord(outside) if isinstance(outside, str) else int(outside)
  pos = np.asarray(pos).reshape(N, A, 2).astype(np.int64)
  dirs = _directions(flags, N, A)
  rows = []
  for n in range(N):
    parts = []
    for a, rad in enumerate(radii):
      if rad is None:
        continue
      d = dirs[n, a] if flags is not None else None
      for l in range(L):
        parts.append(window(layers[n, l], pos[n, a, 0], pos[n, a, 1], rad, d, 1 if chars[l] == outside else 0).reshape(-1))
    rows.append(np.concatenate(parts))
  return np.stack(rows).astype(np.uint8)


def track_performance_ref(perf, step_type, per_agent, last, total, count):
  """sgw_track_performance: one step's bookkeeping of _episodic_performances (safety_game.py:194-263, 301-302;
  safety_game_mo.py:917-938, 1015-1016).  perf float64 [N, C], step_type uint8 [N, A]; an episode ends where the step type
  is LAST (per_agent: every agent LAST or DEAD, the families whose agents finish one by one).  There last = perf, total +=
  perf (episode after episode, left to right), count += 1.  Returns new (last, total, count, done)."""
  st = np.asarray(step_type).reshape(len(perf), -1)
  done = (st >= LAST).all(axis=1) if per_agent else st[:, 0] == LAST
  last, total, count = last.copy(), total.copy(), count.copy()
  last[done] = perf[done]
  total[done] = total[done] + perf[done]
  count[done] += 1
  return last, total, count, done.astype(np.uint8)


def assert_bits(name, got, want):
  """Every element equal as a bit pattern (so -0.0 != 0.0), NaN for NaN whatever its payload."""
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.shape == want.shape, "%s: shape %s vs %s" % (name, got.shape, want.shape)
  if got.dtype.kind == "f":
    want = want.astype(got.dtype)
    bits = np.dtype("u%d" % got.dtype.itemsize)
    same = (got.view(bits) == want.view(bits)) | (np.isnan(got) & np.isnan(want))
  else:
    same = got.astype(np.int64) == want.astype(np.int64)
  if not same.all():
    bad = np.argwhere(~same)
    raise AssertionError("%s: %d mismatches, first at %s: got %r want %r" % (
        name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
