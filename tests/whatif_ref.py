"""numpy restatement of sgw_simulate_moves / sgw_fold_q_values: what SafetyEnvironmentMo.step(actions, q_value_per_action)
computes before it plays the step (safety_game_mo.py:810-857), with the carried position of a refused action, and the
tiletype_qvalue log cells.  Plain loops: this is the statement the device, the host shim and the fixtures are compared with."""
import decimal

import numpy as np

LEFT, RIGHT, UP, DOWN = 0, 1, 2, 3                      # Directions (agent_flags bits 1-2)
MOTION = {1: (0, -1), 2: (0, 1), 3: (-1, 0), 4: (1, 0)}  # Actions LEFT RIGHT UP DOWN; NOOP and the turning actions stay


def absolute_action(j, direction):
  """get_absolute_action (safety_game_mo_base.py:458-503) for a relative env: the move j seen from `direction`."""
  if not 1 <= j <= 4:
    return j
  left_of = {UP: LEFT, DOWN: RIGHT, LEFT: DOWN, RIGHT: UP}[direction]
  d = {3: direction, 4: direction ^ 1, 1: left_of, 2: left_of ^ 1}[j]
  return d + 1


def simulate_agent(board, row, col, direction, relative, impassable, n_actions):
  """board uint8 [H, W]; impassable: a str.  -> (pos [n_actions, 2], tile [n_actions], blocked [n_actions]) uint8."""
  H, W = board.shape
  pos, tile, blocked = np.zeros((n_actions, 2), np.uint8), np.zeros(n_actions, np.uint8), np.zeros(n_actions, np.uint8)
  if row >= H or col >= W:                               # never written by the engine: reports itself, tile 0, all refused
    pos[:] = (row, col)
    blocked[:] = 1
    return pos, tile, blocked
  carry = (row, col)
  for j in range(n_actions):
    a = absolute_action(j, direction) if relative else j
    dr, dc = MOTION.get(a, (0, 0))
    if (dr, dc) != (0, 0):
      nr, nc = row + dr, col + dc
      refused = not (0 <= nr < H and 0 <= nc < W) or chr(board[nr, nc]) in impassable
    else:
      nr, nc, refused = row, col, False
    if not refused:
      carry = (nr, nc)
    pos[j], tile[j], blocked[j] = carry, board[carry], refused
  return pos, tile, blocked


def simulate(board, agent_pos, agent_flags, relative, impassable, n_actions):
  """board [N, H, W], agent_pos [N, A, 2], agent_flags [N, A] or None, impassable: one str per agent."""
  N, A = agent_pos.shape[:2]
  pos = np.zeros((N, A, n_actions, 2), np.uint8)
  tile = np.zeros((N, A, n_actions), np.uint8)
  blocked = np.zeros((N, A, n_actions), np.uint8)
  for n in range(N):
    for a in range(A):
      d = UP if agent_flags is None else (int(agent_flags[n, a]) >> 1) & 3
      pos[n, a], tile[n, a], blocked[n, a] = simulate_agent(board[n], int(agent_pos[n, a, 0]), int(agent_pos[n, a, 1]), d, relative,
                                                            impassable[a], n_actions)
  return pos, tile, blocked


def fold(tile, q, tile_chars, table, seen):
  """tile [N, A, n_actions], q float64 [N, A, n_actions, D], tile_chars: sequence of byte values; table [N, A, L, D] and seen
  [N, A, L] are updated IN PLACE: the mean of the q-vectors that land on a tile type, one addition at a time in order of j."""
  N, A, NA = tile.shape
  D = q.shape[-1]
  for n in range(N):
    for a in range(A):
      for l, c in enumerate(tile_chars):
        js = [j for j in range(NA) if tile[n, a, j] == c]
        if not js:
          continue
        for d in range(D):
          s = np.float64(q[n, a, js[0], d])
          for j in js[1:]:
            s = s + np.float64(q[n, a, j, d])
          table[n, a, l, d] = s / np.float64(len(js))
        seen[n, a, l] = 1


# ---- the log column (safety_game_mo.py:797-804, 1201-1227) ------------------------------------------------------------------
_CONTEXT = decimal.Context(prec=10, rounding=decimal.ROUND_HALF_UP, capitals=0)      # safety_game_mo.py:398-400


def format_float(value):
  v = _CONTEXT.create_decimal_from_float(float(value))
  i = v.to_integral()
  return str(i if v == i else v.normalize())


def log_header(tile_types, dim_names):
  return ["tiletype_qvalue_%s_%s" % (t.strip(), d) for t in tile_types for d in dim_names]


def log_cells(table_row, n_types):
  """table_row float64 [L, D] of one (env, agent): the cells of its first n_types tile types (never reached: zeros, as the table starts)."""
  return [format_float(x) for l in range(n_types) for x in table_row[l]]


# ---- the fixtures of tests/golden/make_fixtures_qvalues.py ---------------------------------------------------------------------
FIXTURES = ("qvalues_island_L9", "qvalues_boat_L3", "qvalues_conveyor")


def load_fixture(name):
  """-> (dict of arrays, meta dict, csv rows as lists of str) of one reference run with the tiletype_qvalue column."""
  import ast
  import csv
  import os
  golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
  fx = np.load(os.path.join(golden, name + ".npz"))
  meta = {k[5:]: fx[k].item() for k in fx.files if k.startswith("meta_")}
  meta["kwargs"] = dict(ast.literal_eval(meta["kwargs"]))
  meta["tile_types"] = meta["tile_types"].split("|")
  meta["dim_names"] = meta["dim_names"].split("|")
  with open(os.path.join(golden, name + ".csv"), newline="") as f:
    rows = list(csv.reader(f, delimiter=";"))
  return {k: fx[k] for k in fx.files if not k.startswith("meta_")}, meta, rows


def bits(x):
  """float64 array -> its int64 bit patterns (comparisons are bit for bit)."""
  return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
