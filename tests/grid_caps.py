"""The capped launches of csrc/sgw_api.hip: which kernels walk their work in a stride loop, and at which shapes the loop makes a
second and a third trip.  No GPU here: constants() reads the named caps from the source text, one function per launch restates the
host's grid arithmetic in a few lines, and ROWS gives every capped launch the shape tests/test_grid_caps_gpu.py runs it at (LARGE:
at least three trips, the last one ragged) next to the largest shape the rest of the suite uses (OLD: one trip).
tests/test_grid_caps.py holds the table to the source; a new capped launch gets a row here.

A "strider" is what owns one loop: a thread (the byte-per-thread kernels), a wave (a window or a load of planes per wave) or a
workgroup (a group of envs, an env, a tile).  max_trips / min_trips are the most and the fewest trips any strider of the launch
makes; `partial` says whether the last unit of work is cut short (None where a unit cannot be: a whole window, a whole env)."""
import collections
import os
import re

from ai_safety_gridworlds_amd.specs import make_spec
from tests import policy_gpu_util as U
from tests import policy_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ai_safety_gridworlds_amd", "csrc")
SOURCES = (os.path.join(CSRC, "sgw_api.hip"), os.path.join(CSRC, "sgw_learn.hpp"), os.path.join(CSRC, "sgw_common.hpp"))
SGW_H = os.path.join(REPO, "include", "sgw.h")

CAP_PATTERN = r"\w+_MAX_BLOCKS"          # the naming pattern of a grid cap; LEARN_BLOCKS (older) is the one exception
BUDGET = 256 << 20                       # device bytes a test may hold (a condition of the suite, not a measurement)
LDS_LIMIT = 64 * 1024                    # the `lds <= 64 * 1024` of the window launches
B_ENVS = 131                             # distinct envs a per-env test repeats: a prime, so no power-of-two stride maps an env onto itself
MAX_AGENTS = 4

Trips = collections.namedtuple("Trips", "workgroups min_trips max_trips partial stride extra")


def _ceil(a, b):
  return -(-a // b)


def _r16(x):
  return (x + 15) // 16 * 16


_CONSTANTS = {}


def constants():
  """{name: int} of every `constexpr int NAME = <integer expression>` of the launch sources, and SGW_MAX_CELLS of sgw.h."""
  if _CONSTANTS:
    return _CONSTANTS
  out = _CONSTANTS
  for path in SOURCES:
    for decl in re.findall(r"constexpr\s+int\s+([^;]+);", open(path).read()):
      for name, value in re.findall(r"(\w+)\s*=\s*([^,;]+)", decl):
        if re.fullmatch(r"[\d\s*+<()-]+", value):
          out[name] = int(eval(value))               # digits and arithmetic signs only
  m = re.search(r"#define\s+SGW_MAX_CELLS\s+(\d+)", open(SGW_H).read())
  assert m, "SGW_MAX_CELLS not found in include/sgw.h"
  out["SGW_MAX_CELLS"] = int(m.group(1))
  return out


def const(name):
  c = constants()
  assert name in c, "%s is not a named constant of %s" % (name, ", ".join(os.path.basename(p) for p in SOURCES))
  return c[name]


def cap_names():
  """Every constant that follows the naming pattern, and LEARN_BLOCKS."""
  return sorted(n for n in constants() if re.fullmatch(CAP_PATTERN, n)) + ["LEARN_BLOCKS"]


def _strided(units, striders, workgroups, partial, stride, **extra):
  return Trips(workgroups, units // striders, _ceil(units, striders), partial, stride, extra)


# ---- the windows ------------------------------------------------------------------------------------------------------------------
def view_total(radii):
  return sum((r[0] + r[1] + 1) * (r[2] + r[3] + 1) for r in radii if r is not None)


def _all_small(radii):
  return all((r[0] + r[1] + 1) * (r[2] + r[3] + 1) <= const("WAVE") for r in radii if r is not None)


def views_path(H, W, radii):
  """The kernel sgw_agent_views launches."""
  if _all_small(radii):
    return "k_agent_views_small"
  G = const("AGENT_VIEWS_LDS_GROUP_ENVS")
  lds = 128 + 16 * G + G * (_r16(H * W) + _r16(view_total(radii)) + 16)
  return "k_agent_layer_views_lds<4>" if lds <= LDS_LIMIT else "k_agent_views"


def layer_views_path(H, W, radii, L):
  """The kernel sgw_agent_layer_views launches."""
  if _all_small(radii):
    return "k_agent_layer_views_small"
  lds = 128 + 16 + _r16(L * H * W) + _r16(view_total(radii) * L) + 16
  return "k_agent_layer_views_lds<1>" if lds <= LDS_LIMIT else "k_agent_layer_views"


def _byte_threads(total, cap, threads=256):
  blocks = min(_ceil(total, threads), cap)
  return blocks, blocks * threads


def views_small(n, H, W, radii):
  total = n * view_total(radii)                                      # one thread per output byte
  blocks, striders = _byte_threads(total, const("AGENT_VIEWS_SMALL_MAX_BLOCKS"))
  return _strided(total, striders, blocks, total % 256 != 0, striders)


def layer_views_small(n, H, W, radii, L):
  total = n * view_total(radii) * L
  blocks, striders = _byte_threads(total, const("AGENT_LAYER_VIEWS_SMALL_MAX_BLOCKS"))
  return _strided(total, striders, blocks, total % 256 != 0, striders)


def views_lds(n, H, W, radii):
  G = const("AGENT_VIEWS_LDS_GROUP_ENVS")                            # a one-wave workgroup takes G envs per trip
  groups = _ceil(n, G)
  blocks = min(groups, const("AGENT_VIEWS_LDS_MAX_BLOCKS"))
  return _strided(groups, blocks, blocks, n % G != 0, blocks * G)


def layer_views_lds(n, H, W, radii, L):
  blocks = min(n, const("AGENT_LAYER_VIEWS_LDS_MAX_BLOCKS"))         # a workgroup per env
  return _strided(n, blocks, blocks, None, blocks)


def _window_waves(windows, cap):
  blocks, threads = _byte_threads(windows * const("WAVE"), cap)      # a wave per window, four waves per workgroup
  return _strided(windows, threads // const("WAVE"), blocks, None, threads // const("WAVE"))


def layer_views_wave(n, H, W, radii, L):
  return _window_waves(n * len(radii) * L, const("AGENT_LAYER_VIEWS_WAVE_MAX_BLOCKS"))


def views_wave(n, H, W, radii):
  return _window_waves(n * len(radii), const("AGENT_VIEWS_WAVE_MAX_BLOCKS"))


def views_wave_cheapest_two_trips():
  """(n, view bytes per env, output bytes) of the cheapest shape at which k_agent_views makes a second trip: more windows than the
  capped grid has waves, with the most agents an env has, and the shortest row that no longer fits the LDS kernel next to the
  largest board."""
  waves = const("AGENT_VIEWS_WAVE_MAX_BLOCKS") * 256 // const("WAVE")
  n = waves // MAX_AGENTS + 1
  G, lay = const("AGENT_VIEWS_LDS_GROUP_ENVS"), _r16(const("SGW_MAX_CELLS"))
  total = 1
  while 128 + 16 * G + G * (lay + _r16(total) + 16) <= LDS_LIMIT:
    total += 1
  return n, total, n * total


# ---- coordinates ------------------------------------------------------------------------------------------------------------------
def plane_coords(items, max_cells):
  """items planes of at most max_cells cells (sgw_layer_coords: n * L of H * W; sgw_agent_layer_coords: n * A * L of the largest
  window)."""
  need = (max_cells + 3 + 3) // 4
  seg_shift = 0
  while (1 << seg_shift) < need and seg_shift < 6:
    seg_shift += 1
  per_wave = const("WAVE") >> seg_shift
  waves = _ceil(items, per_wave)
  blocks = min(_ceil(waves, 4), const("PLANE_COORDS_MAX_BLOCKS"))
  return _strided(waves, blocks * 4, blocks, items % per_wave != 0, blocks * 4 * per_wave, seg_shift=seg_shift, per_wave=per_wave)


# ---- actions and tables -----------------------------------------------------------------------------------------------------------
def fill_actions(T, n, A):
  total = T * n * A
  blocks, striders = _byte_threads(total, const("FILL_ACTIONS_MAX_BLOCKS"))
  return _strided(total, striders, blocks, total % 256 != 0, striders)


def learn_geometry(geo, P):
  """What sgw_policy_* read of a tests/policy_gpu_util geometry with the test policies' alphabet (layer characters + WIN + code 0)."""
  name, kw, source = U.GEOMETRIES[geo]
  spec = make_spec(name, **kw)
  c_a, off_a, row = policy_ref.geometry(spec, source)
  return dict(row_bytes=row, c_a=c_a, A=spec.A, C=max(c_a), G=len(spec.layer_chars) + 2, NA=int(spec.n_actions), P=P)


def policy_apply(row_bytes, c_a, A, C, G, NA, P, with_bias=True):
  total = P * A * C * G * NA + (P * A * NA if with_bias else 0)
  blocks, striders = _byte_threads(total, const("POLICY_APPLY_MAX_BLOCKS"), const("LEARN_THREADS"))
  return _strided(total, striders, blocks, total % const("LEARN_THREADS") != 0, striders, elements=total)


def policy_accumulate(n, T, row_bytes, c_a, A, C, G, NA, P):
  E = 64
  while E > 16 and E * row_bytes > const("LEARN_MAX_ROW_LDS"):
    E >>= 1
  assert E * row_bytes <= const("LEARN_MAX_ROW_LDS")
  max_c = max([1] + list(c_a))
  R = max_c                                                          # P > 1: no bins, a slice per agent
  if P == 1:
    R = min((const("LEARN_MAX_BIN_LDS") - NA * 8) // (G * NA * 8), max_c)
  slices = sum(max(_ceil(c, R), 1) for c in c_a)
  groups = _ceil(n, E)
  tiles = groups * T
  per_slice = min(max(const("LEARN_BLOCKS") // slices, 1), tiles)
  return _strided(tiles, per_slice, per_slice * slices, n % E != 0, per_slice, E=E, R=R, slices=slices, per_slice=per_slice, tiles=tiles,
                  in_lds=P == 1)


# ---- the table --------------------------------------------------------------------------------------------------------------------
R4 = lambda r: (r, r, r, r)
SMALL_RADII = [(3, 4, 3, 4), (3, 4, 3, 4), None, (3, 3, 3, 3)]        # 8 x 8, 8 x 8, none, 7 x 7: 177 bytes per env (odd: a ragged last wave)
LDS_RADII = [R4(4), None]                                            # one 9 x 9 window (> 64 cells), an agent without one
WAVE_RADII = [(6, 7, 6, 7)] * 4                                      # four 14 x 14 windows


def _views_bytes(n, H, W, radii, L=0):
  """Device bytes of a window test: boards or layer planes, positions, flags, the output."""
  A = len(radii)
  return n * (H * W * max(L, 1) + 3 * A + view_total(radii) * max(L, 1))


def _coords_bytes(n, planes_per_env, cells, cap):
  return n * planes_per_env * (cells + 4 + 4 * cap)


def _learn_bytes(n, T, g):
  table = g["P"] * g["A"] * (g["C"] * g["G"] + 1) * g["NA"]
  return (T + 1) * (n + 63) // 64 * 64 * g["row_bytes"] + T * n * g["A"] * 9 + 12 * table


def _row(id, entry, kernel, caps, fn, large, old, nbytes, covered=True, per_env=None, path=None, why=None):
  return dict(id=id, entry=entry, kernel=kernel, caps=caps, fn=fn, large=large, old=old, bytes=nbytes, covered=covered, per_env=per_env,
              path=path, why=why)


def rows():
  """One row per capped launch (three for k_policy_accumulate's three ways through its tile loop).  `large` / `old`: the keyword
  arguments of `fn`; `per_env`: work items of one env in the units of Trips.stride, for the tests that repeat B_ENVS envs; `path`:
  the dispatch the shape must take; `bytes`: the device bytes of the large shape."""
  old_small = dict(n=65, H=6, W=8, radii=[R4(2), R4(2)])
  old_lds = dict(n=65, H=17, W=17, radii=[R4(2), R4(2), R4(16)])
  out = [
      _row("views_small", "sgw_agent_views", "k_agent_views_small", ["AGENT_VIEWS_SMALL_MAX_BLOCKS"], views_small,
           dict(n=200003, H=8, W=8, radii=SMALL_RADII), old_small, lambda s: _views_bytes(**s), per_env=view_total(SMALL_RADII),
           path=lambda s: views_path(s["H"], s["W"], s["radii"])),
      _row("layer_views_small", "sgw_agent_layer_views", "k_agent_layer_views_small", ["AGENT_LAYER_VIEWS_SMALL_MAX_BLOCKS"],
           layer_views_small, dict(n=22003, H=8, W=8, radii=SMALL_RADII, L=9), dict(old_small, L=9), lambda s: _views_bytes(**s),
           per_env=view_total(SMALL_RADII) * 9, path=lambda s: layer_views_path(s["H"], s["W"], s["radii"], s["L"])),
      _row("views_lds", "sgw_agent_views", "k_agent_layer_views_lds<4>", ["AGENT_VIEWS_LDS_MAX_BLOCKS", "AGENT_VIEWS_LDS_GROUP_ENVS"],
           views_lds, dict(n=70003, H=10, W=10, radii=LDS_RADII), old_lds, lambda s: _views_bytes(**s), per_env=1,
           path=lambda s: views_path(s["H"], s["W"], s["radii"])),
      _row("layer_views_lds", "sgw_agent_layer_views", "k_agent_layer_views_lds<1>", ["AGENT_LAYER_VIEWS_LDS_MAX_BLOCKS"], layer_views_lds,
           dict(n=9001, H=10, W=10, radii=LDS_RADII, L=3), dict(old_lds, L=9), lambda s: _views_bytes(**s), per_env=1,
           path=lambda s: layer_views_path(s["H"], s["W"], s["radii"], s["L"])),
      # rows of 4 * 196 * 64 = 50 176 bytes next to 64 * 320 = 20 480 bytes of planes: 70 KB, no LDS kernel takes them
      _row("layer_views_wave", "sgw_agent_layer_views", "k_agent_layer_views", ["AGENT_LAYER_VIEWS_WAVE_MAX_BLOCKS"], layer_views_wave,
           dict(n=2053, H=16, W=20, radii=WAVE_RADII, L=64), dict(n=20, H=13, W=13, radii=[R4(16), R4(16)], L=32),
           lambda s: _views_bytes(**s), per_env=4 * 64, path=lambda s: layer_views_path(s["H"], s["W"], s["radii"], s["L"])),
      _row("views_wave", "sgw_agent_views", "k_agent_views", ["AGENT_VIEWS_WAVE_MAX_BLOCKS"], views_wave, None,
           dict(n=20, H=17, W=17, radii=[R4(45), R4(45)]), None, covered=False, path=lambda s: views_path(s["H"], s["W"], s["radii"]),
           why="a second trip needs more than 65 536 * 4 windows, so more than 65 536 envs of at most 4 agents, and the launch is only "
               "reached by rows of about 16 KB (4 envs' boards and rows over 64 KiB of LDS): over 1 GB of output"),
      _row("plane_coords", "sgw_layer_coords", "k_plane_coords<false>", ["PLANE_COORDS_MAX_BLOCKS"], plane_coords,
           dict(items=60013 * 9, max_cells=25), dict(items=130 * 32, max_cells=289), lambda s: _coords_bytes(60013, 9, 25, 25), per_env=9),
      _row("plane_coords_rel", "sgw_agent_layer_coords", "k_plane_coords<true>", ["PLANE_COORDS_MAX_BLOCKS"], plane_coords,
           dict(items=60013 * 9, max_cells=25), dict(items=130 * 2 * 2, max_cells=33 * 33), lambda s: _coords_bytes(60013, 9, 25, 25),
           per_env=9),
      _row("fill_actions", "sgw_fill_actions", "k_fill_actions", ["FILL_ACTIONS_MAX_BLOCKS"], fill_actions, dict(T=257, n=4099, A=2),
           dict(T=17, n=1000, A=4), lambda s: s["T"] * s["n"] * s["A"]),
      _row("policy_apply", "sgw_policy_apply", "k_policy_apply", ["POLICY_APPLY_MAX_BLOCKS"], policy_apply, learn_geometry("firemaker_views", 12),
           learn_geometry("firemaker_views", 3), lambda s: 12 * (s["P"] * s["A"] * (s["C"] * s["G"] + 1) * s["NA"])),
  ]
  for id, geo, P, n, T, old_n, old_T in (("accumulate_lds_one_slice", "island_l9_board", 1, 2100, 65, 70, 5),
                                         ("accumulate_lds_sliced_window", "firemaker_views", 1, 70, 30, 70, 5),
                                         ("accumulate_global_atomics", "island_ma_board", 3, 650, 100, 70, 5)):
    g = learn_geometry(geo, P)
    out.append(_row(id, "sgw_policy_accumulate", "k_policy_accumulate", ["LEARN_BLOCKS"], policy_accumulate, dict(g, n=n, T=T),
                    dict(g, n=old_n, T=old_T), lambda s: _learn_bytes(s["n"], s["T"], s)))
    out[-1]["geo"] = geo
  return out


ROWS = rows()
BY_ID = {r["id"]: r for r in ROWS}
