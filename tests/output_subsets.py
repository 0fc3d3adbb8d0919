"""Output subsets for tests/test_output_subsets_gpu.py: `sgw_out` promises that any output pointer may be NULL, and in the
step kernels the set of requested outputs is the runtime mask KArgs::need from which the host derives the LDS layout of every
env-wave (csrc/sgw_common.hpp lds_plan): regions exist only for requested outputs, the parked cumulative vectors of the
CUM_IN_LDS families alias one of three other regions or get rows of their own, the board image is staged for four different
outputs, and the small outputs take a different route per launch path.  This module names the subsets every row of
tests/launch_paths.py is run with, says what each field must equal (the one-sgw_step-at-a-time record that
test_launch_paths_gpu.case() pins to the C oracle, plus plain numpy derivations of the fields that record does not hold), and
wraps every output buffer in guard bytes so that a store that leaves its buffer is seen.  Importing it needs no GPU."""
import numpy as np

from ai_safety_gridworlds_amd import _native as N
from ai_safety_gridworlds_amd.engine import DEFAULT_OUTPUTS, BatchedEngine

BENCH_OUTPUTS = ("board", "reward", "step_type", "term_reason", "safety", "frame")    # bench.py's headline output set
WINDOW_EXTRAS = ("obs_views", "obs_dir", "act_dir")
LEAVE_ONE_OUT = ("board", "obs_board", "reward", "cumulative", "metrics", "step_type", "views")
# the four layouts of the parked cumulative vectors (LdsPlan::cstash): inside the reward rows, the cumulative rows, the returns
# rows (accumulate on, neither of the two requested), rows of their own -- asked of every row, not only the CUM_IN_LDS families
CSTASH_SHAPES = ((("reward", "cumulative"), False), (("cumulative",), False), (("step_type",), True), (("step_type",), False))
# one more: the reward rows alone, with no rows behind them (accumulate off, `cumulative` not requested) -- parked vectors that
# missed the reward rows would land on the trash row, the flag words and the small outputs
MORE_SHAPES = ((("reward",), False),)
WINDOW_SHAPES = (("views", "obs_views"), ("board", "views"), ("obs_board", "obs_views"), ("done", "obs_dir", "act_dir"))
N_RANDOM = 8
# (row id, launch path or None for every path, outputs, accumulate): subsets that once exposed a bug, kept by name
REGRESSIONS = ()


def is_window_row(row):
  return "views" in row["outs"]


def full_outputs(row, spec):
  """The row's outputs plus `done`, and for the families with agent windows `obs_views`, `obs_dir` and `act_dir`."""
  out = list(row["outs"])
  for f in ("done",) + (WINDOW_EXTRAS if is_window_row(row) else ()):
    if f not in out:
      out.append(f)
  return tuple(out)


def subsets(row, spec, path=None):
  """The deterministic list of (outputs, accumulate) a row is run with; outputs in the order of full_outputs."""
  from tests import launch_paths as LP
  full = full_outputs(row, spec)
  order = {f: i for i, f in enumerate(full)}
  out, seen = [], set()

  def add(fields, acc):
    e = (tuple(sorted(set(fields), key=order.__getitem__)), bool(acc))
    assert all(f in order for f in e[0]), "%s: %s holds a field the row does not have" % (row["id"], fields)
    if e in seen:
      return False
    seen.add(e)
    out.append(e)
    return True

  for f in full:                                            # every field alone
    add((f,), True)
  add((), True)                                             # the state-only launches
  add((), False)
  for f in LEAVE_ONE_OUT:
    if f in order:
      add([g for g in full if g != f], True)
  for fields, acc in CSTASH_SHAPES + MORE_SHAPES:
    add(fields, acc)
  if is_window_row(row):
    for fields in WINDOW_SHAPES:
      add(fields, True)
  add(DEFAULT_OUTPUTS, True)
  if row["name"] == "island_navigation_ex":
    add(BENCH_OUTPUTS, True)
  rs = np.random.default_rng(LP.ROWS.index(row))
  n = 0
  while n < N_RANDOM:                                       # each field kept with probability 1/2, the flag a coin flip
    keep = rs.random(len(full)) < 0.5
    n += add([f for f, k in zip(full, keep) if k], rs.random() < 0.5)
  for rid, p, fields, acc in REGRESSIONS:
    if rid == row["id"] and (p is None or path is None or p == path):
      add(fields, acc)
  return out


def expected(c, field):
  """The expected [E, S + 1, ...] array of a field from the cached case `c` (test_launch_paths_gpu.case): the row's own fields
  straight from the sgw_step record c["ref"], the others derived from fields it holds."""
  ref = c["ref"]
  if field == "done":
    return (ref["step_type"] >= 2).astype(np.uint8)
  if field == "obs_dir":
    return ((ref["agent_flags"] >> 3) & 3).astype(np.uint8)
  if field == "act_dir":
    return ((ref["agent_flags"] >> 1) & 3).astype(np.uint8)
  if field == "obs_views":
    value_map = np.array(list(c["spec"].native.value_map), dtype=np.float32)
    assert value_map.shape == (128,)
    return value_map[ref["views"] & 0x7f]
  return ref[field]


def first_difference(got, want):
  """got, want: [S, E, ...] arrays (time-major, as the engine returns them) -> (env, step index) of the first difference in
  (step, env) order, or None; NaN == NaN."""
  bad = ~((got == want) | ((got != got) & (want != want)))
  bad = bad.reshape(bad.shape[0], bad.shape[1], -1).any(axis=2)
  if not bad.any():
    return None
  t, e = np.argwhere(bad)[0]
  return int(e), int(t)


GUARD = 4096          # bytes on each side of an output buffer: keeps the 16-byte alignment the drains assume
FILL = 0xA5


class GuardedEngine(BatchedEngine):
  """A BatchedEngine whose every output buffer is the middle of a larger uint8 tensor with GUARD bytes of FILL on each side.  The
  middle has the dtype and shape BatchedEngine allocates and its pointer goes into sgw_out, so the library sees nothing
  different.  guards_intact() names the buffers whose guard bytes changed (of every allocation the engine has made).  The rows
  from N up to N_pad belong to the buffer and are scratch by contract: they are not checked."""

  def _alloc_outputs(self, T):
    self._broken = getattr(self, "_broken", set()) | set(self._broken_now())       # the buffers about to be replaced: a last look
    self._raw = {}
    BatchedEngine._alloc_outputs(self, T)

  def _new_output(self, name, dtype, shape):
    """The dtype and shape BatchedEngine asks for, as the zeroed middle of a guarded allocation."""
    import torch
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=self.device)
    raw[GUARD:GUARD + nbytes].zero_()
    self._raw[name] = (raw, nbytes)
    buf = raw[GUARD:GUARD + nbytes].view(dtype).reshape(shape)
    assert buf.data_ptr() == raw.data_ptr() + GUARD and buf.data_ptr() % 16 == 0
    return buf

  def _broken_now(self):
    import torch
    raws = getattr(self, "_raw", None)
    if not raws:
      return []
    names = sorted(raws)
    flags = torch.stack([((raws[k][0][:GUARD] != FILL).any() | (raws[k][0][GUARD + raws[k][1]:] != FILL).any()) for k in names])
    return [k for k, f in zip(names, flags.cpu().numpy()) if f]

  def guards_intact(self):
    """Names of the output buffers next to which a guard byte changed; empty: every store stayed inside its buffer."""
    return sorted(getattr(self, "_broken", set()) | set(self._broken_now()))


def make_guarded(row, spec, inp, outputs):
  """launch_paths.make_engine with a GuardedEngine and these outputs; not reset."""
  from tests.launch_paths import DEV
  eng = GuardedEngine(spec, row["n"], device=DEV, outputs=tuple(outputs))
  if inp["bits"] is not None or inp["bits_seed"]:
    eng.set_episode_bits(inp["bits"], seed=inp["bits_seed"])
  if inp["rand"] is not None or inp["rand_seed"]:
    eng.set_random_stream(inp["rand"], seed=inp["rand_seed"])
  if inp["rng"] is not None:
    eng.set_rng_state(inp["rng"])
  return eng


# ---- the CPU tier's geometries (tests/host_shim/lds_plan_check.cpp) ------------------------------------------------------
CUM_IN_LDS_FAMILIES = (N.ISLAND_NAVIGATION_EX_MA, N.AINTELOPE_SAVANNA)


def view_chunk(vb, want):
  """csrc/sgw_common.hpp lds_view_chunk restated: the smallest of 8 / 16 / 32 / 64 envs that is at least `want` and makes the
  chunk's rows a whole number of 16-byte stores."""
  g = 8
  while g < 64 and (g < want or (g * vb) % 16):
    g *= 2
  return g


def plan_geometries(row, spec):
  """The `HW A K M pa vb cs vg` lines of a row for the plan checker: vg = 64 and whatever chunk lds_view_chunk can return."""
  A, K = spec.A, spec.K
  pa = A if getattr(spec, "per_agent", False) else 1
  cs = A * K if spec.family in CUM_IN_LDS_FAMILIES else 0
  vb = int(sum(h * w for (h, w) in spec.view_shapes))
  vgs = sorted({64} | ({view_chunk(vb, w) for w in (8, 16, 32)} if vb else set()))
  return [(spec.H * spec.W, A, K, spec.M, pa, vb, cs, vg) for vg in vgs]
