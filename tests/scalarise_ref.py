"""The reference's scalarisation restated as explicit loops (safety_game_mo.py:1027-1066): `s = 0.0; for x in row: s = s + x`,
an IEEE double addition per column, column 0 first.  The loop, not the builtin sum(): Python 3.12 compensates sum() over floats,
and these tests must not depend on the interpreter that runs them.  Shared by the CPU and the GPU tier."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ("island_L9", "boat_ex_L3")
# name -> (env name of the batched framework, its constructor arguments)
ENVS = {"island_L9": ("island_navigation_ex", dict(level=9)), "boat_ex_L3": ("boat_race_ex", dict(level=3))}
# two agents: the arrays carry an agent axis in the library's column layout; the env and its arguments are in the file
MA_CONFIGS = ("firemaker_a2", "savanna_a2")


def ma_env(z):
  """(env name, constructor arguments) of a two-agent fixture."""
  import ast
  return str(z["meta_family"]), dict(ast.literal_eval(str(z["meta_kwargs"])))


def load(name):
  with np.load(os.path.join(GOLDEN, "scalarise_%s.npz" % name)) as z:
    return {k: z[k] for k in z.files}


def loop_sum(row):
  s = np.float64(0.0)
  for x in np.asarray(row, np.float64).reshape(-1):
    s = s + x
  return s


def loop_sums(a, k=None):
  """Left-to-right sums over the first k entries of the last axis of `a` (float64), one Python addition at a time."""
  a = np.asarray(a, np.float64)
  k = a.shape[-1] if k is None else k
  flat = a.reshape(-1, a.shape[-1])
  out = np.empty(flat.shape[0], np.float64)
  with np.errstate(all="ignore"):
    for i in range(flat.shape[0]):
      out[i] = loop_sum(flat[i, :k])
  return out.reshape(a.shape[:-1])


def loop_averages(cumulative, frame, k=None):
  """sum([x / (frame + 1) for x in row]): the sum of the quotients, left to right."""
  c = np.asarray(cumulative, np.float64)
  d = (np.asarray(frame).astype(np.int64) + 1).astype(np.float64)
  with np.errstate(all="ignore"):
    q = c / d.reshape(d.shape + (1,) * (c.ndim - d.ndim))
  return loop_sums(q, k)


def same_bits(a, b):
  """Bit-for-bit equality of two float64 arrays (NaN payloads and the sign of zero included)."""
  a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
  return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())
