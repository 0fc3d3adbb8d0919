"""The flag fixtures of tests/flag_fixtures.py (numeric rule parameters, reward values, lopsided observation windows; each a
recorded run of the reference) played through every launch path that takes the caller's actions: sgw_step_n as direct launches,
sgw_step_n as a replayed graph, and the fused sgw_replay.  Every field the reference run recorded and the engine writes is
compared with the fixture bit for bit, NaN for NaN, the agent windows and the generator position among them.  The fixtures' own
E <= 24 and T <= 160 are the shapes."""
import numpy as np
import pytest
import torch

from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec
from tests import flag_fixtures as FF
from tests import launch_paths as LP

pytestmark = pytest.mark.gpu

ORACLE = {"island_ex": "scalar", "ma": "ma", "ima": "ima", "sav": "sav"}      # the layout launch_paths.oracle_mismatches reads
OUTS = {"scalar": LP.ALL_OUTPUTS, "ma": LP.WIN, "ima": LP.WIN, "sav": LP.SAV}
RESET = -128
# steps per call.  step_n: fewer than the graph cache's minimum of 8, so every call is plain launches; step_n_graph: the same
# buffer refilled in place, so the second call captures and every later one replays; replay: a whole stretch between two
# explicit resets in one fused launch
CHUNK = {"step_n": 5, "step_n_graph": 10, "replay": None}


def _stretches(fx, multi):
  """[(first tick, ticks)] between the explicit resets of the tape (the same ticks in every stream), and the reset ticks."""
  acts = fx["actions"]
  T = acts.shape[1]
  ticks = [t for t in range(T) if multi and acts[0, t, 0] == RESET]
  for t in ticks:
    assert (acts[:, t, 0] == RESET).all()
  edges = [-1] + ticks + [T]
  return [(a + 1, b - a - 1) for a, b in zip(edges[:-1], edges[1:]) if b - a - 1 > 0], ticks


@pytest.mark.parametrize("path", sorted(CHUNK))
@pytest.mark.parametrize("name", sorted(FF.ROWS))
def test_flag_fixture_on_every_caller_action_path(name, path):
  family = FF.ROWS[name][0]
  fx, kwargs = FF.load(name)
  spec = make_spec(FF.FAMILIES[family][0], **kwargs)
  kind = ORACLE[family]
  E, T = fx["actions"].shape[:2]
  row = dict(id=name, name=spec.name, oracle=kind, n=E, outs=OUTS[kind])
  want = {k: fx[k] for k in fx.files if not k.startswith("meta_")}
  eng = BatchedEngine(spec, E, device=LP.DEV, outputs=row["outs"])
  if kind != "scalar":
    eng.set_rng_state(fx["rng_init"] if kind == "ma" else fx["rng_seeded"])
  acts = torch.from_numpy(np.ascontiguousarray(np.moveaxis(fx["actions"], 0, 1))).to(LP.DEV)       # [T, E(, A)]
  off = LP.resets(row) - 1                       # fixture slot of step s: s + off

  def check(o, stacked, s0, what):
    got = LP.to_np({k: v.clone() for k, v in o.items()}, stacked)
    views = LP.split_views(spec, got["views"]) if "views" in got else None
    bad = LP.oracle_mismatches(row, spec, got, want, s0, views=views)
    S = got["board"].shape[1]
    if "obs_board" in want and not LP._same(got["obs_board"].reshape(E, S, -1), want["obs_board"][:, s0 + off:s0 + off + S].reshape(E, S, -1)):
      bad.append("obs_board")
    assert not bad, "%s %s %s (steps %d..%d) differs from the reference run in %s" % (name, path, what, s0, s0 + S - 1, bad)

  check(LP.start(eng, row), False, 0, "reset")
  stretches, ticks = _stretches(fx, kind in ("ima", "sav"))
  bufs = {}
  for t0, n in stretches:
    if t0 - 1 in ticks:
      check(eng.reset(), False, t0, "explicit reset")
    step = CHUNK[path] or n
    for k in range(0, n, step):
      m = min(step, n - k)
      tape = acts[t0 + k:t0 + k + m]
      if path == "replay":
        o = eng.replay(tape.contiguous(), write_every=True)
      else:
        buf = bufs.setdefault(m, torch.empty_like(tape))
        buf.copy_(tape)
        o = eng.step_n(buf, write_every=True)
      check(o, True, 1 + t0 + k, "call at tick %d" % (t0 + k))
  assert stretches[-1][0] + stretches[-1][1] == T
  if kind != "scalar":
    state = eng.get_state()[:, :E].cpu().numpy()
    assert not LP.rng_mismatch(row, state, want, T), "%s %s: generator position after the tape" % (name, path)
  eng.close()
