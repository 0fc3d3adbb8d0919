"""Times sgw_layer_coords / sgw_agent_layer_coords beside the launches that produce their input bytes (sgw_observe_layers,
sgw_agent_layer_views) and beside the host path a user had before (layers.cpu().numpy() + np.argwhere per env and layer).

    python tools/diag/coords_probe.py [--out profiles/r05_coords.json] [--launches 300]

Every launch sits between its own pair of HIP events on the stream (the time between them is the kernel plus ~1 us of event
overhead, whatever the host does meanwhile); 30 warm-up launches, then the median and the 10th / 90th percentile over
--launches timed ones.  The envs are stepped 12 random rounds first, so the planes hold a game in progress."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ai_safety_gridworlds_amd.engine import BatchedEngine      # noqa: E402
from ai_safety_gridworlds_amd.specs import make_spec          # noqa: E402


def timed(fn, launches, warmup=30):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
  for a, b in ev:
    a.record(); fn(); b.record()
  torch.cuda.synchronize()
  us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
  return {"median_us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2),
          "p90_us": round(float(np.percentile(us, 90)), 2), "launches": launches}


def host_argwhere(layers):
  t0 = time.perf_counter()
  a = layers.cpu().numpy()
  out = [[np.argwhere(a[i, l]) for l in range(a.shape[1])] for i in range(a.shape[0])]
  return time.perf_counter() - t0, out


def probe(name, n, launches, agents, **kw):
  spec = make_spec(name, **kw)
  eng = BatchedEngine(spec, n, outputs=("board", "reward", "step_type", "agent_pos", "agent_flags"))
  if spec.family == 4 or getattr(spec, "needs_rng", False):
    eng.set_rng_seeds(np.arange(n))
  eng.reset()
  rng = np.random.default_rng(0)
  for _ in range(12):
    eng.step(torch.from_numpy(rng.integers(spec.action_lo, spec.action_lo + spec.n_actions, (n, spec.A)).astype(np.int8)).cuda())
  layers = eng.observe_layers()
  L = layers.shape[1]
  out = eng.layer_coords(layers=layers)
  res = {"env": name, "n_envs": n, "layers": L, "board": [spec.H, spec.W],
         "set_cells_per_env": round(float(out[0].sum()) / n, 1),
         "sgw_observe_layers (producer)": timed(lambda: eng.observe_layers(), launches),
         "sgw_layer_coords": timed(lambda: eng.layer_coords(layers=layers, out=out), launches)}
  sec, ref = host_argwhere(layers)
  res["host: layers.cpu().numpy() + argwhere per env and layer"] = {"seconds": round(sec, 3)}
  counts, coords = out[0].cpu().numpy(), out[1].cpu().numpy()
  for i in range(0, n, max(1, n // 512)):                        # the timed kernel computed what the host path computes
    for l in range(L):
      assert counts[i, l] == len(ref[i][l]) and np.array_equal(coords[i, l, :counts[i, l]], ref[i][l]), (i, l)
  if agents:
    cubes = eng.agent_layer_views(layers=layers)
    cap = max(h * w for h, w in spec.view_shapes)
    aout = (torch.zeros((n, spec.A, L), dtype=torch.int32, device="cuda"), torch.zeros((n, spec.A, L, cap, 2), dtype=torch.int16, device="cuda"))
    res["windows"] = [list(s) for s in spec.view_shapes]
    res["sgw_agent_layer_views (producer)"] = timed(lambda: eng.agent_layer_views(layers=layers), launches)
    res["sgw_agent_layer_coords"] = timed(lambda: eng.agent_layer_coords(cubes, out=aout), launches)
    res["set_window_cells_per_env"] = round(float(aout[0].clamp(min=0).sum()) / n, 1)
  eng.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--launches", type=int, default=300)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("coords_probe: no HIP device; there is nothing to time on a CPU")
  res = {"device": torch.cuda.get_device_name(0), "method": "one HIP event pair per launch; 30 warm-up launches; median, p10, p90",
         "runs": [probe("island_navigation_ex", 65536, args.launches, False, level=9),
                  probe("firemaker_ex_ma", 16384, args.launches, True)]}
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
