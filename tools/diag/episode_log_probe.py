"""Times sgw_log_episodes beside what a caller had before on the same buffers: torch.nonzero on step_type (a host
synchronisation: the number of rows is read back) and an index_select per field.

    python tools/diag/episode_log_probe.py [--out profiles/r08_episode_log.json] [--launches 200]

65 536 island_navigation_ex envs, the [N_pad] buffers of one step (T = 1) and the [T, N_pad] buffers of 32 steps written by
step_n (T = 32), 40 random steps in, so the buffers hold episodes ending at the rate of a run in progress.  Every call sits
between its own pair of HIP events on the stream; 30 warm-up calls, then the median and the 10th / 90th percentile over --launches
timed ones.  The log is cleared (its counter zeroed) outside the timed pairs, so every timed call appends at 0.  The torch path's
time between its events includes the host's wait for nonzero's row count; its host time per call is reported too (the log's
host time is the one library call).  There is no pass mark: the log's point is that it is deterministic, sync-free and capturable."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from ai_safety_gridworlds_amd.engine import ALL_OUTPUTS, BatchedEngine, EpisodeLog      # noqa: E402
from ai_safety_gridworlds_amd.specs import make_spec                                  # noqa: E402

FIELDS = {"length": "frame", "term_reason": "term_reason", "ret": "cumulative", "hidden": "hidden", "metrics": "metrics"}


def timed(fn, launches, before=None, warmup=30):
  for _ in range(warmup):
    if before:
      before()
    fn()
  torch.cuda.synchronize()
  ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
  host = []
  for a, b in ev:
    if before:
      before()
    a.record()
    t0 = time.perf_counter()
    fn()
    host.append(time.perf_counter() - t0)
    b.record()
  torch.cuda.synchronize()
  us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
  return {"median_us": round(float(np.median(us)), 2), "p10_us": round(float(np.percentile(us, 10)), 2),
          "p90_us": round(float(np.percentile(us, 90)), 2), "host_median_us": round(float(np.median(host)) * 1e6, 2), "launches": launches}


def torch_path(eng, T):
  """What a caller does today: the ended rows by nonzero (synchronises), then one index_select per field."""
  rows = T * eng.n_pad
  st = eng._bufs["step_type"].reshape(rows, -1)
  live = (torch.arange(rows, device=eng.device) % eng.n_pad) < eng.n_envs
  flat = {f: eng._bufs[s].reshape(rows, -1) for f, s in FIELDS.items()}

  def run():
    idx = torch.nonzero((st[:, 0] == 2) & live).reshape(-1)
    out = {f: v.index_select(0, idx) for f, v in flat.items()}
    out["env"], out["step"] = idx % eng.n_pad, idx // eng.n_pad
    return out
  return run


def probe(n, T, launches):
  spec = make_spec("island_navigation_ex", level=9)
  eng = BatchedEngine(spec, n, outputs=ALL_OUTPUTS)
  eng.reset()
  eng.step_n(eng.fill_actions(40, 3))
  acts = eng.fill_actions(T, 3, step0=40)
  if T > 1:
    eng.step_n(acts, write_every=True)
  else:
    eng.step(acts[0])
  log = EpisodeLog(eng, T * n)
  eng.log_episodes(log)
  episodes = log.count()
  run = torch_path(eng, T)
  ref, rec = run(), log.records()
  assert len(ref["env"]) == episodes
  for f in ("env", "step", "length", "hidden", "ret", "metrics", "term_reason"):      # both paths produce the same records
    a, b = (x.reshape(episodes, -1) for x in (rec[f], ref[f]))
    assert torch.equal(*(x.view(torch.int64) if x.dtype == torch.float64 else x.to(torch.int64) for x in (a, b))), f      # bits: metrics hold NaNs
  res = {"n_envs": n, "T": T, "episodes_in_the_buffers": episodes, "record_bytes": 4 + 8 + 4 + 1 + 8 * spec.K + 8 + 8 * spec.M,
         "sgw_log_episodes (3 launches)": timed(lambda: eng.log_episodes(log), launches, before=log.clear),
         "torch.nonzero + index_select per field": timed(run, launches)}
  eng.close()
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--launches", type=int, default=200)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("episode_log_probe: no HIP device; there is nothing to time on a CPU")
  res = {"device": torch.cuda.get_device_name(0),
         "method": "one HIP event pair per call; 30 warm-up calls; median, p10, p90; host_median_us: host time inside the call",
         "env": "island_navigation_ex level 9", "runs": [probe(65536, 1, args.launches), probe(65536, 32, args.launches)]}
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
