#!/usr/bin/env python3
"""Seeding the env generators: one BatchedEngine.seed_rng(base=...) call (sgw_seed_rng: one launch, timed to the end of a stream
synchronisation) against the host path set_rng_seeds(np.arange(N)) (numpy SeedSequence + PCG64 per env in Python, an upload,
sgw_set_rng_state), at the benchmark sizes of the three families with an env generator.  The two are alternated; both leave the
same state (checked word for word before anything is timed).

    python tools/diag/seed_rng_probe.py [--out profiles/r09_seed_rng.json] [--calls 300] [--host-reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np
import torch

from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec

CASES = (("firemaker_ex_ma", dict(amount_agents=3), 16384),
         ("island_navigation_ex_ma", dict(level=9, map_randomization_frequency=3), 65536),
         ("aintelope_savanna", dict(), 65536))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--calls", type=int, default=300)
  ap.add_argument("--host-reps", type=int, default=3)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("seed_rng_probe: no HIP device (a measurement path does not fall back)")
  rows = []
  for name, kw, n in CASES:
    eng = BatchedEngine(make_spec(name, **kw), n)
    stream = torch.cuda.current_stream()
    eng.set_rng_seeds(np.arange(n))
    want = eng.get_state().clone()
    eng.seed_rng(base=12345)
    eng.seed_rng(base=0)
    same = bool(torch.equal(eng.get_state(), want))
    dev_us, host_s = [], []
    for rep in range(a.host_reps):                 # alternate: a block of device calls, one host call
      for i in range(a.calls // a.host_reps):
        stream.synchronize()
        t0 = time.perf_counter()
        eng.seed_rng(base=i)
        stream.synchronize()
        dev_us.append((time.perf_counter() - t0) * 1e6)
      t0 = time.perf_counter()
      eng.set_rng_seeds(np.arange(n))              # ends in the library's own stream synchronisation
      host_s.append(time.perf_counter() - t0)
    # the launches alone, back to back between two device events
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    k = 2000
    ev0.record()
    for i in range(k):
      eng.seed_rng(base=i)
    ev1.record()
    ev1.synchronize()
    row = dict(family=name, n_envs=n, same_state=same,
               seed_rng_call_us_median=statistics.median(dev_us), seed_rng_call_us_min=min(dev_us), seed_rng_call_us_p90=sorted(dev_us)[int(0.9 * len(dev_us))],
               seed_rng_back_to_back_us=ev0.elapsed_time(ev1) * 1e3 / k,
               set_rng_seeds_s=host_s, set_rng_seeds_s_median=statistics.median(host_s),
               ratio=statistics.median(host_s) * 1e6 / statistics.median(dev_us))
    rows.append(row)
    print(json.dumps(row))
    eng.close()
  res = dict(what="seed_rng(base=...) + stream synchronise vs set_rng_seeds(np.arange(N)), alternated in one process", device=torch.cuda.get_device_name(0),
             calls=a.calls, host_reps=a.host_reps, rows=rows)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(res, f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
