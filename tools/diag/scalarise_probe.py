#!/usr/bin/env python3
"""k_scalarise beside k_derived_stats -- the yardstick: it reads the same `reward` / `cumulative` / `frame` rows -- at 65 536 envs of
island_navigation_ex level 9 (T = 1), alternated in one process after 16 real steps.  Meant to run under a kernel trace of its own,

    rocprofv3 --kernel-trace --stats -d <dir> -o trace --output-format csv -- python tools/diag/scalarise_probe.py

whose per-kernel durations are the figures of profiles/README.md (profiles/r12_scalarise_kernel_stats.csv); the HIP-event
launch-to-launch times it prints itself include the host's enqueue cost (and the tracer's, under the tracer).
Per env and agent the kernel reads 16 K + 4 bytes and writes 24."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec


def main():
  n, reps = 65536, 400
  e = BatchedEngine(make_spec("island_navigation_ex", level=9), n, outputs=("reward", "cumulative", "frame", "step_type"))
  e.reset()
  acts = e.fill_actions(16, 5)
  for t in range(16):
    e.step(acts[t])
  for _ in range(20):      # warm-up: code objects, result tensors
    e.scalarise()
    e.derived_stats()
  torch.cuda.synchronize()
  out = {}
  for name, fn in (("scalarise", e.scalarise), ("derived_stats", e.derived_stats)):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
      fn()
    b.record()
    torch.cuda.synchronize()
    out[name] = a.elapsed_time(b) * 1e3 / reps
  K, A = e.spec.K, e.spec.A
  nbytes = n * A * (16 * K + 4 + 24)
  print("launch-to-launch us: scalarise %.2f derived_stats %.2f; k_scalarise moves %.2f MB per launch" % (
      out["scalarise"], out["derived_stats"], nbytes / 1e6))
  s = e.scalarise()
  print("nonzero scalar_cumulative: %d of %d" % (int((s["scalar_cumulative"] != 0).sum().item()), n))
  e.close()


if __name__ == "__main__":
  main()
