#!/usr/bin/env python3
"""What each action would do, timed: us per call, launched from Python, on island_navigation_ex level 9 at 65 536 envs, of

  (a) BatchedEngine.simulate_moves                     one launch: targets, tiles and the action mask of all 5 actions,
  (b) simulate_moves + fold_q_values (D = K)           two launches: (a) and the per-tile-type Q-value table,
  (c) BatchedEngine.lookahead with B = n_actions       the only way to learn "what would action j do" before (a) existed:
                                                       per action one state copy and one full step of a fork,
  (d) one plain BatchedEngine.step                     for scale.

Every path runs `runs` times, alternating; a run is >= `seconds` of calls between two device events after a warm-up.  The envs
stand a few random steps into their episodes; (a) - (c) leave the state where it is, so every call does the same work.
condition: every (a) run is faster than every (c) run.

    python tools/time_whatif.py [--out profiles/r15_whatif.json] [--envs 65536] [--seconds 0.5] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.specs import make_spec

DEV = "cuda:0"


def timed(fn, reps):
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ev0.record()
  for _ in range(reps):
    fn()
  ev1.record()
  ev1.synchronize()
  return ev0.elapsed_time(ev1) * 1e-3          # seconds


def reps_for(fn, seconds):
  """Warm up, then how many calls fill `seconds`."""
  for _ in range(4):
    fn()
  torch.cuda.synchronize()
  once = timed(fn, 8) / 8
  return max(8, int(seconds / once) + 1)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--envs", type=int, default=65536)
  ap.add_argument("--seconds", type=float, default=0.5)
  ap.add_argument("--runs", type=int, default=3)
  args = ap.parse_args()
  spec = make_spec("island_navigation_ex", level=9)
  n, NA = args.envs, spec.n_actions
  eng = BatchedEngine(spec, n, device=DEV, outputs=("board", "reward", "step_type", "term_reason", "agent_pos", "agent_flags"))
  eng.reset()
  tape = eng.fill_actions(16, 3)
  for t in range(8):
    eng.step(tape[t])
  q = torch.randn((n, 1, NA, spec.K), dtype=torch.float64, device=DEV)
  cand = torch.arange(NA, dtype=torch.int8, device=DEV)[:, None].expand(NA, n).contiguous()
  step_actions = tape[8]

  def both():
    eng.simulate_moves()
    eng.fold_q_values(q)

  paths = {"simulate_moves": eng.simulate_moves, "simulate_moves+fold_q_values": both,
           "lookahead_B=n_actions": lambda: eng.lookahead(cand)}
  reps = {k: reps_for(fn, args.seconds) for k, fn in paths.items()}
  got = {k: [] for k in paths}
  for _ in range(args.runs):
    for k, fn in paths.items():
      got[k].append(timed(fn, reps[k]) / reps[k] * 1e6)
  # the plain step moves the envs on: timed last, over the tape, so that the paths above all saw one state
  step = lambda: eng.step(step_actions)
  r = reps_for(step, args.seconds)
  got["step"] = [timed(step, r) / r * 1e6 for _ in range(args.runs)]
  res = {"env": "island_navigation_ex level 9", "envs": n, "n_actions": NA, "D": spec.K, "device": torch.cuda.get_device_name(0),
         "unit": "us per call, launched from Python, between device events", "runs": args.runs, "seconds_per_run": args.seconds,
         "paths": {k: dict(us=v, median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in got.items()}}
  res["simulate_moves_faster_than_lookahead"] = max(got["simulate_moves"]) < min(got["lookahead_B=n_actions"])
  text = json.dumps(res, indent=1)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")
  eng.close()
  return 0 if res["simulate_moves_faster_than_lookahead"] else 1


if __name__ == "__main__":
  sys.exit(main())
