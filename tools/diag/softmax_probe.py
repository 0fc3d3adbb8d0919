#!/usr/bin/env python3
"""The softmax table policy beside its greedy twin and beside the same iteration written with torch ops, at 65 536 envs of
island_navigation_ex level 9, T = 128:

    python tools/diag/softmax_probe.py [--out profiles/r21_softmax.json] [--envs 65536] [--T 128] [--parent-library libsgw_parent.so]

Every figure is µs between two device events around back-to-back calls that together last at least --min-seconds, after a warm-up;
the two sides of a comparison alternate, --runs times, in the same session; the median is reported beside the runs.
  closed loop   policy_step_n per step: sampled (this build) against greedy (this build, whose k_policy_act is the parent's byte for
                byte; with --parent-library also a library built from the parent commit, run in a child process under SGW_LIBRARY,
                between the runs)
  acting alone  act() with a temperature (k_policy_sample) against act() without (k_policy_act)
  gradient      policy_accumulate_softmax against policy_accumulate over the same rollout and coefficients
  pg_learn      one iteration against the same iteration as torch ops: per step a gather-and-add score loop, softmax, multinomial
                and step(); then per step one index_add_ of coef * (one-hot - pi) into a float64 table (random coefficients, no
                td_targets: a weak baseline, dominated by the contended index_add_)
Also the registers of the new kernels from the installed build's assembly."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from ai_safety_gridworlds_amd import build
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec

KERNELS = ("k_policy_act", "k_policy_sample", "k_policy_scores", "k_policy_probs", "k_policy_accumulate", "k_policy_accumulate_softmax")


def timed(fn, min_seconds):
  """µs per call of fn over enough back-to-back calls to last min_seconds."""
  reps = 1
  while True:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
      fn()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b)
    if ms >= min_seconds * 1e3:
      return ms * 1e3 / reps
    reps = max(reps + 1, int(reps * min_seconds * 1.2e3 / max(ms, 1e-3)))


def registers(kernel):
  if not os.path.exists(build.ASM):
    return None
  text = open(build.ASM).read()
  out = {}
  for key in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size"):
    m = re.search(r"\.set \S*%s[A-Z]\S*\.%s, (\d+)" % (kernel, key), text)
    out[key] = int(m.group(1)) if m else None
  return out


def summary(runs):
  return {"us": round(statistics.median(runs), 3), "runs": [round(x, 3) for x in runs]}


def torch_scores(board, code_of, w, b):
  """board uint8 [N, C]; w float32 [C, G, NA]; b [NA] -> [N, NA], one gather and one addition per cell, in cell order."""
  codes = code_of.long()[board.long()]
  s = b.expand(board.shape[0], -1).clone()
  for c in range(board.shape[1]):
    s = s + w[c][codes[:, c]]
  return s


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--envs", type=int, default=65536)
  ap.add_argument("--T", type=int, default=128)
  ap.add_argument("--runs", type=int, default=3)
  ap.add_argument("--min-seconds", type=float, default=1.0)
  ap.add_argument("--parent-library", default=None)
  ap.add_argument("--greedy-only", action="store_true", help="(the child process of --parent-library) print the greedy closed loop's µs per step")
  args = ap.parse_args()
  n, T, tau = args.envs, args.T, 0.7
  spec = make_spec("island_navigation_ex", level=9)
  e = BatchedEngine(spec, n, outputs=("board", "reward", "step_type", "term_reason"))
  dev = e.device
  e.reset()
  gen = torch.Generator(device=dev).manual_seed(1)
  pol = TablePolicy(e, seed=3, epsilon=0.1)
  pol.weights.copy_(torch.randn(pol.weights.shape, device=dev, generator=gen) * 0.1)
  pol.bias.copy_(torch.randn(pol.bias.shape, device=dev, generator=gen))

  def loop(temperature):
    pol.set_temperature(temperature)
    for _ in range(3):                                       # direct, capture, replay
      e.policy_step_n(pol, T, write_every=True)
    return timed(lambda: e.policy_step_n(pol, T, write_every=True), args.min_seconds) / T

  if args.greedy_only:
    print(json.dumps({"greedy_us_per_step": loop(None)}))
    e.close()
    return

  row = {"env": "island_navigation_ex level 9", "envs": n, "T": T, "temperature": tau, "cells": pol.cells, "n_codes": pol.n_codes,
         "n_actions": pol.n_actions}
  greedy, sampled, parent = [], [], []
  for _ in range(args.runs):
    greedy.append(loop(None))
    if args.parent_library:
      env = dict(os.environ, SGW_LIBRARY=os.path.abspath(args.parent_library))
      out = subprocess.run([sys.executable, os.path.abspath(__file__), "--greedy-only", "--envs", str(n), "--T", str(T), "--min-seconds",
                            str(args.min_seconds)], env=env, capture_output=True, text=True, check=True, timeout=300).stdout
      parent.append(json.loads(out.strip().splitlines()[-1])["greedy_us_per_step"])
    sampled.append(loop(tau))
  base = statistics.median(parent or greedy)
  row["closed_loop_per_step"] = {"sampled": summary(sampled), "greedy_this_build": summary(greedy),
                                 "greedy_parent_build": summary(parent) if parent else None,
                                 "sampled_over_greedy": round(statistics.median(sampled) / base, 4)}

  act_g, act_s = [], []
  for _ in range(args.runs):
    pol.set_temperature(None); e.act(pol)
    act_g.append(timed(lambda: e.act(pol), args.min_seconds))
    pol.set_temperature(tau); e.act(pol)
    act_s.append(timed(lambda: e.act(pol), args.min_seconds))
  row["act_alone"] = {"k_policy_sample": summary(act_s), "k_policy_act": summary(act_g),
                      "ratio": round(statistics.median(act_s) / statistics.median(act_g), 4)}

  pol.set_temperature(tau)
  traj = e.policy_rollout(pol, T)
  obs0, obs, actions = traj["obs0"].clone(), e._bufs["board"].clone(), traj["actions"].clone()
  coef = torch.randn((T, n, 1), dtype=torch.float64, device=dev, generator=gen)
  acc_p, acc_s = [], []
  for _ in range(args.runs):
    for fn, runs in ((lambda: e.policy_accumulate(pol, coef, T, obs0, obs, actions), acc_p),
                     (lambda: e.policy_accumulate_softmax(pol, coef, T, obs0, obs, actions), acc_s)):
      fn()
      runs.append(timed(fn, args.min_seconds))
  pol.acc_weights.zero_(); pol.acc_bias.zero_(); pol.acc_frac_bits = None
  row["accumulate"] = {"softmax": summary(acc_s), "plain": summary(acc_p), "ratio": round(statistics.median(acc_s) / statistics.median(acc_p), 4),
                       "bin_additions_per_call_softmax": T * n * pol.cells * pol.n_actions, "bin_additions_per_call_plain": T * n * pol.cells}

  gamma, lr, NA = 0.99, 1e-3, pol.n_actions
  w64 = pol.weights[0, 0].double().clone()                   # the torch learner's own table [C, G, NA]
  b32 = pol.bias[0, 0].clone()

  def torch_pg():
    probs_t, acts_t, boards_t = [], [], []
    board = e.reset()["board"].reshape(n, -1).clone()
    w32 = w64.float()
    for t in range(T):
      s = torch_scores(board, pol.code_of, w32, b32)
      pi = torch.softmax(s / tau, dim=-1)
      a = torch.multinomial(pi, 1)
      probs_t.append(pi); acts_t.append(a); boards_t.append(board)
      board = e.step(a.to(torch.int8))["board"].reshape(n, -1).clone()
    return probs_t, acts_t, boards_t

  def torch_update(probs_t, acts_t, boards_t, coef_t):
    flat = w64.view(-1, NA)
    cells = torch.arange(pol.cells, device=dev).unsqueeze(0)
    for t in range(T):
      d = -probs_t[t].double()
      d.scatter_add_(1, acts_t[t], torch.ones((n, 1), dtype=torch.float64, device=dev))
      g = d * coef_t[t].reshape(n, 1) * lr
      idx = (cells * pol.n_codes + pol.code_of.long()[boards_t[t].long()]).reshape(-1)
      flat.index_add_(0, idx, g.unsqueeze(1).expand(-1, pol.cells, -1).reshape(-1, NA))

  def torch_iteration():
    probs_t, acts_t, boards_t = torch_pg()
    torch_update(probs_t, acts_t, boards_t, coef)           # (coefficients of the same shape; the returns' launch is not the difference)

  pg_d, pg_t = [], []
  for _ in range(args.runs):
    for _ in range(3):
      e.pg_learn(pol, T, gamma, lr)
    pg_d.append(timed(lambda: e.pg_learn(pol, T, gamma, lr), args.min_seconds))
    torch_iteration()
    pg_t.append(timed(torch_iteration, args.min_seconds))
  row["pg_learn"] = {"device": summary(pg_d), "torch_ops": summary(pg_t), "torch_over_device": round(statistics.median(pg_t) / statistics.median(pg_d), 2),
                     "us_per_transition_device": round(statistics.median(pg_d) / (T * n), 6),
                     "weights_finite": bool(torch.isfinite(pol.weights).all().item()),
                     "note": ("the torch side is the composition a user would write first (random coefficients, no td_targets); nearly all of "
                              "its time is the 128 float64 index_add_ calls of [N * cells, n_actions] rows into cells * n_codes bins, a "
                              "heavily contended atomic: a weak baseline, no measure of headroom")}
  row["registers"] = {k: registers(k) for k in KERNELS}
  row["how"] = ("device events around back-to-back calls from Python that last >= %.1f s, after a warm-up; the sides of a comparison alternate; "
                "median of %d runs; launch-to-launch, so the host's enqueue cost is inside" % (args.min_seconds, args.runs))
  print(json.dumps(row))
  if args.out:
    with open(args.out, "w") as f:
      json.dump(row, f, indent=1)
      f.write("\n")
  e.close()


if __name__ == "__main__":
  main()
