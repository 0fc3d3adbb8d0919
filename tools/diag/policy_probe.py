#!/usr/bin/env python3
"""Closed-loop stepping with a table policy: us per step of

  (a) BatchedEngine.policy_step_n replayed (sgw_policy_step_n: 2T + 1 launches, one graph replay per call),
  (b) a Python loop of BatchedEngine.act + BatchedEngine.step (the same two kernels, launched from the host),
  (c) a Python loop whose policy is the equivalent torch ops (index the table by the observation codes, sum over the cells,
      argmax) + BatchedEngine.step -- the only way to close the loop before sgw_policy_act existed,

on island_navigation_ex level 9, 65 536 envs, T = 64, source board, with one table (P = 1) and with 256 tables and a per-env
index (P = 256); k_policy_act alone (us per launch, 64 launches on a fixed observation per graph replay); and (a), (b) on firemaker_ex_ma, 16 384
envs, source views.  Every path runs `runs` times, alternating; a run is >= `seconds` of work between two device events after a
warm-up (the third identical policy_step_n call is the first replay).  (c) sums in torch's own order: it does the same work, not
the same bits.  criterion: every (a) run below every (c) run by more than 3 x the larger spread (max - min) of the two.

    python tools/diag/policy_probe.py [--out profiles/r14_policy.json] [--seconds 1.0] [--runs 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy
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


def spread(v):
  return dict(us=v, median_us=statistics.median(v), min_us=min(v), max_us=max(v), spread_us=max(v) - min(v))


def alternate(paths, steps_per_call, seconds, runs):
  """paths {name: fn}; returns {name: [us per step of each run]}, the paths alternated run by run."""
  reps = {k: reps_for(fn, seconds) for k, fn in paths.items()}
  got = {k: [] for k in paths}
  for _ in range(runs):
    for k, fn in paths.items():
      got[k].append(timed(fn, reps[k]) * 1e6 / (reps[k] * steps_per_call[k]))
  return {k: spread(v) for k, v in got.items()}, reps


ACT_PER_GRAPH = 64


def act_graph(eng, pol):
  """k_policy_act alone: ACT_PER_GRAPH act launches on the engine's current observation, captured once (launched one by one from
  the host they would measure the host's launch rate, not the kernel); returns the replay."""
  eng.act(pol)                                   # (the persistent result buffer exists before the capture)
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(ACT_PER_GRAPH):
      eng.act(pol)
  return g.replay


def random_policy(eng, source, P, seed):
  pol = TablePolicy(eng, source=source, n_policies=P, seed=seed, epsilon=0.05)
  g = torch.Generator(device="cpu"); g.manual_seed(seed)
  pol.weights.copy_(torch.randn(pol.weights.shape, generator=g))
  pol.bias.copy_(torch.randn(pol.bias.shape, generator=g))
  if P > 1:
    pol.set_policy_of_env(torch.arange(eng.n_envs, dtype=torch.int32) % P)
  return pol


def torch_policy(eng, pol):
  """The greedy part of the policy as torch ops on the engine's board output (A = 1): int8 [N] actions."""
  n, C = eng.n_envs, pol.cells
  code_of = pol.code_of.long()
  cells = torch.arange(C, device=DEV)[None, :]
  pidx = pol.policy_of_env.long()[:, None] if pol.policy_of_env is not None else None
  board = eng._bufs["board"]

  def fn():
    codes = code_of[board[:n].long()]                                            # [N, C]
    if pidx is None:
      terms = pol.weights[0, 0][cells, codes]                                    # [N, C, NA]
      score = terms.sum(dim=1) + pol.bias[0, 0]
    else:
      terms = pol.weights[pidx, 0, cells, codes]
      score = terms.sum(dim=1) + pol.bias[pidx[:, 0], 0]
    return (score.argmax(dim=1) + pol.action_lo).to(torch.int8)
  return fn


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--seconds", type=float, default=1.0)
  ap.add_argument("--runs", type=int, default=3)
  ap.add_argument("--n", type=int, default=65536)
  ap.add_argument("--T", type=int, default=64)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("policy_probe: no HIP device (a measurement path does not fall back)")
  T, rows = a.T, []
  spec = make_spec("island_navigation_ex", level=9)
  for P in (1, 256):
    eng = BatchedEngine(spec, a.n, device=DEV)
    eng.reset()
    pol = random_policy(eng, "board", P, 7)
    greedy = torch_policy(eng, pol)

    def path_a():
      eng.policy_step_n(pol, T)

    def path_b():
      for t in range(T):
        eng.step(eng.act(pol, t=t))

    def path_c():
      for t in range(T):
        eng.step(greedy())

    # the same policy either way where nobody explores: the torch ops choose what the kernel chooses up to the order of the sum
    pol.set_epsilon(0.0)
    agree = float((eng.act(pol).reshape(-1) == greedy()).float().mean().item())
    pol.set_epsilon(0.05)
    act_alone = act_graph(eng, pol)
    res, reps = alternate({"a_policy_step_n": path_a, "b_act_step_loop": path_b, "c_torch_step_loop": path_c, "k_policy_act_alone": act_alone},
                          {"a_policy_step_n": T, "b_act_step_loop": T, "c_torch_step_loop": T, "k_policy_act_alone": ACT_PER_GRAPH}, a.seconds, a.runs)
    A_, C_ = res["a_policy_step_n"], res["c_torch_step_loop"]
    margin = C_["min_us"] - A_["max_us"]
    row = dict(env="island_navigation_ex level 9", n_envs=a.n, T=T, source="board", n_policies=P, n_codes=pol.n_codes, n_actions=pol.n_actions,
               table_bytes=pol.weights.numel() * 4, greedy_agreement_with_torch=agree, calls_per_run=reps, **res,
               criterion=dict(a_max_us=A_["max_us"], c_min_us=C_["min_us"], margin_us=margin, larger_spread_us=max(A_["spread_us"], C_["spread_us"]),
                              holds=bool(margin > 3 * max(A_["spread_us"], C_["spread_us"]))))
    rows.append(row)
    print(json.dumps(row))
    eng.close()
  # windows as the observation: firemaker_ex_ma, every agent its own window (5 x 5, 5 x 5, 33 x 33)
  fspec = make_spec("firemaker_ex_ma")
  n2 = 16384
  fm = BatchedEngine(fspec, n2, device=DEV, outputs=("board", "reward", "step_type", "term_reason", "views"))
  fm.seed_rng(base=1)
  fm.reset()
  fpol = random_policy(fm, "views", 1, 9)

  def fm_a():
    fm.policy_step_n(fpol, T)

  def fm_b():
    for t in range(T):
      fm.step(fm.act(fpol, t=t))

  fm_act = act_graph(fm, fpol)
  res, reps = alternate({"a_policy_step_n": fm_a, "b_act_step_loop": fm_b, "k_policy_act_alone": fm_act},
                        {"a_policy_step_n": T, "b_act_step_loop": T, "k_policy_act_alone": ACT_PER_GRAPH}, a.seconds, a.runs)
  row = dict(env="firemaker_ex_ma (default)", n_envs=n2, T=T, source="views", n_policies=1, n_codes=fpol.n_codes, n_actions=fpol.n_actions,
             view_shapes=[list(s) for s in fspec.view_shapes], table_bytes=fpol.weights.numel() * 4, calls_per_run=reps, **res,
             c_torch_step_loop="not measured")
  rows.append(row)
  print(json.dumps(row))
  fm.close()
  out = dict(what="closed-loop stepping with a table policy: us per step; (a) policy_step_n replayed, (b) Python loop of act + step, (c) Python "
             "loop of torch ops + step; k_policy_act alone in us per launch; every path %d runs of >= %.1f s between device events, alternating"
             % (a.runs, a.seconds), device=torch.cuda.get_device_name(0), rows=rows)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(out, f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
