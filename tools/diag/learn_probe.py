#!/usr/bin/env python3
"""The learning calls beside the same integers and floats computed with torch ops -- what a user can do without them -- at 65 536
envs of island_navigation_ex level 9, T = 128, over the buffers of one policy_rollout(T):

    python tools/diag/learn_probe.py [--out profiles/r17_learn.json] [--envs 65536] [--T 128] [--reps 10] [--torch-reps 2]

Reports µs per call (HIP events around `reps` back-to-back calls after a warm-up, the median of --runs such timings) of
policy_scores, policy_accumulate at P = 1 and P = 256, policy_apply and a whole q_learn iteration (its closed-loop chain replayed
from the engine's graph cache), each beside its torch statement and whether that gives the same bits:
  scores      per observation and cell one gather of the cell's [N, n_actions] table rows and one float32 addition, in cell order
  accumulate  quantise with torch ops, then per step one scatter_add_ on the flattened int64 table (N x C indices) and one on the bias
  apply       float64 arithmetic over the whole table, torch.where on acc != 0
  q_learn     policy_rollout + torch scores + td_targets + torch accumulate + torch apply
The torch statements do not call the code under test.  Also: the accumulate kernel's bytes read against the HBM floor (every
observation byte, coefficient and action once), its registers from the installed build's assembly, and its LDS bytes."""
import argparse
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from ai_safety_gridworlds_amd import build
from ai_safety_gridworlds_amd.engine import BatchedEngine
from ai_safety_gridworlds_amd.policy import TablePolicy
from ai_safety_gridworlds_amd.specs import make_spec

HBM_BYTES_PER_S = 8e12
FRAC = 24
Q_MAX = 2147483647.0


def timed(fn, reps, runs):
  out = []
  for _ in range(runs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
      fn()
    b.record()
    torch.cuda.synchronize()
    out.append(a.elapsed_time(b) * 1e3 / reps)
  return out


def registers(kernel):
  if not os.path.exists(build.ASM):
    return None
  text = open(build.ASM).read()
  out = {}
  for key in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size"):
    m = re.search(r"\.set \S*%s\S*\.%s, (\d+)" % (kernel, key), text)
    out[key] = int(m.group(1)) if m else None
  return out


def torch_scores(O, code_of, w, b, actions):
  """O uint8 [S, N, C]; w float32 [C, G, NA]; b [NA] -> scores [S, N, NA], vmax [S, N], chosen [S-1, N] (P = 1, A = 1)."""
  S, n, Cn = O.shape
  codes = code_of.long()[O.long()]                           # [S, N, C]
  s = b.expand(S, n, -1).clone()
  for c in range(Cn):
    s = s + w[c][codes[:, :, c]]
  vmax = s.max(dim=-1).values.double()
  j = actions.long()
  inside = (j >= 0) & (j < s.shape[-1])
  chosen = torch.where(inside, s[:-1].gather(-1, j.clamp(0, s.shape[-1] - 1).unsqueeze(-1))[..., 0].double(), torch.zeros((), dtype=torch.float64, device=O.device))
  return s, vmax, chosen


def torch_quantise(coef):
  x = coef * float(2 ** FRAC)
  q = torch.where(x >= Q_MAX, torch.full_like(x, Q_MAX), torch.where(x <= -Q_MAX, torch.full_like(x, -Q_MAX), torch.round(x)))
  return torch.where(torch.isnan(x), torch.zeros_like(x), q).long()


def torch_accumulate(acc_w, acc_b, O, code_of, p_of_env, actions, coef, G, NA):
  """acc_w int64 [P, C, G, NA], acc_b int64 [P, NA] (A = 1), one scatter_add_ per step."""
  T, n = actions.shape
  Cn = O.shape[-1]
  q = torch_quantise(coef)
  j = actions.long()
  q = torch.where((j >= 0) & (j < NA), q, torch.zeros_like(q))
  j = j.clamp(0, NA - 1)
  flat_w, flat_b = acc_w.view(-1), acc_b.view(-1)
  cells = torch.arange(Cn, device=O.device).unsqueeze(0)
  for t in range(T):
    codes = code_of.long()[O[t].long()]                      # [N, C]
    idx = ((p_of_env.unsqueeze(1) * Cn + cells) * G + codes) * NA + j[t].unsqueeze(1)
    flat_w.scatter_add_(0, idx.reshape(-1), q[t].unsqueeze(1).expand(-1, Cn).reshape(-1))
    flat_b.scatter_add_(0, p_of_env * NA + j[t], q[t])


def torch_apply(w, acc, lr):
  new = (w.double() + lr * (acc.double() * float(2.0 ** -FRAC))).float()
  w.copy_(torch.where(acc != 0, new, w))
  acc.zero_()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--envs", type=int, default=65536)
  ap.add_argument("--T", type=int, default=128)
  ap.add_argument("--reps", type=int, default=10)
  ap.add_argument("--torch-reps", type=int, default=2)
  ap.add_argument("--runs", type=int, default=3)
  ap.add_argument("--P", type=int, default=256)
  args = ap.parse_args()
  n, T = args.envs, args.T
  spec = make_spec("island_navigation_ex", level=9)
  e = BatchedEngine(spec, n, outputs=("board", "reward", "step_type", "term_reason"))
  dev = e.device
  e.reset()
  gen = torch.Generator(device=dev).manual_seed(1)
  row = {"env": "island_navigation_ex level 9", "envs": n, "T": T, "frac_bits": FRAC}

  def fresh_policy(P):
    pol = TablePolicy(e, n_policies=P, seed=3, epsilon=0.1)
    pol.weights.copy_(torch.randn(pol.weights.shape, device=dev, generator=gen) * 0.1)
    pol.bias.copy_(torch.randn(pol.bias.shape, device=dev, generator=gen))
    if P > 1:
      pol.set_policy_of_env(torch.arange(n, device=dev, dtype=torch.int32) % P)
    return pol

  pol = fresh_policy(1)
  Cn, G, NA = pol.cells, pol.n_codes, pol.n_actions
  row.update({"cells": Cn, "n_codes": G, "n_actions": NA})
  traj = e.policy_rollout(pol, T)
  obs0 = traj["obs0"].clone()
  obs = e._bufs["board"].clone()                             # [T, N_pad, C]
  actions = traj["actions"].clone()
  coef = torch.randn((T, n, 1), dtype=torch.float64, device=dev, generator=gen)
  O = torch.cat([obs0.unsqueeze(0), obs[:, :n]], dim=0)      # [T + 1, N, C] for the torch statements
  torch.cuda.synchronize()

  # -- scores
  call = lambda: e.policy_scores(pol, T, obs0, obs, actions)
  for _ in range(3):
    res = call()
  us = timed(call, args.reps, args.runs)
  ts = lambda: torch_scores(O, pol.code_of, pol.weights[0, 0], pol.bias[0, 0], actions[:, :, 0])
  want = ts()
  t_us = timed(ts, args.torch_reps, args.runs)
  same = bool(torch.equal(want[0].view(torch.int32), res["scores"][:, :, 0].view(torch.int32)) and
              torch.equal(want[1].view(torch.int64), res["vmax"][:, :, 0].view(torch.int64)) and
              torch.equal(want[2].view(torch.int64), res["chosen"][:, :, 0].view(torch.int64)))
  row["policy_scores"] = {"us_per_call": round(statistics.median(us), 2), "us_runs": [round(x, 2) for x in us],
                          "torch_us_per_call": round(statistics.median(t_us), 2), "torch_us_runs": [round(x, 2) for x in t_us],
                          "torch_gives_the_same_bits": same, "registers": registers("k_policy_scores")}

  # -- accumulate, P = 1 and P = args.P
  for P in (1, args.P):
    pp = pol if P == 1 else fresh_policy(P)
    p_of_env = torch.zeros(n, dtype=torch.int64, device=dev) if P == 1 else pp.policy_of_env.long()
    call = lambda: e.policy_accumulate(pp, coef, T, obs0, obs, actions, frac_bits=FRAC)
    pp.acc_weights.zero_(); pp.acc_bias.zero_()
    call()
    got_w, got_b = pp.acc_weights.clone(), pp.acc_bias.clone()
    for _ in range(2):
      call()
    us = timed(call, args.reps, args.runs)
    tw, tb = torch.zeros_like(pp.acc_weights[:, 0]), torch.zeros_like(pp.acc_bias[:, 0])
    ta = lambda: torch_accumulate(tw, tb, O, pp.code_of, p_of_env, actions[:, :, 0], coef[:, :, 0], G, NA)
    ta()
    same = bool(torch.equal(tw, got_w[:, 0]) and torch.equal(tb, got_b[:, 0]))
    t_us = timed(ta, args.torch_reps, args.runs)
    nbytes = T * n * (Cn + 8 + 1)
    med = statistics.median(us)
    lds = (64 * Cn + 15) // 16 * 16 + 256 + 64 * 12 + ((Cn * G * NA + NA) * 8 if P == 1 else 0)
    row["policy_accumulate_P%d" % P] = {
        "P": P, "us_per_call": round(med, 2), "us_runs": [round(x, 2) for x in us], "torch_us_per_call": round(statistics.median(t_us), 2),
        "torch_us_runs": [round(x, 2) for x in t_us], "torch_gives_the_same_integers": same, "bytes_read_per_call": nbytes,
        "hbm_floor_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2), "hbm_fraction_of_8TBps": round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 4),
        "bin_additions_per_call": T * n * Cn, "lds_bytes_per_workgroup": lds,
        "nonzero_bins": int((got_w != 0).sum().item()), "bins": got_w.numel()}
    pp.acc_weights.zero_(); pp.acc_bias.zero_(); pp.acc_frac_bits = None
  row["k_policy_accumulate_registers"] = registers("k_policy_accumulate")

  # -- apply
  acc_keep = torch.randint(-2 ** 36, 2 ** 36, pol.acc_weights.shape, dtype=torch.int64, device=dev, generator=gen)
  w_keep = pol.weights.clone()

  def apply_call():
    pol.acc_weights.copy_(acc_keep)
    e.policy_apply(pol, 0.01, clear=True)

  def refill():
    pol.acc_weights.copy_(acc_keep)

  for _ in range(3):
    apply_call()
  us, base = timed(apply_call, args.reps, args.runs), timed(refill, args.reps, args.runs)
  pol.weights.copy_(w_keep); apply_call()
  got = pol.weights.clone()
  tw_ = w_keep.clone()

  def torch_apply_call():
    acc = acc_keep.clone()
    torch_apply(tw_, acc, 0.01)

  torch_apply_call()
  same = bool(torch.equal(tw_.view(torch.int32), got.view(torch.int32)))
  t_us = timed(torch_apply_call, args.reps, args.runs)
  row["policy_apply"] = {"elements": pol.weights.numel(), "us_per_call_with_refill": round(statistics.median(us), 2),
                         "refill_copy_us": round(statistics.median(base), 2), "torch_us_per_call_with_clone": round(statistics.median(t_us), 2),
                         "torch_gives_the_same_bits": same, "registers": registers("k_policy_apply")}
  pol.weights.copy_(w_keep)

  # -- a whole q_learn iteration: the rollout chain is one graph replay from the third call on
  gamma, lr = 0.99, 1e-3
  for _ in range(4):
    e.q_learn(pol, T, gamma, lr)
  torch.cuda.synchronize()
  us = timed(lambda: e.q_learn(pol, T, gamma, lr), max(2, args.reps // 2), args.runs)

  def torch_q_learn():
    tr = e.policy_rollout(pol, T)
    Oq = torch.cat([tr["obs0"].unsqueeze(0), e._bufs["board"][:, :n]], dim=0)
    a = tr["actions"][:, :, 0]
    _, vmax, chosen = torch_scores(Oq, pol.code_of, pol.weights[0, 0], pol.bias[0, 0], a)
    td = e.td_targets(T, gamma, lam=0.0, values=vmax[1:].contiguous(), value0=vmax[0].contiguous(), scalar=True)
    delta = (td["advantages"].reshape(T, n) + vmax[:-1]) - chosen
    delta = torch.where(td["valid"].reshape(T, n), delta, torch.zeros((), dtype=torch.float64, device=dev))
    aw, ab = torch.zeros_like(pol.acc_weights[:, 0]), torch.zeros_like(pol.acc_bias[:, 0])
    torch_accumulate(aw, ab, Oq, pol.code_of, torch.zeros(n, dtype=torch.int64, device=dev), a, delta, G, NA)
    torch_apply(pol.weights[:, 0], aw, lr)
    torch_apply(pol.bias[:, 0], ab, lr)

  torch_q_learn()
  t_us = timed(torch_q_learn, args.torch_reps, args.runs)
  row["q_learn"] = {"us_per_iteration": round(statistics.median(us), 2), "us_runs": [round(x, 2) for x in us],
                    "us_per_transition": round(statistics.median(us) / (T * n), 6),
                    "torch_learner_us_per_iteration": round(statistics.median(t_us), 2), "torch_us_runs": [round(x, 2) for x in t_us],
                    "weights_finite": bool(torch.isfinite(pol.weights).all().item())}
  row["how"] = ("HIP events around back-to-back calls from Python after a warm-up; median of the runs; launch-to-launch, so the host's "
                "enqueue cost is inside")
  print(json.dumps(row))
  if args.out:
    with open(args.out, "w") as f:
      json.dump(row, f, indent=1)
      f.write("\n")
  e.close()


if __name__ == "__main__":
  main()
