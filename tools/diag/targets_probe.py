#!/usr/bin/env python3
"""td_targets beside the same rule written as a torch loop over T -- one set of elementwise ops per step, what a user can do
without sgw_td_targets -- at 65 536 envs of island_navigation_ex level 9, T = 128, K = 10, values given, bootstrap_truncated,
over the [T, N_pad, ...] buffers of one rollout(T, write_every=True):

    python tools/diag/targets_probe.py [--out profiles/r16_targets.json] [--envs 65536] [--T 128] [--reps 20] [--loop-reps 3]

Reports µs per call of both (HIP events around `reps` back-to-back calls after a warm-up, the median of --runs such timings),
whether the torch loop gives the kernel's bits, and the kernel's bytes moved / time as a fraction of 8 TB/s.  Bytes per call:
every (env, agent, column) of every step reads its reward and value and writes its return and advantage (32 bytes); every
(env, agent) of every step reads step_type and term_reason and writes valid (3 bytes); value0 once.  The register count comes
from the installed build's assembly (ai_safety_gridworlds_amd/libsgw.s) where it stands beside the library."""
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
from ai_safety_gridworlds_amd.specs import make_spec

MID, LAST, MAX_STEPS = 1, 2, 1
HBM_BYTES_PER_S = 8e12


def torch_loop(reward, step_type, term_reason, values, value0, gamma, lam, ret, adv, valid):
  """The rule of include/sgw.h (sgw_td_targets, BOOTSTRAP_TRUNCATED) with torch ops: reward / values / ret / adv [T, N, K],
  step_type / term_reason / valid [T, N]."""
  T = reward.shape[0]
  gl = gamma * lam
  carry_ret = values[T - 1]
  carry_adv = torch.zeros_like(carry_ret)
  zero = torch.zeros_like(carry_ret)
  for t in range(T - 1, -1, -1):
    st, r, v = step_type[t], reward[t], values[t]
    mid = (st == MID).unsqueeze(-1)
    last = st == LAST
    truncated = (last & (term_reason[t] == MAX_STEPS)).unsqueeze(-1)
    terminated = last.unsqueeze(-1) & ~truncated
    vprev = values[t - 1] if t > 0 else value0
    boot = r + gamma * v
    delta = boot - vprev
    ret_t = torch.where(mid, r + gamma * carry_ret, torch.where(truncated, boot, torch.where(terminated, r, zero)))
    adv_t = torch.where(mid, delta + gl * carry_adv, torch.where(truncated, delta, torch.where(terminated, r - vprev, zero)))
    ret[t] = ret_t
    adv[t] = adv_t
    valid[t] = (st == MID) | last
    carry_ret, carry_adv = ret_t, adv_t


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


def registers():
  if not os.path.exists(build.ASM):
    return None
  text = open(build.ASM).read()
  out = {}
  for key in ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size"):
    m = re.search(r"\.set \S*k_td_targets\S*\.%s, (\d+)" % key, text)
    out[key] = int(m.group(1)) if m else None
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--envs", type=int, default=65536)
  ap.add_argument("--T", type=int, default=128)
  ap.add_argument("--reps", type=int, default=20)
  ap.add_argument("--loop-reps", type=int, default=3)
  ap.add_argument("--runs", type=int, default=3)
  args = ap.parse_args()
  n, T = args.envs, args.T
  e = BatchedEngine(make_spec("island_navigation_ex", level=9), n, outputs=("reward", "step_type", "term_reason"))
  K, A = e.spec.K, e.spec.A
  e.reset()
  o = e.rollout(T, 0x5AFE, write_every=True)
  gen = torch.Generator(device=e.device).manual_seed(1)
  values = torch.randn((T, n, K), dtype=torch.float64, device=e.device, generator=gen)
  value0 = torch.randn((n, K), dtype=torch.float64, device=e.device, generator=gen)
  gamma_list = [(0.99, 1.0, 0.0, 0.5)[c % 4] for c in range(K)]
  lam = 0.95

  def call():
    return e.td_targets(T, gamma_list, lam, values=values, value0=value0, bootstrap_truncated=True)

  for _ in range(3):
    res = call()
  torch.cuda.synchronize()
  kernel_us = timed(call, args.reps, args.runs)

  reward, st, tr = o["reward"], o["step_type"][..., 0], o["term_reason"]
  gamma = torch.tensor(gamma_list, dtype=torch.float64, device=e.device)
  ret, adv = torch.empty_like(values), torch.empty_like(values)
  valid = torch.empty((T, n), dtype=torch.bool, device=e.device)
  loop = lambda: torch_loop(reward, st, tr, values, value0, gamma, lam, ret, adv, valid)
  loop()
  torch.cuda.synchronize()
  loop_us = timed(loop, args.loop_reps, args.runs)
  same = bool(torch.equal(ret.view(torch.int64), res["returns"].view(torch.int64)) and
              torch.equal(adv.view(torch.int64), res["advantages"].view(torch.int64)) and torch.equal(valid, res["valid"]))

  nbytes = T * n * A * (K * 32 + 3) + n * A * K * 8
  k_us, l_us = statistics.median(kernel_us), statistics.median(loop_us)
  row = {"env": "island_navigation_ex level 9", "envs": n, "T": T, "K": K, "values": True, "bootstrap_truncated": True,
         "td_targets_us_per_call": round(k_us, 2), "td_targets_us_runs": [round(x, 2) for x in kernel_us],
         "torch_loop_us_per_call": round(l_us, 2), "torch_loop_us_runs": [round(x, 2) for x in loop_us],
         "torch_loop_launches_per_call_about": 22 * T, "speedup": round(l_us / k_us, 2), "torch_loop_gives_the_same_bits": same,
         "bytes_per_call": nbytes, "hbm_fraction_of_8TBps": round(nbytes / (k_us * 1e-6) / HBM_BYTES_PER_S, 3),
         "valid_fraction": round(float(res["valid"].float().mean().item()), 4),
         "k_td_targets_registers": registers(),
         "how": "HIP events around back-to-back calls from Python after a warm-up; median of the runs; launch-to-launch, so the host's "
                "enqueue cost is inside (negligible at this size)"}
  print(json.dumps(row))
  if args.out:
    with open(args.out, "w") as f:
      json.dump(row, f, indent=1)
      f.write("\n")
  e.close()


if __name__ == "__main__":
  main()
