#!/usr/bin/env python3
"""Forking envs: BatchedEngine.copy_envs (sgw_copy_envs: one launch) against the only route there was before it -- get_state ->
torch indexing -> set_state, plus one torch copy (identity) or index_copy_ (permutation) per output -- at 65 536 envs of default
island_navigation_ex with every output allocated: a full identity copy and a random-permutation copy, each with and without the
output rows; then one lookahead(B = 5) against set_state + step + clone per candidate on a second engine.  The two routes are
alternated in blocks inside one process and leave the same bytes (checked before anything is timed).  A block is `calls` calls
back to back between two device events; every block's time per call is kept, so the spread is in the file.

bytes = (state words * 8 + the rows of the copied outputs) * n, read and written; `hbm_fraction` is bytes / time over the 8 TB/s
HBM peak -- at this size (about 0.2 GB both ways with outputs, 10 MB without) the buffers fit the 256 MiB Infinity Cache, so it is a
rate against that yardstick, not a claim about HBM traffic.

    python tools/diag/copy_envs_probe.py [--out profiles/r11_copy_envs.json] [--n 65536] [--calls 200] [--blocks 7]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch

from ai_safety_gridworlds_amd.engine import ALL_OUTPUTS, BatchedEngine, _dtype_shape
from ai_safety_gridworlds_amd.specs import make_spec

HBM_PEAK = 8.0e12


def timed(fn, calls):
  """us per call of `calls` calls back to back between two device events."""
  ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  ev0.record()
  for _ in range(calls):
    fn()
  ev1.record()
  ev1.synchronize()
  return ev0.elapsed_time(ev1) * 1e3 / calls


def alternate(new, old, calls, blocks):
  for fn in (new, old):                       # warm both routes at the shapes of the timed window
    for _ in range(3):
      fn()
  torch.cuda.synchronize()
  a, b = [], []
  for _ in range(blocks):
    a.append(timed(new, calls))
    b.append(timed(old, max(calls // 10, 5)))
  return a, b


def spread(v):
  return dict(us=v, median_us=statistics.median(v), min_us=min(v), max_us=max(v))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--n", type=int, default=65536)
  ap.add_argument("--calls", type=int, default=200)
  ap.add_argument("--blocks", type=int, default=7)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("copy_envs_probe: no HIP device (a measurement path does not fall back)")
  n, dev = a.n, "cuda:0"
  spec = make_spec("island_navigation_ex")
  src = BatchedEngine(spec, n, device=dev, outputs=ALL_OUTPUTS)
  dst = BatchedEngine(spec, n, device=dev, outputs=ALL_OUTPUTS)
  src.reset(); dst.reset()
  src.rollout(24, 3); dst.rollout(9, 4)
  src.step(src.fill_actions(1, 5)[0]); dst.step(dst.fill_actions(1, 6)[0])       # (plain [N_pad, ...] rows of one step)
  words = int(src._lib.sgw_state_words(src._h))
  state_bytes = words * 8
  row_bytes = sum(_dtype_shape(spec, k)[0].itemsize * int(torch.Size(_dtype_shape(spec, k)[1]).numel()) for k in ALL_OUTPUTS
                  if not (k == "metrics" and spec.M == 0))
  g = torch.Generator(device="cpu"); g.manual_seed(1)
  perm = torch.randperm(n, generator=g)
  ident = torch.arange(n)
  rows = []
  for label, sidx in (("identity", ident), ("permutation", perm)):
    si32, di32 = sidx.to(dev, torch.int32), ident.to(dev, torch.int32)
    si64, di64 = sidx.to(dev), ident.to(dev)
    for with_out in (True, False):
      if label == "identity":
        def new():
          dst.copy_envs(src, outputs=with_out)

        def old():
          dst.set_state(src.get_state())
          if with_out:
            for k in ALL_OUTPUTS:
              dst._bufs[k].copy_(src._bufs[k])
      else:
        def new():
          dst.copy_envs(src, src_idx=si32, dst_idx=di32, outputs=with_out)

        def old():
          st, d = src.get_state(), dst.get_state()
          d[:, di64] = st[:, si64]
          dst.set_state(d)
          if with_out:
            for k in ALL_OUTPUTS:
              dst._bufs[k].index_copy_(0, di64, src._bufs[k].index_select(0, si64))
      # the same bytes either way
      dst.rollout(3, 9); dst.step(dst.fill_actions(1, 7)[0])
      keep_s, keep_b = dst.get_state().clone(), {k: v.clone() for k, v in dst._bufs.items()}
      new()
      got_s, got_b = dst.get_state().clone(), {k: v.clone() for k, v in dst._bufs.items()}
      dst.set_state(keep_s)
      for k, v in keep_b.items():
        dst._bufs[k].copy_(v)
      old()
      equal = bool(torch.equal(dst.get_state()[:, :n], got_s[:, :n])) and all(
          torch.equal(dst._bufs[k][:n].view(torch.uint8), got_b[k][:n].view(torch.uint8)) for k in ALL_OUTPUTS)
      t_new, t_old = alternate(new, old, a.calls, a.blocks)
      nbytes = 2 * n * (state_bytes + (row_bytes if with_out else 0))
      row = dict(case=label, outputs=with_out, n_envs=n, same_bytes=equal, bytes_moved=nbytes, copy_envs=spread(t_new), baseline=spread(t_old),
                 ratio=statistics.median(t_old) / statistics.median(t_new),
                 bytes_per_s=nbytes / (statistics.median(t_new) * 1e-6), hbm_fraction=nbytes / (statistics.median(t_new) * 1e-6) / HBM_PEAK)
      rows.append(row)
      print(json.dumps(row))
  # one-step lookahead over B = 5 candidate action sets, end to end (to the end of a synchronisation)
  B = 5
  cand = src.fill_actions(B, 11)
  other = BatchedEngine(spec, n, device=dev, outputs=ALL_OUTPUTS)
  stacked = {k: torch.empty((B,) + tuple(v.shape), dtype=v.dtype, device=dev) for k, v in other.reset().items()}

  def look_new():
    src.lookahead(cand)

  def look_old():
    snap = src.get_state()
    for b in range(B):
      other.set_state(snap)
      for k, v in other.step(cand[b]).items():
        stacked[k][b].copy_(v)

  res = src.lookahead(cand)
  look_old()
  equal = all(torch.equal(res[k].reshape(-1).view(torch.uint8), stacked[k].reshape(-1).view(torch.uint8)) for k in ALL_OUTPUTS)
  t_new, t_old = alternate(look_new, look_old, max(a.calls // 5, 10), a.blocks)
  row = dict(case="lookahead", B=B, n_envs=n, same_bytes=equal, lookahead=spread(t_new), baseline=spread(t_old),
             ratio=statistics.median(t_old) / statistics.median(t_new))
  rows.append(row)
  print(json.dumps(row))
  out = dict(what="copy_envs vs get_state -> torch index -> set_state + a torch copy per output; lookahead(B=5) vs set_state + step + clone per "
             "candidate; us per call, blocks of back-to-back calls between device events, the two routes alternated in one process",
             device=torch.cuda.get_device_name(0), env="island_navigation_ex (default)", state_words=words, state_bytes_per_env=state_bytes,
             output_row_bytes_per_env=row_bytes, calls_per_block=a.calls, blocks=a.blocks, hbm_peak_bytes_per_s=HBM_PEAK, rows=rows)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      json.dump(out, f, indent=1)
      f.write("\n")
  for e in (src, dst, other):
    e.close()


if __name__ == "__main__":
  main()
