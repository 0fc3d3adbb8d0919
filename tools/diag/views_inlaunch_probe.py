"""Agent windows larger than the board: the round with the windows written by its own launch (sgw_out.views) beside the round
without windows and the round followed by sgw_agent_views, for each chunk size G of the in-launch assembly.

    python tools/diag/views_inlaunch_probe.py [--out profiles/r06_views_inlaunch.json] [--launches 200] [--runs 3]
                                              [--sweep-library libsgw_knob.so --chunks 8,16,32,64]
                                              [--baseline-library /path/to/parent/libsgw.so]

Configurations: aintelope_savanna with default flags (21 x 21 windows on 13 x 13), one and two agents, and
island_navigation_ex_ma with observation_radius [3, 3, 3, 3] (7 x 7 = 49 cells on 6 x 8 = 48), 65 536 envs each, with the
outputs the Zoo vector env asks for.  Every launch (the pair of launches in the third case) sits between its own pair of HIP
events; 30 warm-up launches, then the median and the 10th / 90th percentile over --launches timed ones.  The installed library runs
its compiled-in chunk size ("installed"); the sweep over G needs a diagnostic build that reads SGW_VIEWS_CHUNK
(hipcc <build.FLAGS> -DSGW_VIEWS_CHUNK_KNOB -o libsgw_knob.so csrc/sgw_api.hip), given as --sweep-library.  Every measurement runs
in a child process of its own; --runs alternates the installed library with --baseline-library (the parent commit's build) for
the round without windows.  Each case also records the dynamic LDS per workgroup the launch asks for (sgw_step_lds_bytes) and,
with the step kernel's registers from the installed build's assembly, the workgroups a CU keeps resident."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ROUND = ("board", "reward", "cumulative", "step_type", "term_reason", "discount", "metrics", "agent_pos", "agent_flags", "done")
CONFIGS = [("aintelope_savanna/1 agent", "aintelope_savanna", dict()),
           ("aintelope_savanna/2 agents", "aintelope_savanna", dict(amount_agents=2)),
           ("island_navigation_ex_ma/radius 3", "island_navigation_ex_ma", dict(observation_radius=[3, 3, 3, 3]))]


def child(n, launches, cases):
  """One process = one library and one chunk size: {config: {case: timing}} as a JSON line."""
  import ctypes as C
  import numpy as np
  import torch
  from ai_safety_gridworlds_amd import _native as N
  from ai_safety_gridworlds_amd.engine import BatchedEngine
  from ai_safety_gridworlds_amd.specs import make_spec

  def timed(fn, warmup=30):
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

  m = (1 << 64) - 1                                          # per-env numpy streams, as BatchedEngine.set_rng_seeds builds them (once)
  words = np.empty((n, 4), np.uint64)
  for i in range(n):
    st = np.random.PCG64(np.random.SeedSequence(i)).state["state"]
    words[i] = (st["state"] >> 64, st["state"] & m, st["inc"] >> 64, st["inc"] & m)
  res = {}
  for label, name, kw in CONFIGS:
    spec = make_spec(name, **kw)
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(rng.integers(spec.action_lo, spec.action_lo + spec.n_actions, (n, spec.A)).astype(np.int8)).cuda() for _ in range(16)]
    r = {"windows": [list(s) for s in spec.view_shapes], "board": [spec.H, spec.W]}
    for case, outs in (("round", ROUND), ("round_with_views", ROUND + ("views",)), ("round_then_sgw_agent_views", ROUND)):
      if case not in cases:
        continue
      eng = BatchedEngine(spec, n, outputs=outs)
      eng.set_rng_state(words)
      k = [0]
      def step():
        eng.step_ptr(acts[k[0] & 15].data_ptr()); k[0] += 1
      try:
        if hasattr(eng._lib, "sgw_step_lds_bytes"):             # (a baseline library may predate it)
          r[case + "_lds_bytes"] = int(eng._lib.sgw_step_lds_bytes(eng._h, C.byref(eng._out)))
        eng.reset()
        for _ in range(12):
          step()
        if case == "round_then_sgw_agent_views":
          buf = torch.empty((n, int(eng._lib.sgw_view_bytes(eng._h))), dtype=torch.uint8, device="cuda")
          def both():
            step(); eng.agent_views(out=buf)
          r[case] = timed(both)
        else:
          r[case] = timed(step)
      except N.SgwError as ex:                              # (the parent commit's library refuses the windows in the launch)
        r[case] = {"refused": str(ex)[:120]}
      eng.close()
    res[label] = r
  print("RESULT " + json.dumps(res))


ALL_CASES = "round,round_with_views,round_then_sgw_agent_views"


def run_child(n, launches, chunk, library, cases=ALL_CASES):
  env = dict(os.environ)
  env.pop("SGW_VIEWS_CHUNK", None); env.pop("SGW_LIBRARY", None)
  if chunk:
    env["SGW_VIEWS_CHUNK"] = str(chunk)
  if library:
    env["SGW_LIBRARY"] = library
  out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--launches", str(launches), "--cases", cases],
                       env=env, capture_output=True, text=True, timeout=240)
  if out.returncode != 0:
    raise RuntimeError("probe child failed (exit %d): %s" % (out.returncode, out.stderr[-2000:]))
  return json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def kernel_registers():
  """Register counts of the one-step kernels from the installed build's assembly (libsgw.s), where it is there."""
  from ai_safety_gridworlds_amd import build as B, isa_lint
  if not os.path.exists(B.ASM):
    return None
  keys = ("vgpr_count", "agpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count")
  return {k: {x: d.get(x) for x in keys} for k, d in isa_lint.metadata_stats(open(B.ASM).read()).items()
          if "k_engine" in k and "Li0E" in k and any(f in k for f in ("Savanna", "IslandMa"))}


KERNELS = {"aintelope_savanna": ("7SavannaE", "15SavannaBigViewsE", 1), "island_navigation_ex_ma": ("9IslandMaTILi4EEE", "16IslandMaBigViewsE", 2)}


def add_residency(res, regs):
  """resident workgroups per CU = min(LDS: 160 KiB / bytes, registers: 4 SIMDs x floor(512 / (VGPR + AGPR)) waves / waves per
  workgroup) for every case that recorded its LDS bytes."""
  if not regs:
    return
  for cfg, r in res.items():
    plain, big, waves = KERNELS[cfg.split("/")[0]]
    for case in ("round", "round_with_views"):
      if case + "_lds_bytes" not in r or r[case + "_lds_bytes"] <= 0:
        continue
      tag = big if case == "round_with_views" else plain
      k = [d for n, d in regs.items() if "INS_" + tag + "Li0E" in n]
      if len(k) != 1:
        continue
      per_simd = 512 // max(1, k[0]["vgpr_count"] + k[0]["agpr_count"])
      r[case + "_resident_workgroups_per_cu"] = min(160 * 1024 // r[case + "_lds_bytes"], 4 * per_simd // waves)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_views_inlaunch.json"))
  ap.add_argument("--n", type=int, default=65536)
  ap.add_argument("--launches", type=int, default=200)
  ap.add_argument("--chunks", default="8,16,32,64")
  ap.add_argument("--runs", type=int, default=3)
  ap.add_argument("--baseline-library", default=None)
  ap.add_argument("--sweep-library", default=None)
  ap.add_argument("--child", action="store_true")
  ap.add_argument("--cases", default=ALL_CASES)
  args = ap.parse_args()
  if args.child:
    return child(args.n, args.launches, args.cases.split(","))
  regs = kernel_registers()
  res = {"n_envs": args.n, "outputs": list(ROUND), "installed": run_child(args.n, args.launches, None, None), "by_chunk": {}, "round_ab": []}
  add_residency(res["installed"], regs)
  print("installed library done", flush=True)
  for g in [int(x) for x in args.chunks.split(",") if x and args.sweep_library]:
    res["by_chunk"][str(g)] = run_child(args.n, args.launches, g, args.sweep_library)
    add_residency(res["by_chunk"][str(g)], regs)
    print("G = %d done" % g, flush=True)
  if args.baseline_library:                                  # A/B of the round without windows: alternating processes
    for i in range(args.runs):
      for tag, lib in (("this", None), ("baseline", args.baseline_library)):
        r = run_child(args.n, args.launches, None, lib, "round")
        res["round_ab"].append({"library": tag, "run": i, **{c: {k: v for k, v in r[c].items() if k.startswith("round")} for c in r}})
        print("A/B run %d %s done" % (i, tag), flush=True)
  res["kernel_registers"] = regs
  text = json.dumps(res, indent=1)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      f.write(text + "\n")
  print(text)


if __name__ == "__main__":
  main()
