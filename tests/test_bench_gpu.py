"""bench.py as the driver runs it, on one GPU: a plain run times exactly --steps steps, prints the contract fields and nothing that
takes a leg of its own, and --dump-outputs writes the same arrays from run to run -- the outputs of the last timed step, checked here
against the C oracle on the same Philox action stream; --full adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_LEGS = ("fused_rollout", "full_observation", "cpu_baseline")


def _bench(*args):
  p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + list(args), cwd=REPO,
                     capture_output=True, text=True, timeout=600)
  assert p.returncode == 0, p.stderr[-3000:]
  lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
  assert len(lines) == 1, p.stdout[-2000:]
  return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_asked_steps_and_dumps_the_last_step(tmp_path):
  import bench as B
  from ai_safety_gridworlds_amd import philox
  from oracle import oracle as O
  K, W = 50, 10
  lines = [_bench("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / str(i))) for i in range(2)]
  for d in lines:
    assert d["timed_steps"] == K and d["repeats"] == 1 and d["steps"] == K and d["warmup"] == W
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 65536 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert not any(k in d for k in FULL_LEGS)
  names = sorted(os.listdir(str(tmp_path / "0")))
  assert names == sorted(os.listdir(str(tmp_path / "1")))
  assert sum(os.path.getsize(str(tmp_path / "0" / f)) for f in names) <= 64 * 10 ** 6
  got = {}
  for f in names:
    a0, a1 = np.load(str(tmp_path / "0" / f)), np.load(str(tmp_path / "1" / f))
    assert a0.dtype in (np.float32, np.float64) and np.array_equal(a0, a1), f
    got[f[:-4]] = a0
  assert set(got) == set(B.WORKLOADS["island_navigation_ex"]["outputs"]) | {"returns"}
  # the steps behind the timed region: W warmup steps (Philox steps 0..W-1), then the K-step batch of steps W..W+K-1 twice
  # untimed (graph capture) and once timed; the envs are independent, so 4096 of them stand for the 65 536
  E = 4096
  steps = np.concatenate([np.arange(W)] + [W + np.arange(K)] * 3)
  acts = philox.actions(B.SEED, np.arange(E), steps, 0, 5).T.copy()
  want = O.run_streams(O.make_config("island_navigation_ex", level=9), acts,
                       fields=["board", "reward", "step_type", "term_reason", "safety", "frame"])
  for k in ("board", "reward", "step_type", "safety", "frame"):
    assert np.array_equal(got[k][:E].reshape(want[k][:, -1].shape), want[k][:, -1]), k      # step_type: [N, 1] per agent
  term = got["term_reason"][:E].astype(np.int16)
  term[term == 255] = -1
  assert np.array_equal(term, want["term_reason"][:, -1])


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
  d = _bench("--steps", "20", "--warmup", "5", "--full", "--min-seconds", "0.2", "--cpu-seconds", "1")
  assert d["timed_steps"] == 20 * d["repeats"] and d["repeats"] >= 1
  for k in FULL_LEGS:
    assert d[k]["value"] > 0, k
