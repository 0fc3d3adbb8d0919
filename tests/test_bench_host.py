"""Host logic of bench.py (no GPU): the timed region must issue EXACTLY count x K steps per engine, batch j from action batch
j modulo the number resident, whatever grouping run_batches uses to hand contiguous batches to sgw_step_n in one call; and the
mixed suite's parts must cover the global env-id ranges exactly once over the ranks."""
import contextlib
import os

import numpy as np
import pytest
import torch

import bench as B


class FakeActs(object):
  """Stands for the resident [steps, N] action tensor: slicing records (start, stop)."""
  def __init__(self, steps):
    self.shape = (steps, 8)
  def __getitem__(self, sl):
    return (sl.start, sl.stop)


class FakeEngine(object):
  def __init__(self):
    self.calls = []
  def step_n(self, span, accumulate=False):
    self.calls.append(span)


@pytest.mark.parametrize("K,nd,first,count", [(20, 204, 0, 3361), (2000, 2, 0, 41), (7, 5, 3, 23), (1, 1, 0, 10), (64, 64, 60, 200)])
def test_run_batches_issues_exactly_the_asked_steps(K, nd, first, count, monkeypatch):
  monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
  engines = [dict(eng=FakeEngine(), acts=FakeActs(K * nd), stream=None), dict(eng=FakeEngine(), acts=FakeActs(K * nd), stream=None)]
  B.run_batches(engines, K, first, count, True)
  for e in engines:
    steps, j = 0, first
    for (lo, hi) in e["eng"].calls:
      assert 0 <= lo < hi <= K * nd and lo % K == 0 and (hi - lo) % K == 0
      assert lo == (j % nd) * K                                  # batch j comes from action batch j modulo nd, in order
      g = (hi - lo) // K
      assert g * K <= max(K, 2000)                               # groups stay near 2 000 steps
      j += g; steps += hi - lo
    assert steps == count * K and j == first + count
  assert [c for c in engines[0]["eng"].calls] == [c for c in engines[1]["eng"].calls]      # batch-major: the same spans per family


@pytest.mark.parametrize("world", [1, 2, 8])
def test_mixed_parts_cover_the_global_ranges_once(world):
  per_gpu = 32768
  seen = {}
  for rank in range(world):
    for fam, cnt, base in B.mixed_parts(rank, world, per_gpu):
      assert cnt > 0
      seen.setdefault(fam, []).append((base, base + cnt))
  total = 0
  for fam, spans in seen.items():
    spans.sort()
    assert spans[0][0] >= 0
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
      assert a1 <= b0                                            # no env id belongs to two ranks
    total += sum(hi - lo for lo, hi in spans)
  assert total == world * per_gpu and set(seen) == set(B.MIXED)


@pytest.mark.parametrize("n_steps,batch,nd", [(20, 20, 1), (4567, 2000, 2), (2000, 2000, 1), (1, 1, 1), (6001, 2000, 2)])
def test_run_steps_times_exactly_the_asked_steps(n_steps, batch, nd, monkeypatch):
  """bench.py --steps N: the timed region is N launches per engine whatever N is -- batches of B <= MAX_CALL_STEPS steps and a
  remainder from the head of action batch 0 -- and every call's outputs are kept as the engine's "out"."""
  monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())

  class Acts(FakeActs):
    def __getitem__(self, sl):
      return (sl.start or 0, sl.stop)

  class Eng(FakeEngine):
    def step_n(self, span, accumulate=False):
      self.calls.append(span)
      return {"last": span}
  engines = [dict(eng=Eng(), acts=Acts(batch * nd), stream=None) for _ in range(2)]
  B.run_steps(engines, n_steps, batch, True)
  for e in engines:
    assert sum(hi - lo for lo, hi in e["eng"].calls) == n_steps
    assert all(hi - lo <= B.MAX_CALL_STEPS for lo, hi in e["eng"].calls)
    assert e["out"] == {"last": e["eng"].calls[-1]}


def test_dump_outputs_float_files_within_budget(tmp_path):
  """--dump-outputs: float32 / float64 .npy files only, at most the budget in all (a seeded sample of env rows beyond it, with
  the rows' env ids), the same files from the same arrays."""
  n = 4096
  g = torch.Generator().manual_seed(3)
  out = {"board": torch.randint(0, 9, (n, 6, 8), generator=g, dtype=torch.uint8),
         "reward": torch.randn(n, 10, generator=g, dtype=torch.float64),
         "frame": torch.randint(0, 100, (n,), generator=g, dtype=torch.int32)}
  engines = [dict(fam="island_navigation_ex", n=n, out=out)]
  returns = {"island_navigation_ex": (None, np.arange(11, dtype=np.float64))}
  full = B.dump_outputs(str(tmp_path / "all"), engines, returns, budget=64 * 10 ** 6)
  assert full == ["board", "frame", "returns", "reward"]
  a = {k: np.load(str(tmp_path / "all" / (k + ".npy"))) for k in full}
  assert a["board"].dtype == np.float32 and a["reward"].dtype == np.float64 and a["frame"].dtype == np.float32
  assert np.array_equal(a["board"], out["board"].numpy()) and np.array_equal(a["reward"], out["reward"].numpy())
  budget = (1 << 20) + 100000                                  # room for ~1/4 of the 4096 rows
  names = B.dump_outputs(str(tmp_path / "s1"), engines, returns, budget=budget)
  B.dump_outputs(str(tmp_path / "s2"), engines, returns, budget=budget)
  assert "env_index" in names
  assert sum(os.path.getsize(str(tmp_path / "s1" / (k + ".npy"))) for k in names) <= budget
  idx = np.load(str(tmp_path / "s1" / "env_index.npy")).astype(np.int64)
  assert 0 < len(idx) < n and np.all(np.diff(idx) > 0)
  for k in names:
    s1, s2 = np.load(str(tmp_path / "s1" / (k + ".npy"))), np.load(str(tmp_path / "s2" / (k + ".npy")))
    assert s1.dtype in (np.float32, np.float64) and np.array_equal(s1, s2)
    if k in ("board", "reward", "frame"):
      assert np.array_equal(s1, a[k][idx])
