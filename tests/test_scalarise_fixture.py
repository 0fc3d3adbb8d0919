"""CPU tier of scalarise=True: the committed fixtures (tests/golden/make_fixtures_scalarise.py: the reference run twice over one
action tape, scalarise=False and scalarise=True) say what the feature has to compute -- the scalar columns are the explicit
left-to-right loop over the vector columns of the same file, bit for bit, and the average is the sum of the quotients."""
import numpy as np
import pytest

from tests import scalarise_ref as R


@pytest.fixture(scope="module", params=R.CONFIGS)
def fx(request):
  return request.param, R.load(request.param)


def test_fixture_shapes_and_tape(fx):
  name, z = fx
  T = z["actions"].shape[0]
  S = T + 2                                                  # the first reset, every step, the explicit reset
  K = len(str(z["meta_dim_names"]).split("|"))
  assert K == {"island_L9": 10, "boat_ex_L3": 6}[name]
  for k in ("reward", "cumulative_reward", "average_reward", "last_performance", "overall_performance"):
    assert z[k].shape == (S, K) and z[k].dtype == np.float64, k
  for k in ("scalar_reward", "scalar_cumulative_reward", "scalar_average_reward", "scalar_last_performance", "scalar_overall_performance"):
    assert z[k].shape == (S,) and z[k].dtype == np.float64, k
  assert z["frame"].shape == (S,) and z["step_type"].shape == (S,)
  assert T >= 60 and 0 < int(z["reset_at"]) < T
  assert (z["step_type"] == 2).sum() >= 1, "an episode ends on the tape"
  assert (z["step_type"] == 0).sum() >= 3, "the first reset, the explicit reset and an auto-reset"
  assert (z["reward"][z["reward_none"]] == 0).all() and (z["scalar_reward"][z["reward_none"]] == 0).all()


def test_scalar_columns_are_the_left_to_right_loop(fx):
  _, z = fx
  assert R.same_bits(z["scalar_reward"], R.loop_sums(z["reward"]))
  assert R.same_bits(z["scalar_cumulative_reward"], R.loop_sums(z["cumulative_reward"]))
  assert R.same_bits(z["scalar_average_reward"], R.loop_averages(z["cumulative_reward"], z["frame"]))
  # the vector run's own average_reward is cumulative / (frame + 1) per dimension: the quotients the scalar run sums
  assert R.same_bits(z["average_reward"], z["cumulative_reward"] / (z["frame"][:, None] + 1.0))
  assert R.same_bits(z["scalar_average_reward"], R.loop_sums(z["average_reward"]))


def test_average_is_not_the_quotient_of_the_sum():
  z = R.load("island_L9")
  naive = R.loop_sums(z["cumulative_reward"]) / (z["frame"] + 1.0)
  differs = naive != z["scalar_average_reward"]
  assert differs.sum() >= 1, "the fixture must hold a row that tells sum(x / n) from sum(x) / n"
  assert np.abs(naive - z["scalar_average_reward"])[differs].max() < 1e-12, "and only the last bits differ"


def test_performance_getters(fx):
  _, z = fx
  for vec, sca in (("last_performance", "scalar_last_performance"), ("overall_performance", "scalar_overall_performance")):
    none = np.isnan(z[sca])
    assert (np.isnan(z[vec]).all(axis=1) == none).all(), "None (NaN) until the first episode ends, in both runs"
    assert (~none).sum() >= 1
    assert R.same_bits(z[sca][~none], R.loop_sums(z[vec][~none])), sca
  # the last performance is the episode return of the row that was LAST
  last_rows = np.nonzero(z["step_type"] == 2)[0]
  for i in last_rows:
    assert R.same_bits(z["last_performance"][i], z["cumulative_reward"][i])



@pytest.mark.parametrize("name", R.MA_CONFIGS)
def test_two_agent_fixtures(name):
  """Per agent, over that agent's own k dimensions (firemaker's worker has 2, its supervisor 3; the absent column none)."""
  z = R.load(name)
  ks, slots = z["k_agent"].tolist(), z["meta_slots"].tolist()
  S, A, K = z["reward"].shape
  assert S == z["actions"].shape[0] + 2 and A == len(ks) and K == max(ks)
  assert ks == {"firemaker_a2": [2, 0, 3], "savanna_a2": [11, 11]}[name]
  assert z["rng_state"].shape == (4,) and z["rng_state"].dtype == np.uint64
  assert (z["step_type"][:, slots] == 2).all(axis=1).sum() >= 1, "an episode ends on the tape"
  nonzero = 0
  for a in range(A):
    k = ks[a]
    assert not z["reward"][:, a, k:].any() and not z["cumulative_reward"][:, a, k:].any()
    assert R.same_bits(z["scalar_reward"][:, a], R.loop_sums(z["reward"][:, a], k))
    assert R.same_bits(z["scalar_cumulative_reward"][:, a], R.loop_sums(z["cumulative_reward"][:, a], k))
    assert R.same_bits(z["scalar_average_reward"][:, a], R.loop_averages(z["cumulative_reward"][:, a], z["frame"], k))
    none = np.isnan(z["scalar_overall_performance"][:, a])
    if a in slots:
      assert (~none).sum() >= 1 and (np.isnan(z["overall_performance"][:, a, :k]).all(axis=1) == none).all()
      assert R.same_bits(z["scalar_overall_performance"][~none, a], R.loop_sums(z["overall_performance"][~none, a], k))
    nonzero += int((z["scalar_reward"][:, a] != 0).sum())
  assert nonzero >= 20
