"""engine.fused_views: which specs the wrappers take their agent windows from the round's own launch for (sgw_out.views /
obs_views).  The one-wavefront families' launch can also write windows larger than the board (tests/test_views_inlaunch_gpu.py),
but it was measured slower than the round followed by sgw_agent_views for both of them (profiles/r06_views_inlaunch.json), so
those specs stay on two launches: the assertion that they fuse is not made."""
import pytest

from ai_safety_gridworlds_amd.engine import fused_views
from ai_safety_gridworlds_amd.specs import make_spec


@pytest.mark.parametrize("name,kw", [
    ("aintelope_savanna", dict()),                                                       # 21 x 21 on 13 x 13
    ("aintelope_savanna", dict(amount_agents=2)),
    ("aintelope_savanna", dict(level=3, amount_food_patches=1, observation_radius=[2, 2, 2, 2])),      # 5 x 5 on 3 x 4
    ("island_navigation_ex_ma", dict(observation_radius=[3, 3, 3, 3])),                  # 7 x 7 = 49 cells on 6 x 8 = 48
])
def test_fused_views_stays_false_where_the_launch_was_measured_slower(name, kw):
  spec = make_spec(name, **kw)
  assert any(h * w > spec.H * spec.W for (h, w) in spec.view_shapes), "the case is about a window with more cells than the board"
  assert not fused_views(spec)


@pytest.mark.parametrize("name,kw", [
    ("aintelope_savanna", dict(observation_radius=[2, 2, 2, 2])),                        # 5 x 5 on 13 x 13
    ("island_navigation_ex_ma", dict()),
    ("firemaker_ex_ma", dict(amount_agents=3)),
])
def test_fused_views_unchanged_for_small_windows(name, kw):
  assert fused_views(make_spec(name, **kw))


@pytest.mark.parametrize("name", ["island_navigation_ex", "boat_race_ex", "safe_interruptibility", "tomato_watering"])
def test_fused_views_false_for_single_agent_families(name):
  assert not fused_views(make_spec(name))
