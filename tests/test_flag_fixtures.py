"""The flag fixtures of tests/flag_fixtures.py pin what they claim to pin: per family the rows name every numeric and reward flag,
every moved flag changes the oracle's outcome on the fixture's own tape, the dead flags change nothing, the lopsided windows have
the shape their radii say, and the files stay small.  (That the oracle reproduces each file bit for bit is the business of the
families' test_oracle_*_golden.py, which pick the files up by their prefixes.)"""
import os

import numpy as np
import pytest

from ai_safety_gridworlds_amd.specs import make_spec
from tests import flag_fixtures as FF
from tests import golden_util as G

NAMES = sorted(FF.ROWS)
MOVED = [(n, f) for n in NAMES for f in FF.ROWS[n][1]]


def _default(family, flag):
  return FF.FAMILIES[family][1][flag]


def _moved(family, flag, value):
  """Whether `value` differs from the flag's default (a reward flag: as the {dimension: value} dict over the default's keys)."""
  d = _default(family, flag)
  if isinstance(d, dict):
    return {k: float(value.get(k, 0)) for k in d} != {k: float(v) for k, v in d.items()} or bool(set(value) - set(d))
  return float(value) != float(d)


def test_every_row_has_its_file_and_every_file_its_row():
  on_disk = {n for n in G.fixture_names() if "_num_" in n or "_asym" in n or n == "sav_radius_none"}
  assert on_disk == set(NAMES)
  for n in NAMES:
    family = FF.ROWS[n][0]
    _, meta = G.load(n)
    assert meta["family_name"] == FF.FAMILIES[family][0], n


@pytest.mark.parametrize("family", sorted(FF.FAMILIES))
def test_rows_name_every_numeric_and_reward_flag(family):
  named = {f for n in NAMES if FF.ROWS[n][0] == family for f in FF.ROWS[n][1]}
  want = set(FF.moved_flags(family))
  assert set(FF.DEAD[family]) <= want, "a dead flag that is no flag of the family"
  missing = want - named - set(FF.DEAD[family])
  assert not missing, "%s: no flag fixture moves %s" % (family, sorted(missing))
  assert named <= want, "%s: rows name %s, which are no numeric or reward flags of the family" % (family, sorted(named - want))


@pytest.mark.parametrize("name", NAMES)
def test_row_lists_exactly_what_the_fixture_moves(name):
  family, flags = FF.ROWS[name]
  _, kwargs = FF.load(name)
  upper = {k.upper(): v for k, v in kwargs.items()}
  for f in flags:
    assert f in upper and _moved(family, f, upper[f]), "%s: %s is listed but sits at its default" % (name, f)
  unlisted = [f for f in FF.moved_flags(family) if f in upper and _moved(family, f, upper[f]) and f not in flags]
  assert not unlisted, "%s moves %s without listing them" % (name, unlisted)
  make_spec(FF.FAMILIES[family][0], **kwargs)                 # inside what the engine accepts (_check_regrowth_exponent among it)
  for f in ("DRINK_GROWTH_LIMIT", "FOOD_GROWTH_LIMIT"):
    assert float(upper.get(f, 20.0)) <= 60.0


_CACHE = {}


def _fixture(name):
  if name not in _CACHE:
    fx, kwargs = FF.load(name)
    family = FF.ROWS[name][0]
    _CACHE[name] = (fx, kwargs, FF.fixture_fields(family, fx))
  return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_fixture_as_recorded(name):
  """The base of the observability check below: with every flag as recorded nothing differs."""
  fx, kwargs, want = _fixture(name)
  assert FF.differing(FF.oracle_fields(FF.ROWS[name][0], fx, kwargs), want) == []


@pytest.mark.parametrize("name,flag", MOVED)
def test_moved_flag_is_observable(name, flag):
  """The oracle with this one flag back at its default: a live flag changes at least one compared field, a dead one none."""
  family = FF.ROWS[name][0]
  fx, kwargs, want = _fixture(name)
  back = {k: v for k, v in kwargs.items() if k.upper() != flag}
  assert len(back) == len(kwargs) - 1
  bad = FF.differing(FF.oracle_fields(family, fx, back), want)
  if flag in FF.DEAD[family]:
    assert bad == [], "%s: %s is listed as dead (%s) but changes %s" % (name, flag, FF.DEAD[family][flag], bad)
  else:
    assert bad, "%s: putting %s back to its default changes nothing on this tape" % (name, flag)


@pytest.mark.parametrize("name", sorted(FF.WINDOWS))
def test_lopsided_windows_have_the_shape_of_their_radii(name):
  fx, kwargs = FF.load(name)
  spec = make_spec(FF.FAMILIES[FF.ROWS[name][0]][0], **kwargs)
  for field, shape in FF.WINDOWS[name].items():
    assert fx[field].shape[-2:] == shape, (name, field, fx[field].shape)
  shapes = {tuple(s) for s in spec.view_shapes if tuple(s) != (0, 0)}
  assert shapes == set(FF.WINDOWS[name].values())
  if "_asym" in name:      # no side equals its opposite: swapping left / right or up / down moves the agent inside the window
    radii = [v for k, v in kwargs.items() if k.endswith("observation_radius")]
    assert radii and all(r[0] != r[1] and r[2] != r[3] and len(set(r)) >= 3 for r in radii)
  # the windows are not blank: they show board cells and, near the border, the character outside the board
  for field in FF.WINDOWS[name]:
    assert len(np.unique(fx[field][:, 1:])) >= 3


def test_size_caps():
  sizes = {n: os.path.getsize(os.path.join(G.GOLDEN, n + ".npz")) for n in NAMES}
  for n, s in sizes.items():
    assert s <= FF.MAX_FILE_BYTES, "%s: %d bytes" % (n, s)
    fx = np.load(os.path.join(G.GOLDEN, n + ".npz"))
    assert int(fx["meta_E"]) <= 24 and int(fx["meta_T"]) <= 160, n
  assert sum(sizes.values()) <= FF.MAX_TOTAL_BYTES, sum(sizes.values())
