"""The launch-path case table (tests/launch_paths.py) is complete: a row for every base env name, and each row's group tag
is exactly what the SGW_GROUP_FAMILIES X-macro of csrc/sgw_group.hpp lists -- so a new family or group member cannot ship
without a row that tests/test_launch_paths_gpu.py runs on every launch path."""
import os
import re

from ai_safety_gridworlds_amd import specs
from ai_safety_gridworlds_amd.specs import make_spec
from tests import launch_paths as LP

GROUP_HPP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ai_safety_gridworlds_amd", "csrc",
                         "sgw_group.hpp")


def group_tags():
  """The member tags of the SGW_GROUP_FAMILIES X-macro, in order."""
  src = open(GROUP_HPP).read()
  m = re.search(r"#define\s+SGW_GROUP_FAMILIES\(X\)((?:[^\n]*\\\n)*[^\n]*)", src)
  assert m, "SGW_GROUP_FAMILIES not found in sgw_group.hpp"
  tags = re.findall(r"X\(\s*(TAG_\w+)\s*,\s*\w+\s*\)", m.group(1))
  assert tags, "SGW_GROUP_FAMILIES lists no member"
  return tags


def test_every_base_env_name_has_a_row():
  names = set(specs.ENV_FAMILIES) | {"aintelope_savanna"}
  rows = {r["name"] for r in LP.ROWS}
  assert names - rows == set(), "base env names without a launch-path row: %s" % sorted(names - rows)
  assert rows <= names, "rows for unknown env names: %s" % sorted(rows - names)
  assert len(LP.BY_ID) == len(LP.ROWS), "row ids must be unique"


def test_group_tags_match_the_x_macro():
  tags = group_tags()
  assert len(set(tags)) == len(tags)
  declared = {r["tag"] for r in LP.ROWS if r["tag"]}
  assert declared == set(tags), "X-macro members without a row: %s; row tags the X-macro does not list: %s" % (
      sorted(set(tags) - declared), sorted(declared - set(tags)))
  # the round-kernel families are no members: their rows must say so
  for r in LP.ROWS:
    if r["name"] in ("firemaker_ex_ma", "island_navigation_ex_ma", "aintelope_savanna"):
      assert r["tag"] is None, r["id"]


def test_every_group_tag_is_in_a_group_of_rows():
  in_groups = [m for _, ms in LP.GROUPS for m in ms]
  assert len(in_groups) == len(set(in_groups)) and set(in_groups) <= set(LP.BY_ID)
  assert {LP.BY_ID[m]["tag"] for m in in_groups} == set(group_tags())
  assert all(LP.BY_ID[m]["tag"] for m in in_groups), "a non-member row is listed in a group"
  assert all(2 <= len(ms) <= 4 for _, ms in LP.GROUPS) and any(len(ms) == 4 for _, ms in LP.GROUPS)
  sizes = [LP.BY_ID[m]["n"] for m in in_groups]
  assert all(n % 64 for n in sizes) and min(sizes) < 64


def test_rows_build_and_the_island_rows_pick_their_state_variant():
  for r in LP.ROWS:
    sp = make_spec(r["name"], **r["kw"])
    assert r["n"] % 64, r["id"]
    if r["name"] == "island_navigation_ex":     # F_GENERAL (16): per-event vectors; integral flags: the packed state
      general = bool(sp.native.flags & 16)
      assert (r["tag"] is None) == general, r["id"]
      assert (r["state_words"] is not None) == (not general), r["id"]
