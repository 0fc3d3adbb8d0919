#!/usr/bin/env python3
"""Spec digests and refusal messages (tests/spec_cases.py), recorded from the package's own specs.py.

    python tests/golden/make_spec_digests.py   ->  tests/golden/spec_digests.json, tests/golden/spec_refusals.json

Both files are this project's own recorded results: {case key: SHA-256 prefix of the spec} and {refusal site: message}.
They were recorded in front of the GameSpec schema refactor and pin every value a spec carries; regenerate them only
for a change that is MEANT to alter a spec, never to make tests/test_spec_digests.py pass.
The one deliberate difference the digest hides is named in spec_cases.digest: `needs_rng` is digested as the effective
value `needs_rng or family == FIREMAKER_EX_MA`.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from ai_safety_gridworlds_amd.specs import make_spec      # noqa: E402
from tests import spec_cases                              # noqa: E402


def main():
  digests = {key: spec_cases.outcome(env, kw) for key, env, kw in spec_cases.cases()}
  refusals = {}
  for site, env, kw, exc, fragment in spec_cases.REFUSALS:
    try:
      make_spec(env, **kw)
    except Exception as e:      # recorded as raised; the test checks type and fragment against the hand-written row
      assert type(e) is exc and fragment in str(e), (site, type(e), str(e))
      refusals[site] = str(e)
    else:
      raise AssertionError("%s: no refusal" % site)
  for name, data in (("spec_digests.json", digests), ("spec_refusals.json", refusals)):
    with open(os.path.join(HERE, name), "w") as f:
      json.dump(data, f, indent=0, sort_keys=True)
      f.write("\n")
  print("%d digests, %d refusals" % (len(digests), len(refusals)))


if __name__ == "__main__":
  main()
