"""What GridworldGymEnv returns for firemaker_ex_ma with a controlled agent, flattened to named arrays: recorded once by
tests/golden/make_fixtures_gym_infos.py (this project's own GPU output, from in front of the facades' shared info helpers)
and compared key by key in tests/test_firemaker_gpu.py."""
import json

import numpy as np

from ai_safety_gridworlds_amd import philox

KW = dict(amount_agents=3, max_iterations=50, FIRE_SPREAD_PROBABILITY_AT_DISTANCE_ONE=0.05)
STEPS, SEED = 12, 31
AGENTS = {"1": 0, "S": 2}                  # controlled agent character -> its column


def _plain(v):
  if isinstance(v, np.ndarray):
    return v.tolist()
  if isinstance(v, np.generic):
    return v.item()
  if isinstance(v, (list, tuple)):
    return [_plain(x) for x in v]
  if isinstance(v, dict):
    return {str(k): _plain(x) for k, x in v.items()}
  if isinstance(v, (bool, int, float, str)) or v is None:
    return v
  return repr(v)                           # enums (TerminationReason)


def flatten(prefix, info, out):
  for k, v in info.items():
    if isinstance(v, np.ndarray) and v.dtype != object:
      out["%s/%s" % (prefix, k)] = v
    elif isinstance(v, dict) and v and all(isinstance(x, np.ndarray) for x in v.values()):
      for c, x in v.items():
        out["%s/%s/%s" % (prefix, k, c)] = x
    else:
      out["%s/%s" % (prefix, k)] = np.array(json.dumps(_plain(v), sort_keys=True))
  return out


def record(agent):
  """{name: array} of reset() and STEPS steps of the controlled `agent`: state, reward, terminated and every info key."""
  from ai_safety_gridworlds_amd.helpers.gridworld_gym_env import GridworldGymEnv
  own = philox.actions(SEED, np.arange(1), np.arange(STEPS), 0, 5, agent=AGENTS[agent])[:, 0]
  env = GridworldGymEnv("firemaker_ex_ma", agent_character=agent, seed=SEED, **KW)
  out = {}
  state, info = env.reset()
  out["%s/0/state" % agent] = state
  flatten("%s/0" % agent, info, out)
  for t in range(STEPS):
    state, reward, terminated, truncated, info = env.step(int(own[t]))
    p = "%s/%d" % (agent, t + 1)
    out[p + "/state"], out[p + "/reward"], out[p + "/terminated"] = state, np.asarray(reward), np.asarray(terminated)
    flatten(p, info, out)
  env.close()
  return out
