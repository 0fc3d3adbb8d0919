"""The four kernels that can step island_navigation_ex level 9 with default parameters (the headline), as sgw_create picks them
(csrc/sgw_api.hip: SGW_GENERIC_STEP, SGW_GENERIC_RULES, SGW_NO_FORK, engine_step_fork), once, for every test that runs a
feature on each of them (tests/test_headline_kernels_gpu.py; the conditions of its tapes: tests/test_headline_kernels.py).

KERNELS: id, the environment variable read at sgw_create (None: the default selection) and the triple
(sgw_step_rules, sgw_step_shape, sgw_step_fork) the engine must report:
  fork        k_step_fork<IslandL9Default, Shape>: the default while n_pad / 64 <= 4 x CUs
  one_wave    k_engine<IslandL9Default, K_STEP, Shape>: the default above that size, SGW_NO_FORK below it
  shape_only  k_engine<IslandPacked, K_STEP, Shape>: SGW_GENERIC_RULES, or a shaped spec the compiled rule set refuses
  generic     k_engine<IslandPacked, K_STEP>: SGW_GENERIC_STEP
(The shaped entry is the packed state's: a level 9 spec that does not pack steps with the plain state's generic kernel.)

select() chooses one for a whole test: eng.fork(), lookahead(), the twins of the closed-loop tests and the facades create their
engines later, and sgw_create reads the environment every time.  It also watches BatchedEngine.__init__, so every engine the
test creates -- wherever -- has its triple asserted when it is made.

quit_case(): the `_quitlate` tape of tests/action_domain.py on the default spec, with the C oracle's arrays (no GPU)."""
import numpy as np

from ai_safety_gridworlds_amd import philox

ENV_VARS = ("SGW_NO_FORK", "SGW_GENERIC_RULES", "SGW_GENERIC_STEP")
KERNELS = (
    dict(id="fork", env=None, triple=(1, 1, 1)),
    dict(id="one_wave", env="SGW_NO_FORK", triple=(1, 1, 0)),
    dict(id="shape_only", env="SGW_GENERIC_RULES", triple=(0, 1, 0)),
    dict(id="generic", env="SGW_GENERIC_STEP", triple=(0, 0, 0)),
)
BY_ID = {k["id"]: k for k in KERNELS}
IDS = [k["id"] for k in KERNELS]
NAME = "island_navigation_ex"


def triple_of(eng):
  """(sgw_step_rules, sgw_step_shape, sgw_step_fork) of a BatchedEngine."""
  from ai_safety_gridworlds_amd import _native as N
  L = N.lib()
  return (int(L.sgw_step_rules(eng._h)), int(L.sgw_step_shape(eng._h)), int(L.sgw_step_fork(eng._h)))


def assert_selected(eng, kernel):
  kernel = BY_ID[kernel] if isinstance(kernel, str) else kernel
  assert triple_of(eng) == kernel["triple"], "an engine of %d envs runs (rules, shape, fork) = %s, not the %s kernel's %s" % (
      eng.n_envs, triple_of(eng), kernel["id"], kernel["triple"])


def select(kernel, monkeypatch, watch=True):
  """The kernel's variable set and the other two cleared until the test ends.  watch: every BatchedEngine made from here on is
  checked with assert_selected as soon as it exists; returns the list those engines are appended to."""
  kernel = BY_ID[kernel] if isinstance(kernel, str) else kernel
  for v in ENV_VARS:
    if v == kernel["env"]:
      monkeypatch.setenv(v, "1")
    else:
      monkeypatch.delenv(v, raising=False)
  made = []
  if watch:
    from ai_safety_gridworlds_amd.engine import BatchedEngine
    init = BatchedEngine.__init__

    def watched(self, *args, **kw):
      init(self, *args, **kw)
      assert_selected(self, kernel)
      made.append(self)

    monkeypatch.setattr(BatchedEngine, "__init__", watched)
  return made


# ---- QUIT and out-of-range actions on the default spec ------------------------------------------------------------------------------
QUIT_NS = (1, 65, 257)                  # on the GPU; the CPU tier also checks 63 and 193
QUIT_T, QUIT_CALLS = 16, 3              # three sgw_step_n calls over one buffer: direct, capture, replay
QUIT_STEPS = QUIT_T * QUIT_CALLS
# episodes that end with QUIT inside the 48 steps, and turn values 5..8 in the tape, from the C oracle on the host
QUIT_ENDS = {1: 2, 63: 102, 65: 105, 193: 322, 257: 424}
QUIT_TURNS = {1: 0, 257: 383}

_QUIT = {}


def quit_tape(n):
  """int8 [QUIT_STEPS, n]: the spec's own Philox stream under the `_quitlate` overlay of tests/action_domain.py."""
  from ai_safety_gridworlds_amd.specs import make_spec
  from tests import action_domain as AD
  spec = make_spec(NAME)
  ids = np.arange(n)
  return AD.overlay(philox.actions(AD.SEED, ids, np.arange(QUIT_STEPS), spec.action_lo, spec.n_actions), ids)


def quit_case(n):
  """(tape int8 [QUIT_STEPS, n], the oracle's arrays [n, QUIT_STEPS + 1, ...] of FIELDS), cached per n and left unchanged."""
  if n not in _QUIT:
    from oracle import oracle as O
    from tests.test_headline_prologue_gpu import FIELDS
    tape = quit_tape(n)
    _QUIT[n] = (tape, O.run_streams(O.make_config(NAME), tape.T.copy(), fields=list(FIELDS), nthreads=8))
  return _QUIT[n]
