"""CPU tier: the forked headline step kernel (k_step_fork, csrc/sgw_kernels.hpp) in the gfx950 assembly of the installed build
(libsgw.s, read the way tests/test_prologue_order.py reads it).

* the kernel is in the build exactly once, uses no scratch and spills no SGPR;
* its prologue is k_engine's: every vector load stands ahead of the first wait, nothing is a flat access, the kernarg touch's
  loads and its wait name one SGPR that nothing in between writes;
* THE ordering the fork rests on -- every wave's loads of the old state have returned before any state wave stores the new
  one -- is in the code: a wait for vmcnt(0) stands between the last load of the prologue and the first s_barrier, and no global
  store or atomic stands ahead of that barrier;
* the island k_engine census of tests/test_prologue_order.py still holds (the fork is a kernel of its own name: eleven island
  k_engine kernels, one of them the headline's)."""
import re

import pytest

from tests.test_prologue_order import LOAD, SETTLE, _all, _kernels, _prologue, _written_sgprs, asm  # noqa: F401  (asm: the fixture)

FORK = re.compile(r"^(_ZN3sgw11k_step_forkI\w+):", re.M)
HEADLINE = "15IslandL9Default"


@pytest.fixture(scope="module")
def fork(asm):  # noqa: F811
  names = FORK.findall(asm)
  assert len(names) == 1 and HEADLINE in names[0], names
  body = asm[asm.index(names[0] + ":") + len(names[0]) + 1:]
  return names[0], body[:body.index(".Lfunc_end")]


def test_the_fork_kernel_is_there_once_and_in_registers(asm, fork):  # noqa: F811
  k, body = fork
  assert re.search(r"\.set %s\.private_seg_size, 0$" % re.escape(k), asm, re.M), "the fork kernel uses scratch memory"
  assert not re.search(r"^\s+v_(writelane|readlane)_b32", body, re.M), "the fork kernel spills SGPRs"


def test_the_island_k_engine_census_still_holds(asm):  # noqa: F811
  ks = _kernels(asm)
  assert sum(1 for k in ks if HEADLINE in k) == 1, sorted(ks)
  assert len(ks) == 3 * 3 + 2, sorted(ks)


def test_every_prologue_load_is_issued_before_the_first_wait(fork):
  k, body = fork
  pro = _prologue(body)
  loads = [i for i, (op, _, _) in enumerate(pro) if LOAD.match(op)]
  waits = [i for i, (op, _, _) in enumerate(pro) if op == "s_waitcnt"]
  # level tables, the packed state's five pairs, the action, the pow piece(s)
  assert len(loads) >= 8 and waits, (len(loads), waits)
  assert waits[0] > loads[-1], "`%s %s` stands ahead of the load `%s %s`" % (pro[waits[0]][:2] + pro[loads[-1]][:2])
  assert not any(op.startswith("flat_") for op, _, _ in pro), "a flat instruction in the prologue"


def test_old_state_loads_return_before_the_barrier_and_nothing_is_stored_ahead_of_it(fork):
  k, body = fork
  pro = _prologue(body)
  assert pro[-1][0] == "s_barrier"
  last_load = max(i for i, (op, _, _) in enumerate(pro) if LOAD.match(op))
  drained = [i for i, (op, rest, _) in enumerate(pro) if op == "s_waitcnt" and re.search(r"vmcnt\(0\)", rest) and i > last_load]
  assert drained, "no s_waitcnt vmcnt(0) between the last prologue load and the barrier: %s" % (pro[last_load:],)
  # the whole kernel up to that barrier, not only from the first load on
  ins = _all(body)
  bar = next(i for i, x in enumerate(ins) if x[0] == "s_barrier")
  early = [(op, rest) for op, rest, _, _ in ins[:bar] if re.match(r"(global|buffer|flat|scratch)_(store|atomic)", op)]
  assert not early, early
  # one barrier in the kernel: the two roles never meet again
  assert sum(1 for x in ins if x[0] == "s_barrier") == 1


def test_the_kernarg_touch_is_split_soundly(fork):
  k, body = fork
  ins = _all(body)
  settle = [i for i, x in enumerate(ins) if x[3]]
  assert len(settle) == 1 and ins[settle[0]][0] == "s_waitcnt" and ins[settle[0]][1].startswith("lgkmcnt(0)"), settle
  touch = [i for i, (op, _, inside, _) in enumerate(ins[:settle[0]]) if inside and op == "s_load_dword"]
  assert len(touch) >= 2
  dst = {ins[i][1].split(",")[0].strip() for i in touch}
  assert len(dst) == 1 and re.fullmatch(r"s\d+", next(iter(dst))), dst
  reg = next(iter(dst))
  assert ("%s free" % reg) in body, "the settle statement holds another register than the touch's %s" % reg
  for op, rest, inside, _ in ins[touch[-1] + 1:settle[0]]:
    assert not inside, (op, rest)
    assert int(reg[1:]) not in _written_sgprs(op, rest), "`%s %s` writes the touch's SGPR before its loads have returned" % (op, rest)
    assert not op.startswith(("ds_read", "ds_load")), (op, rest)
    c = re.search(r"lgkmcnt\((\d+)\)", rest) if op == "s_waitcnt" else None
    assert not c or c.group(1) == "0", (op, rest)
    assert op not in ("s_barrier", "s_endpgm"), op
  after = ins[settle[0] + 1:]
  bar = next(i for i, x in enumerate(after) if x[0] == "s_barrier")
  assert not any(LOAD.match(op) or op.startswith("ds_") for op, _, _, _ in after[:bar]), after[:bar]
