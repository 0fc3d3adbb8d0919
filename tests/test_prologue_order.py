"""CPU tier: the prologue of every kernel that stages the pow tables makes ONE memory round trip, read off the
gfx950 assembly of the installed build (libsgw.s, as tests/test_isa_lint.py reads it).

In the eleven island kernels (the ones that stage pow tables), between the first global load and the staging barrier
* every vector load (level tables, pow tables, state, first action) is issued before the first wait of any kind -- the compiler
  used to sink the pow-table loads, which it knows to be constant memory, below the kernarg touch and its wait;
  (the three IslandGeneral kernels: but for the one or two 8-byte loads of their per-event table, see the test);
* no load is a flat_load (a laundered table address that lost its address space would become one, and count in lgkmcnt).

In every k_engine kernel, whatever its family (all of them hold the split kernarg touch, and the split rests on the register
allocator leaving one SGPR alone, which only the assembly shows): the touch's scalar loads and its wait name the same SGPR,
nothing between them writes it, reads LDS or waits on a counted lgkmcnt, and no memory access stands between the wait and the
barrier.  Limit of that check: it scans the instructions in the order the assembly lists them from the last touch load to the
wait.  A block that executes between the two but is laid out elsewhere in the function (the pipelined rollout's
`drainer && a.actions == nullptr` branch may be) escapes it; what it does catch is the SGPR being reallocated, or spilled and
reloaded into another register, on the straight-line path.
"""
import os
import re

import pytest

ISLAND = re.compile(r"^(_ZN3sgw8k_engineINS_(?:7IslandTILb|15IslandL9Default)\w*):", re.M)
GENERAL = "7IslandTILb1E"                                   # IslandT<GENERAL = true, ...>
HEADLINE = "15IslandL9Default"
SETTLE = "kernarg touch settled"
LOAD = re.compile(r"^(global_load|buffer_load|scratch_load)_")


@pytest.fixture(scope="module")
def asm():
  if not os.path.exists("/opt/rocm/bin/hipcc"):
    pytest.skip("hipcc not present")
  from ai_safety_gridworlds_amd import build as B
  B.build()
  if not os.path.exists(B.ASM) or os.path.getmtime(B.ASM) < max(os.path.getmtime(d) for d in B._deps()):
    B.build(force=True)
  return open(B.ASM).read()


def _kernels(asm):
  out = {}
  for m in ISLAND.finditer(asm):
    body = asm[m.end():]
    out[m.group(1)] = body[:body.index(".Lfunc_end")]
  return out


def _prologue(body):
  """[(mnemonic, operands, in_asm_statement)] from the first vector load to the first s_barrier, the barrier included."""
  out, inside, started = [], False, False
  for line in body.splitlines():
    t = line.strip()
    if t.startswith(";;#ASMSTART"): inside = True; continue
    if t.startswith(";;#ASMEND"): inside = False; continue
    m = re.match(r"(s|v|ds|global|buffer|flat|scratch)_\w+", t)
    if not m or t.startswith(".") or t.endswith(":"):
      continue
    op, rest = m.group(0), t[m.end():].split(";")[0].strip()
    if not started and not (LOAD.match(op) or op.startswith("flat_load")):
      continue
    started = True
    out.append((op, rest, inside))
    if op == "s_barrier":
      return out
  raise AssertionError("no s_barrier after the first vector load")


def _written_sgprs(op, rest):
  """SGPR numbers an SALU / VALU instruction names as its destination (first operand); vcc / exec / m0 are not numbered SGPRs."""
  if op.startswith(("s_waitcnt", "s_barrier", "s_nop", "s_cbranch", "s_branch", "s_cmp", "s_bitcmp", "ds_", "global_", "buffer_", "scratch_")):
    return set()
  out = set()
  # (a VALU instruction with a carry-out -- v_mad_u64_u32, v_add_co_u32_e64, ... -- names that SGPR pair second: both count)
  for operand in rest.split(",")[:2 if op.startswith("v_") else 1]:
    m = re.fullmatch(r"s(\d+)", operand.strip())
    if m:
      out.add(int(m.group(1)))
    m = re.fullmatch(r"s\[(\d+):(\d+)\]", operand.strip())
    if m:
      out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
  return out


def test_the_island_kernels_are_all_there(asm):
  ks = _kernels(asm)
  # packed, plain and general x step, rollout and reset, the shaped step kernel and the compiled-rules headline
  assert sum(1 for k in ks if HEADLINE in k) == 1
  assert len(ks) == 3 * 3 + 2, sorted(ks)
  # the group kernels run the same island prologue as member bodies: at least no load of theirs lost its address space
  groups = [m.end() for m in re.finditer(r"^_ZN3sgw14k_engine_group\w*:", asm, re.M)]
  assert len(groups) == 2
  for at in groups:
    body = asm[at:]
    assert not re.search(r"^\s+flat_", body[:body.index(".Lfunc_end")], re.M)


def test_every_prologue_load_is_issued_before_the_first_wait(asm):
  bad = []
  for k, body in _kernels(asm).items():
    pro = _prologue(body)
    loads = [i for i, (op, _, _) in enumerate(pro) if LOAD.match(op)]
    waits = [i for i, (op, _, _) in enumerate(pro) if op == "s_waitcnt"]
    assert len(loads) >= 3 and waits, k
    if GENERAL in k:
      # The per-event reward vectors (init_args) are read through a.ftable, a pointer in the cold part of the argument block:
      # that scalar load and its wait cannot go ahead of the prologue without widening the kernels' preloaded arguments.  The
      # rule holds for everything else: only those 8-byte loads (at most two per thread) may follow the first wait.
      late = [pro[i] for i in loads if i > waits[0]]
      assert 1 <= len(late) <= 2 and all(op == "global_load_dwordx2" for op, _, _ in late), (k, late)
      loads = [i for i in loads if i < waits[0]]
      assert len(loads) >= 6, (k, len(loads))
    if waits[0] < loads[-1]:
      bad.append("%s: `%s %s` (instruction %d of the prologue) stands ahead of the load `%s %s` (%d)"
                 % (k, pro[waits[0]][0], pro[waits[0]][1], waits[0], pro[loads[-1]][0], pro[loads[-1]][1], loads[-1]))
    if any(op.startswith("flat_") for op, _, _ in pro):
      bad.append("%s: a flat instruction in the prologue" % k)
  assert not bad, "\n".join(bad)


def _all(body):
  out, inside = [], False
  for line in body.splitlines():
    t = line.strip()
    if t.startswith(";;#ASMSTART"): inside = True; continue
    if t.startswith(";;#ASMEND"): inside = False; continue
    m = re.match(r"(s|v|ds|global|buffer|flat|scratch)_\w+", t)
    if m and not t.endswith(":"):
      out.append((m.group(0), t[m.end():].split(";")[0].strip(), inside, SETTLE in t))
  return out


def test_the_kernarg_touch_is_split_soundly_in_every_kernel_that_has_it(asm):
  checked = 0
  for m in re.finditer(r"^(_ZN3sgw8k_engineI\w+):", asm, re.M):
    body = asm[m.end():]
    body = body[:body.index(".Lfunc_end")]
    if SETTLE not in body:
      continue
    k, ins = m.group(1), _all(body)
    settle = [i for i, x in enumerate(ins) if x[3]]
    assert len(settle) == 1 and ins[settle[0]][0] == "s_waitcnt" and ins[settle[0]][1].startswith("lgkmcnt(0)"), (k, settle)
    touch = [i for i, (op, _, inside, _) in enumerate(ins[:settle[0]]) if inside and op == "s_load_dword"]
    assert len(touch) >= 2, k
    dst = {ins[i][1].split(",")[0].strip() for i in touch}
    assert len(dst) == 1 and re.fullmatch(r"s\d+", next(iter(dst))), (k, dst)
    reg = next(iter(dst))
    assert ("%s free" % reg) in body, "%s: the settle statement holds another register than the touch's %s" % (k, reg)
    for op, rest, inside, _ in ins[touch[-1] + 1:settle[0]]:
      assert not inside, (k, op, rest)                                                   # no other asm statement in between
      assert int(reg[1:]) not in _written_sgprs(op, rest), "%s: `%s %s` writes the touch's SGPR before its loads have returned" % (k, op, rest)
      assert not op.startswith(("ds_read", "ds_load")), "%s: `%s %s` between the touch and its wait" % (k, op, rest)
      # a scalar load of the compiler's own with its lgkmcnt(0) settles the touch early and is harmless; a COUNTED lgkmcnt wait
      # would be one that waits for more than its author meant
      c = re.search(r"lgkmcnt\((\d+)\)", rest) if op == "s_waitcnt" else None
      assert not c or c.group(1) == "0", "%s: `%s %s` between the touch and its wait" % (k, op, rest)
      assert op not in ("s_barrier", "s_endpgm"), (k, op)
    # the wait stands ahead of the staging barrier with no memory access in between
    after = ins[settle[0] + 1:]
    bar = next((i for i, x in enumerate(after) if x[0] == "s_barrier"), 0)       # (a one-wave workgroup's barrier is no instruction)
    assert not any(LOAD.match(op) or op.startswith("ds_") for op, _, _, _ in after[:bar]), (k, after[:bar])
    assert bar <= 40, (k, bar)
    checked += 1
  assert checked >= 50, checked      # every family's step, rollout and reset kernels
