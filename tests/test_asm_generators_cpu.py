"""The scheduled asm blocks of the leaf hash's row, lane and pair forms (csrc/*_asm.inc) are generated: each generator schedules its
blocks under the gfx950 wait-state rules, checks the rules on the result and executes every block with an interpreter of the
instructions used against the Poseidon round in Python integers.  Here: the generators pass their own checks, and the files
in the tree are what they produce (an edit by hand, or a generator changed without regenerating, fails)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


@pytest.mark.parametrize("tool,inc", [("gen_row_layer_asm.py", "row_layer_asm.inc"), ("gen_row_round_asm.py", "row_round_asm.inc"),
                                      ("gen_lane_round_asm.py", "lane_round_asm.inc"), ("gen_pair_round_asm.py", "pair_round_asm.inc")])
def test_generated_asm_is_current_and_self_checked(tool, inc):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]   # hazard rules and the interpreter's comparison are assertions inside
    have = open(os.path.join(ROOT, "starky_bls12_381_amd", "csrc", inc)).read()
    assert out.stdout == have


# ---------------------------------------------------------------- the generators' own checks can fail (tools/asm_blocks.py)
import dataclasses  # noqa: E402
import importlib  # noqa: E402
import itertools  # noqa: E402
import random  # noqa: E402
import re  # noqa: E402

TOOLS = os.path.join(ROOT, "tools")
GENERATORS = ("gen_row_round_asm", "gen_lane_round_asm", "gen_pair_round_asm")


def fresh_import(*names):
    """the named tools modules, imported anew in this order"""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    for n in ("asm_blocks",) + GENERATORS:
        sys.modules.pop(n, None)
    return [importlib.import_module(n) for n in names]


AB, = fresh_import("asm_blocks")
HW = AB.Hazards(valu_raw=1, sgpr_raw=3, dpp_read=3, war=2, war_load=1, load_latency=16, mfma_result=20, mfma_spacing=9, mfma_operand=3, mfma_war=6)
PIPE = AB.MFMA_PIPE


def nops(n):
    return [AB.Ins("s_nop 0", kind=AB.NOP) for _ in range(n)]


def mfma(reads, tile):
    return AB.Ins("mfma", list(reads) + [PIPE], [tile, tile + 1, PIPE], kind=AB.MFMA, junk=[tile + 2])


def rejected(rule, order, inputs=frozenset()):
    with pytest.raises(AssertionError, match=rule):
        AB.check_hazards(order, HW, inputs)
    return True


def test_checker_w1_sgpr_read_after_valu_write():
    write, read = AB.Ins("w", [1], [2], swrites=[44]), AB.Ins("r", [3], [4], sreads=[44])
    assert rejected("W1", [write, read]) and rejected("W1", [write] + nops(1) + [read])
    AB.check_hazards([write] + nops(2) + [read], HW)


@pytest.mark.parametrize("kind", ["dpp", "swap"])
def test_checker_w2_cross_lane_read_after_write(kind):
    write, read = AB.Ins("w", [1], [2]), AB.Ins("x", [2], [3], kind=kind)
    assert rejected("W2", [write, read]) and rejected("W2", [write] + nops(1) + [read])
    AB.check_hazards([write] + nops(2) + [read], HW)
    assert rejected("W2", [read], inputs={2}) and rejected("W2", nops(1) + [read], inputs={2})   # the caller may have written it just before the block
    AB.check_hazards(nops(2) + [read], HW, inputs={2})
    AB.check_hazards([read], HW, inputs={7})


def test_checker_w3_write_right_after_read():
    read, write = AB.Ins("r", [1], [2]), AB.Ins("w", [3], [1])
    assert rejected("W3", [read, write])
    AB.check_hazards([read] + nops(1) + [write], HW)
    AB.check_hazards([read, AB.Ins("ds_read", [3], [1], kind=AB.LOAD)], HW)


def test_checker_mfma_rules():
    use = AB.Ins("r", [10], [30])
    assert rejected("result read too early", [mfma([1], 10)] + nops(18) + [use])
    AB.check_hazards([mfma([1], 10)] + nops(19) + [use], HW)
    feed = AB.Ins("w", [5], [1])
    assert rejected("operand written too late", [feed] + nops(1) + [mfma([1], 10)])
    AB.check_hazards([feed] + nops(2) + [mfma([1], 10)], HW)
    assert rejected("operand overwritten too early", [mfma([1], 10)] + nops(4) + [feed])
    AB.check_hazards([mfma([1], 10)] + nops(5) + [feed], HW)
    assert rejected("MFMAs too close", [mfma([1], 10)] + nops(7) + [mfma([2], 20)])
    AB.check_hazards([mfma([1], 10)] + nops(8) + [mfma([2], 20)], HW)
    assert rejected("junk row", [mfma([1], 10)] + nops(30) + [AB.Ins("r", [12], [30])])
    assert rejected("junk row is still to land", [mfma([1], 10)] + nops(10) + [AB.Ins("w", [5], [12])])


def test_scheduler_keeps_every_distance_and_pads_only_when_nothing_is_ready():
    t = AB.Hazards(valu_raw=2, sgpr_raw=6, dpp_read=4, war=3, war_load=1, load_latency=8, mfma_result=12, mfma_spacing=9, mfma_operand=5, mfma_war=7)
    prog = [AB.Ins("p0", [], [1], swrites=[44]),
            AB.Ins("p1", [1], [2]),
            AB.Ins("p2", [], [3], sreads=[44]),
            AB.Ins("p3", [2], [4], kind=AB.DPP),
            AB.Ins("p4", [0], [5], kind=AB.LOAD, boost=True),
            AB.Ins("p5", [5], [6]),
            AB.Ins("p6", [], [1]),
            mfma([6], 10),
            AB.Ins("p8", [10], [13]),
            mfma([3], 20),
            AB.Ins("p10", [], [6]),
            AB.Ins("p11", [0], [2], kind=AB.LOAD, boost=True)]
    edges = [(0, 1, t.valu_raw), (0, 2, t.sgpr_raw), (1, 3, t.dpp_read), (4, 5, t.load_latency), (0, 6, 1), (1, 6, t.war), (5, 7, t.mfma_operand),
             (7, 8, t.mfma_result), (7, 9, t.mfma_spacing), (2, 9, t.mfma_operand), (5, 10, 1), (7, 10, t.mfma_war), (1, 11, 1), (3, 11, t.war_load)]
    order = AB.schedule(prog, t)
    pos = {i: order.index(p) for i, p in enumerate(prog)}
    assert sorted(pos.values()) == [s for s, o in enumerate(order) if o.kind != AB.NOP]    # every instruction once, everything else is s_nop
    for p, c, d in edges:
        assert pos[c] - pos[p] >= d, (p, c, d, pos)
    for s, o in enumerate(order):
        if o.kind == AB.NOP:
            for i in range(len(prog)):
                assert pos[i] < s or any(c == i and pos[p] + d > s for p, c, d in edges), ("s_nop in slot %d although p%d was ready" % (s, i), pos)
    assert any(o.kind == AB.NOP for o in order)    # (this program cannot be packed: the padding rule above was exercised)
    assert pos[4] == 0 and pos[8] - pos[7] == t.mfma_result


def test_block_scheduled_with_a_weaker_table_is_rejected():
    L, = fresh_import("gen_lane_round_asm")
    AB.check_hazards(L.schedule(L.block_partial_mfma()), L.HAZARDS)
    for weaker, rule in ((dict(sgpr_raw=1), "W1"), (dict(war=1), "W3"), (dict(mfma_operand=1), "operand written too late"), (dict(mfma_spacing=4), "MFMAs too close")):
        with pytest.raises(AssertionError, match=rule):
            AB.check_hazards(L.schedule(L.block_partial_mfma(), dataclasses.replace(L.HAZARDS, **weaker)), L.HAZARDS)


def test_interpreter_rejects_a_wrong_block(monkeypatch):
    L, = fresh_import("gen_lane_round_asm")
    random.seed(5)
    L.test_round(L.schedule(L.block_full()), False)
    monkeypatch.setattr(L, "CIRC", L.CIRC[:3] + [L.CIRC[3] + 1] + L.CIRC[4:])    # the block builder's copy; the reference keeps asm_blocks.CIRC
    with pytest.raises(AssertionError):
        L.test_round(L.schedule(L.block_full()), False)


@pytest.mark.parametrize("names", list(itertools.permutations(GENERATORS)), ids=lambda names: "-".join(n.split("_")[1] for n in names))
def test_generators_do_not_depend_on_import_order(names):
    mods = dict(zip(names, fresh_import(*names)))
    G, L, Q = (mods[n] for n in GENERATORS)
    random.seed(1)
    order = G.AB.schedule(G.block_partial(), G.HAZARDS)
    G.AB.check_hazards(order, G.HAZARDS, {G.S_LO, G.S_HI} | set(G.SEEDS))
    G.test(order, True)
    L.test_round(L.schedule(L.block_partial()), True)
    L.test_round_mfma(L.schedule(L.block_partial_mfma()), True)
    Q.test_round_pair(Q.schedule_pair(Q.block_partial_pair(), Q.ROUND_LOAD_LATENCY), True)
    Q.test_four_pair(Q.schedule_pair(Q.block_four_pair(), Q.FOUR_LOAD_LATENCY))


def test_no_configuration_by_assignment_and_no_guessing_of_instruction_kinds():
    for name in ("asm_blocks",) + GENERATORS:
        src = open(os.path.join(TOOLS, name + ".py")).read()
        assert not re.search(r"^\s*(G|L|AB)\.[A-Za-z_]+ *=[^=]", src, re.M), name
        assert "getattr(" not in src and ".startswith(" not in src, name
