"""The bytecode evaluator's host side (csrc/expr_bytecode.hip zk_program_assemble): a step program becomes bytecode for the
interpreter kernel inside libzkgpu -- no GPU, no hipRTC, no helper process.  What the assembler decided is read from the
listing zk_program_source returns: one line per instruction, then "; slots: <words> (lds <words>, arena <words>), ..."."""
import os
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import test_program as TP
from test_program import T, M, N, BUF, _fib_like_program

ROOT = pathlib.Path(__file__).resolve().parent.parent


def assemble(zk, program, mode="bytecode"):
    ops = {"add": zk.OP_ADD, "sub": zk.OP_SUB, "mul": zk.OP_MUL, "copy": zk.OP_COPY}
    return zk.Program([zk.instr(ops[op], TP._conv(zk, d), TP._conv(zk, a), TP._conv(zk, b) if b else None)
                       for op, d, a, b in program], mode=mode)


def summary(listing):
    """-> (slots, lds, arena) of the summary line"""
    m = re.search(r"^; slots: (\d+) words \(lds (\d+), arena (\d+)\)", listing.splitlines()[-1])
    assert m, listing.splitlines()[-1]
    return tuple(int(g) for g in m.groups())


def live_values_program(n_live=400):
    """n_live cubic-extension values, all live at once (each is read only after the last one was written), summed into q"""
    ch = lambda i: {"kind": "challenge", "id": i}
    prog = [("mul", T(k), ch(k % 8), M("cm1", k % 2, 2, prime=bool(k % 3 == 0))) for k in range(n_live)]
    prog.append(("add", T(n_live), T(0), T(1)))
    for k in range(2, n_live):
        prog.append(("add", T(n_live + k - 1), T(n_live + k - 2), T(k)))
    prog.append(("mul", M("q", 0, 3, dim=3), T(2 * n_live - 2), {"kind": "x"}))
    return prog


def _stats(zk):
    o = np.zeros(3, np.uint64); zk.lib().zk_jit_cache_stats(o.ctypes.data); return [int(v) for v in o]


def test_assembling_needs_no_gpu_and_no_compiler(zk):
    before = _stats(zk)
    prog = assemble(zk, _fib_like_program())
    assert _stats(zk) == before                                             # nothing compiled, nothing looked up
    assert prog.kind == "bytecode" and zk.lib().zk_program_kind(prog._h) == 1


def test_listing_has_one_line_per_instruction_and_static_dims(zk):
    program = _fib_like_program()
    lines = assemble(zk, program).source.splitlines()
    assert len(lines) == len(program) + 1 and lines[-1].startswith("; slots:")
    ops = [l.split()[1] for l in lines[:-1]]
    assert [l.split()[0] for l in lines[:-1]] == [str(k) for k in range(len(program))]
    assert ops[8] == "mul31" and ops[9] == "add31" and ops[10] == "mul33" and ops[11] == "sub13"   # vc * t6, t8 + t7, vc * t9, public - t10
    assert ops[0] == "mul11" and ops[13] == "copy1" and ops[14] == "copy3" and ops[15] == "mul31"
    assert all(o[:-2] == op[:3] or o[:-1] == op for o, (op, *_r) in zip(ops, program))


def test_slots_follow_liveness_not_tmp_ids(zk):
    prog = []
    for k in range(5000):                                                   # t[k+1] = t[k] * cm + t[k]: 10 000 instructions, 10 000 tmp ids
        src = T(2 * k - 1) if k else M("cm1", 1, 2)
        prog.append(("mul", T(2 * k), src, M("cm1", 0, 2)))
        prog.append(("add", T(2 * k + 1), T(2 * k), src))
    prog.append(("copy", M("cm3", 0, 4), T(9999), None))
    slots, lds, arena = summary(assemble(zk, prog).source)
    assert slots <= 4 and arena == 0 and lds == slots


def test_values_past_the_lds_budget_go_to_the_arena(zk):
    listing = assemble(zk, live_values_program(400)).source
    slots, lds, arena = summary(listing)
    assert arena > 0 and lds > 0 and slots == lds + arena and slots >= 3 * 400
    assert re.search(r"\bA\d+:3\b", listing) and re.search(r"\bL\d+:3\b", listing)


def test_rejections_are_the_translators(zk):
    """the cases and messages of test_program.py::test_program_rejects_bad_code"""
    with pytest.raises(zk.ZkError, match="tmp read before write"):
        assemble(zk, [("add", T(1), T(0), N(1))])
    with pytest.raises(zk.ZkError, match="written at one row and read at the next row"):
        assemble(zk, [("copy", M("cm3", 0, 4), N(1), None), ("copy", T(0), M("cm3", 0, 4, prime=True), None)])
    with pytest.raises(zk.ZkError, match="written at one row and read at the next row"):
        assemble(zk, [("copy", M("cm3", 0, 4, prime=True), N(1), None), ("copy", T(0), M("cm3", 0, 4), None)])
    with pytest.raises(zk.ZkError, match="written at one row and read at the next row"):
        assemble(zk, [("copy", T(0), {"kind": "challenge", "id": 4}, None), ("copy", M("cm3", 0, 4, dim=3), T(0), None), ("copy", T(1), M("cm3", 1, 4, prime=True), None)])
    assemble(zk, [("copy", M("cm3", 0, 4, prime=True), N(1), None), ("copy", T(0), M("cm3", 0, 4, prime=True), None), ("copy", M("q", 0, 3), T(0), None)])
    import ctypes as C
    assert not zk.lib().zk_program_assemble(C.cast(None, C.POINTER(zk.Instr)), 3)
    assert b"null code" in zk.lib().zk_last_error()


def test_partial_overlap_of_an_own_write_is_accepted(zk):
    """the translator hoists reads and must reject this; the interpreter runs in program order"""
    program = [("copy", T(0), {"kind": "challenge", "id": 4}, None), ("copy", M("cm3", 0, 4, dim=3), T(0), None), ("copy", T(1), M("cm3", 1, 4), None)]
    with pytest.raises(zk.ZkError, match="partially overlaps an earlier write"):
        assemble(zk, program, mode="jit")
    assert assemble(zk, program).kind == "bytecode"


def test_program_kind(zk):
    small = [("add", T(0), M("cm1", 0, 2), N(1)), ("copy", M("cm3", 0, 4), T(0), None)]
    a, c = assemble(zk, small), assemble(zk, small, mode="jit")
    assert (zk.lib().zk_program_kind(a._h), zk.lib().zk_program_kind(c._h)) == (1, 0)
    assert (a.kind, c.kind) == ("bytecode", "jit")
    assert "zk_eval_kernel" in c.source and "zk_eval_kernel" not in a.source
    with pytest.raises(zk.ZkError):
        assemble(zk, small, mode="fast")


def test_set_eval_mode_returns_the_previous_mode(zk):
    first = zk.set_eval_mode("bytecode")
    try:
        assert zk.set_eval_mode("jit") == "bytecode"
        assert zk.set_eval_mode("bytecode") == "jit"
        assert zk.lib().zk_eval_set_mode(7) == -1 and zk.set_eval_mode("bytecode") == "bytecode"   # an unknown mode changes nothing
    finally:
        zk.set_eval_mode(first)


_MODE_PROBE = r'''
import sys, pathlib
ROOT = pathlib.Path(sys.argv[1]); sys.path.insert(0, str(ROOT / "tests"))
import zkgpu_loader
zk = zkgpu_loader.load()
print("initial", zk.set_eval_mode("jit"))
'''


@pytest.mark.parametrize("env,expected", [("bytecode", "bytecode"), ("jit", "jit"), (None, "jit")])
def test_initial_mode_comes_from_the_environment(env, expected):
    e = {k: v for k, v in os.environ.items() if k != "ZK_EVAL"}
    if env is not None:
        e["ZK_EVAL"] = env
    r = subprocess.run([sys.executable, "-c", _MODE_PROBE, str(ROOT)], capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["initial", expected]
