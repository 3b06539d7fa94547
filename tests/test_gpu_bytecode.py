"""The bytecode evaluator on the GPU (csrc/expr_bytecode.hip): the interpreter kernel against the Python restatement of the
reference interpreter (oracle/interp.py) and against the run-time compiled kernels on the same inputs, then whole proofs with
every step and public program interpreted -- and nothing compiled.  Every comparison is bit-exact."""
import importlib
import json
import pathlib
import sys

import numpy as np
import pytest

import test_program as TP
from test_program import T, M, N, BUF, P, _fib_like_program, _long_chain_program, _random_program, _wide_program
from test_bytecode_program import assemble, live_values_program, summary

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tools"))
D = ROOT / "tests" / "golden" / "starky_data"
OUT = {"q": 3, "cm3": 4}                                                   # the sections the builder programs write: words per row


def _uniform_kw(zk, u):
    return {k: zk.DevArray.from_host(v) if isinstance(v, np.ndarray) else v for k, v in u.items() if v is not None}


def _run(zk, prog, host, n, nbits, nxt, uni, rows=None, fill=0):
    d = {k: zk.DevArray.from_host(v) for k, v in host.items()}
    for k, w in OUT.items():
        d[k] = zk.DevArray.from_host(np.full(w * n, fill, dtype=np.uint64))
    prog.run({BUF[k]: v for k, v in d.items()}, nbits, nxt, rows=rows, **_uniform_kw(zk, uni))
    return {k: d[k].to_host() for k in OUT}


def _reference(program, host, n, nxt, uni):
    import interp
    bufs = {k: [int(v) for v in a] for k, a in host.items()}
    for k, w in OUT.items():
        bufs[k] = [0] * (w * n)
    lst = lambda a: None if a is None else [int(v) for v in a]
    f3s = lambda a: () if a is None else a.reshape(-1, 3).astype(object).tolist()
    interp.run(program, bufs, n, nxt, publics=lst(uni.get("publics")) or (), challenges=f3s(uni.get("challenges")), evals=f3s(uni.get("evals")),
               x=lst(uni.get("x")), zi=lst(uni.get("zi")), xdiv=lst(uni.get("xdiv")), xdivw=lst(uni.get("xdivw")))
    return {k: np.array(bufs[k], dtype=np.uint64) for k in OUT}


def _check_both(zk, program, host, n, nbits, nxt, uni):
    """bytecode == reference interpreter, and bytecode == the compiled program, on the same inputs; -> (bytecode program, reference)"""
    ref = _reference(program, host, n, nxt, uni)
    bc, jit = assemble(zk, program), assemble(zk, program, mode="jit")
    assert (bc.kind, jit.kind) == ("bytecode", "jit")
    got, cmp_ = _run(zk, bc, host, n, nbits, nxt, uni), _run(zk, jit, host, n, nbits, nxt, uni)
    for k in OUT:
        assert np.array_equal(got[k], ref[k]), k
        assert np.array_equal(got[k], cmp_[k]), k
    return bc, ref


@pytest.mark.parametrize("nbits,ext", [(3, 1), (6, 1), (8, 2)])
def test_fib_like_program(zk, orc, nbits, ext):
    zk.init(0)
    rng = np.random.default_rng(nbits * 10 + ext)
    n = 1 << (nbits + ext); nxt = 1 << ext
    host = {"cm1": rng.integers(0, P, size=2 * n, dtype=np.uint64), "const": rng.integers(0, 2, size=n, dtype=np.uint64)}
    uni = {"challenges": rng.integers(0, P, size=24, dtype=np.uint64), "publics": rng.integers(0, P, size=2, dtype=np.uint64),
           "zi": orc.zh_inv(nbits, ext), "x": zk.x_table(nbits + ext, 49).to_host()}
    _check_both(zk, _fib_like_program(), host, n, nbits + ext, nxt, uni)


@pytest.mark.parametrize("n_terms", [3, 700, 1300])
def test_long_horner_chains(zk, orc, n_terms):
    zk.init(0)
    nbits, ext = 4, 1
    rng = np.random.default_rng(n_terms)
    n = 1 << (nbits + ext); nxt = 1 << ext
    cm1 = rng.integers(0, P, size=2 * n, dtype=np.uint64)
    cm1[:4] = [0, P - 1, 1, P - 2]
    uni = {"challenges": rng.integers(0, P, size=24, dtype=np.uint64), "evals": rng.integers(0, P, size=12, dtype=np.uint64),
           "xdiv": rng.integers(0, P, size=3 * n, dtype=np.uint64)}
    bc, _ = _check_both(zk, _long_chain_program(n_terms), {"cm1": cm1}, n, nbits + ext, nxt, uni)
    assert summary(bc.source)[0] <= 12                                     # the accumulator, the pending term, a product and a result: four cubic values at most, whatever the length


@pytest.mark.parametrize("seed", range(24))
def test_random_programs(zk, orc, seed):
    zk.init(0)
    rng = np.random.default_rng(1000 + seed)
    nbits, ext = 4, 1
    n = 1 << (nbits + ext); nxt = 1 << ext
    program = _random_program(rng, int(rng.integers(5, 120)))
    cm1 = rng.integers(0, P, size=4 * n, dtype=np.uint64); cm1[:6] = [0, P - 1, 1, P - 2, 0, 0]
    const = rng.integers(0, P, size=2 * n, dtype=np.uint64)
    chal = rng.integers(0, P, size=24, dtype=np.uint64); evals = rng.integers(0, P, size=12, dtype=np.uint64)
    if seed % 3 == 0: chal[3:6] = [5, 0, 0]                                # a base-field valued challenge
    pub = rng.integers(0, P, size=2, dtype=np.uint64)
    xd, xdw = rng.integers(0, P, size=3 * n, dtype=np.uint64), rng.integers(0, P, size=3 * n, dtype=np.uint64)
    uni = {"challenges": chal, "evals": evals, "publics": pub, "xdiv": xd, "xdivw": xdw, "zi": orc.zh_inv(nbits, ext), "x": zk.x_table(nbits + ext, 49).to_host()}
    _check_both(zk, program, {"cm1": cm1, "const": const}, n, nbits + ext, nxt, uni)


@pytest.mark.parametrize("w_cm1,w_const,nbits", [(19, 18, 9), (40, 9, 8), (36, 8, 7), (73, 20, 8), (300, 20, 7)])
def test_wide_sections(zk, orc, w_cm1, w_const, nbits):
    zk.init(0)
    BUF["wide"] = 4
    rng = np.random.default_rng(w_cm1 * 100 + w_const)
    ext = 1
    n = 1 << (nbits + ext); nxt = 1 << ext
    program = _wide_program(rng, w_cm1, w_const)
    host = {"cm1": rng.integers(0, P, size=w_cm1 * n, dtype=np.uint64), "const": rng.integers(0, P, size=w_const * n, dtype=np.uint64),
            "wide": rng.integers(0, P, size=64 * n, dtype=np.uint64)}
    uni = {"challenges": rng.integers(0, P, size=24, dtype=np.uint64), "x": zk.x_table(nbits + ext, 49).to_host(), "zi": orc.zh_inv(nbits, ext)}
    bc, ref = _check_both(zk, program, host, n, nbits + ext, nxt, uni)
    for row0, count in [(n - 70, 70), (37, 300 if n > 400 else 100), (5, 1)]:
        got = _run(zk, bc, host, n, nbits + ext, nxt, uni, rows=(row0, count), fill=7)
        inside = np.zeros(n, dtype=bool); inside[row0:row0 + count] = True
        for k, w in OUT.items():
            g, r = got[k].reshape(n, w), ref[k].reshape(n, w)
            assert (g[inside] == r[inside]).all() and (g[~inside] == 7).all(), (k, row0, count)


def test_row_ranges_touch_only_their_rows(zk, orc):
    """rows=(row0, count): count = 1 (a public calculator's one row), counts that end inside a wave, the last rows of the domain"""
    zk.init(0)
    nbits, ext = 6, 1
    rng = np.random.default_rng(99)
    n = 1 << (nbits + ext); nxt = 1 << ext
    host = {"cm1": rng.integers(0, P, size=2 * n, dtype=np.uint64), "const": rng.integers(0, 2, size=n, dtype=np.uint64)}
    uni = {"challenges": rng.integers(0, P, size=24, dtype=np.uint64), "publics": rng.integers(0, P, size=2, dtype=np.uint64),
           "zi": orc.zh_inv(nbits, ext), "x": zk.x_table(nbits + ext, 49).to_host()}
    program = _fib_like_program()
    ref = _reference(program, host, n, nxt, uni)
    bc = assemble(zk, program)
    for row0, count in [(0, 1), (n - 1, 1), (n - 3, 3), (17, 40), (3, 100), (0, n)]:
        got = _run(zk, bc, host, n, nbits + ext, nxt, uni, rows=(row0, count), fill=7)
        inside = np.zeros(n, dtype=bool); inside[row0:row0 + count] = True
        for k, w in OUT.items():
            g, r = got[k].reshape(n, w), ref[k].reshape(n, w)
            assert (g[inside] == r[inside]).all() and (g[~inside] == 7).all(), (k, row0, count)
    with pytest.raises(zk.ZkError, match="outside the domain"):
        _run(zk, bc, host, n, nbits + ext, nxt, uni, rows=(n - 1, 2))


def test_values_in_the_arena(zk, orc):
    """400 cubic-extension values live at once: most of them past the LDS budget, in the pooled arena; expected values
    from the oracle's C interpreter"""
    import interp
    zk.init(0)
    nbits = 10
    n, nxt = 1 << nbits, 1
    rng = np.random.default_rng(400)
    program = live_values_program(400)
    cm1 = rng.integers(0, P, size=2 * n, dtype=np.uint64)
    chal = rng.integers(0, P, size=24, dtype=np.uint64)
    x = zk.x_table(nbits, 49).to_host()
    bc = assemble(zk, program)
    assert summary(bc.source)[2] > 0
    got = _run(zk, bc, {"cm1": cm1}, n, nbits, nxt, {"challenges": chal, "x": x})
    bufs = {"cm1": cm1.copy(), "q": np.zeros(3 * n, dtype=np.uint64)}
    interp.run_c(orc.lib, program, bufs, n, nxt, challenges=chal, x=x)
    assert np.array_equal(got["q"], bufs["q"])
    assert np.array_equal(_run(zk, bc, {"cm1": cm1}, n, nbits, nxt, {"challenges": chal, "x": x})["q"], bufs["q"])   # the arena reused


def test_primed_reads_wrap_at_the_end_of_the_domain(zk, orc):
    """rows n - next .. n - 1 read rows 0 .. next - 1: the last wave of the domain"""
    zk.init(0)
    nbits, ext = 7, 2
    n = 1 << (nbits + ext); nxt = 1 << ext
    rng = np.random.default_rng(5)
    cm1 = rng.integers(0, P, size=2 * n, dtype=np.uint64)
    program = [("copy", T(0), M("cm1", 1, 2, prime=True), None),
               ("copy", M("cm3", 0, 4), T(0), None),
               ("sub", T(1), M("cm1", 0, 2, prime=True), M("cm1", 0, 2)),
               ("mul", M("q", 0, 3, dim=3), {"kind": "challenge", "id": 1}, T(1))]
    uni = {"challenges": rng.integers(0, P, size=24, dtype=np.uint64)}
    ref = _reference(program, {"cm1": cm1}, n, nxt, uni)
    bc = assemble(zk, program)
    got = _run(zk, bc, {"cm1": cm1}, n, nbits + ext, nxt, uni)
    rows = cm1.reshape(n, 2)
    assert np.array_equal(got["cm3"].reshape(n, 4)[n - nxt:, 0], rows[:nxt, 1])            # the values themselves, not only "what the reference says"
    assert np.array_equal(got["cm3"].reshape(n, 4)[:n - nxt, 0], rows[nxt:, 1])
    assert np.array_equal(got["q"], ref["q"]) and np.array_equal(got["cm3"], ref["cm3"])
    last = _run(zk, bc, {"cm1": cm1}, n, nbits + ext, nxt, uni, rows=(n - nxt, nxt))       # only those rows: the same values
    assert np.array_equal(last["q"].reshape(n, 3)[n - nxt:], ref["q"].reshape(n, 3)[n - nxt:])


# ---- whole proofs ----------------------------------------------------------------------------------------------------------
from test_gpu_stark_prove import CASES, GL_STRUCT, BN128_STRUCT, BN128_CASES, PROVER_ADDR


def _stark(zk):
    zk.init(0)
    return importlib.import_module("eigen_zkvm_amd.stark")


def _jit_stats(zk):
    o = np.zeros(3, np.uint64); zk.lib().zk_jit_cache_stats(o.ctypes.data); return [int(v) for v in o]


def _assert_nothing_compiled(ns):
    t = ns.setup_timing()
    assert t["eval_mode"] == "bytecode" and t["bytecode_programs"] >= 3
    assert (t["hiprtc_compiled"], t["code_cache_disk_hits"], t["code_cache_mem_hits"]) == (0, 0, 0)
    assert t["hiprtc_processes"] == 0


@pytest.mark.parametrize("name", list(CASES))
def test_gl_proofs_in_bytecode_mode_equal_the_oracle(zk, orc, monkeypatch, name):
    import stark_prover as SP
    import starkinfo as SI
    monkeypatch.setenv("ZK_JIT_CACHE", "off")
    stark = _stark(zk)
    pil_f, const_f, cm_f = CASES[name]
    su = SP.setup(json.load(open(D / pil_f)), D / const_f, GL_STRUCT, orc)
    exp = SP.to_zkin(SP.stark_gen(D / cm_f, su, GL_STRUCT, orc))
    before = _jit_stats(zk)
    ns = stark.NativeStarkSetup(np.fromfile(D / const_f, dtype="<u8"), json.dumps(SI.to_json(su["starkinfo"], su["program"])), json.dumps(GL_STRUCT),
                                eval_mode="bytecode")
    _assert_nothing_compiled(ns)
    got = ns.gen(np.fromfile(D / cm_f, dtype="<u8"))
    assert list(got.keys()) == list(exp.keys())
    assert json.dumps(got) == json.dumps(exp)                                # byte-equal zkin
    assert ns.gen(np.fromfile(D / cm_f, dtype="<u8"))  == got               # a second proof of the same setup
    assert _jit_stats(zk) == before                                          # proving compiled nothing either
    assert ns.verify(got) is True
    ns.free()


def test_bn128_proof_in_bytecode_mode_equals_the_oracle(zk, orc, monkeypatch):
    """scalar-field hashing: the publics and the transcript are untouched by the choice of evaluator"""
    import stark_prover as SP
    import starkinfo as SI
    monkeypatch.setenv("ZK_JIT_CACHE", "off")
    stark = _stark(zk)
    pil_f, const_f, cm_f = BN128_CASES["fibonacci"]
    b = SP.BN128Backend(orc)
    su = SP.setup(json.load(open(D / pil_f)), D / const_f, BN128_STRUCT, b)
    exp = SP.to_zkin_bn128(SP.stark_gen(D / cm_f, su, BN128_STRUCT, b), b, PROVER_ADDR)
    ns = stark.NativeStarkSetup(np.fromfile(D / const_f, dtype="<u8"), json.dumps(SI.to_json(su["starkinfo"], su["program"])), json.dumps(BN128_STRUCT),
                                prover_addr=PROVER_ADDR, eval_mode="bytecode")
    _assert_nothing_compiled(ns)
    got = ns.gen(np.fromfile(D / cm_f, dtype="<u8"))
    assert list(got.keys()) == list(exp.keys())
    for k in exp:
        assert got[k] == exp[k], k
    assert ns.gen(np.fromfile(D / cm_f, dtype="<u8")) == got
    ns.free()


def test_poseidong_2p12_in_bytecode_mode_equals_the_oracle(zk, orc, monkeypatch):
    """PoseidonG, built as tests/test_gpu_round4.py builds it: step programs of thousands of instructions, slots past the LDS budget"""
    import stark_prover as SP, starkinfo as SI, poseidong as PG
    monkeypatch.setenv("ZK_JIT_CACHE", "off")
    stark = _stark(zk)
    nbits, ext_bits = 12, 2
    ss, const = PG.stark_struct(nbits, ext_bits=ext_bits), PG.consts(nbits)
    cm = PG.trace(nbits, None, PG.FIRST_COUNT, seed=nbits)
    su = SP.setup(PG.pil(nbits), const, ss, orc)
    exp = SP.to_zkin(SP.stark_gen(cm, su, ss, orc))
    ns = stark.NativeStarkSetup(const, json.dumps(PG.program(nbits, ss)), json.dumps(ss), eval_mode="bytecode")
    _assert_nothing_compiled(ns)
    got = ns.gen(zk.DevArray.from_host(cm))
    assert list(got) == list(exp)
    for k in exp:
        assert got[k] == exp[k], k
    assert ns.gen(cm) == got
    assert ns.verify(got) is True
    ns.free()


def test_a_jit_setup_and_a_bytecode_setup_side_by_side(zk, orc):
    """two setups of one PIL alive in one process, one per evaluator: the same zkin, and the thread's mode is left as it was"""
    import stark_prover as SP
    import starkinfo as SI
    stark = _stark(zk)
    pil_f, const_f, cm_f = CASES["plookup_gl"]
    su = SP.setup(json.load(open(D / pil_f)), D / const_f, GL_STRUCT, orc)
    text = json.dumps(SI.to_json(su["starkinfo"], su["program"]))
    const, cm = np.fromfile(D / const_f, dtype="<u8"), np.fromfile(D / cm_f, dtype="<u8")
    mode0 = zk.set_eval_mode("jit"); zk.set_eval_mode(mode0)
    a = stark.NativeStarkSetup(const, text, json.dumps(GL_STRUCT), eval_mode="jit")
    b = stark.NativeStarkSetup(const, text, json.dumps(GL_STRUCT), eval_mode="bytecode")
    assert zk.set_eval_mode(mode0) == mode0
    ta, tb = a.setup_timing(), b.setup_timing()
    assert (ta["eval_mode"], ta["bytecode_programs"]) == ("jit", 0) and tb["eval_mode"] == "bytecode" and tb["bytecode_programs"] >= 3
    za, zb = a.gen(cm), b.gen(cm)
    assert json.dumps(za) == json.dumps(zb)
    assert json.dumps(b.gen(cm)) == json.dumps(a.gen(cm)) == json.dumps(za)
    a.free(); b.free()
