"""wtns_check on the GPU (csrc/r1cs_check.hip behind zk_r1cs_check_*): the device's report against the plain-Python checker
(tests/r1cs_check_ref.py), the whole report and exactly -- these are integers, there is no tolerance.  The circuits are those of
tests/r1cs_check_cases.py and tests/c12_setup_circuits.py; tests/test_r1cs_check_host.py shows on the CPU that each corruption is
the case its name says."""
import functools
import importlib
import json
import pathlib
import random
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import c12_setup_circuits as CIRC  # noqa: E402
import c12_setup_ref as REF  # noqa: E402
import r1cs_check_cases as CASES  # noqa: E402
import r1cs_check_ref as RC  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = ROOT / "tests" / "golden" / "groth16"


@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)
    return importlib.import_module("eigen_zkvm_amd.r1cs")


@functools.lru_cache(maxsize=None)
def _products(field, n):
    b, w, outs = CASES.products(field, n)
    return b, w, outs, RC.circuit(field, b)


@functools.lru_cache(maxsize=None)
def _shapes(field):
    b, w, long_row, cw = CASES.shapes(field)
    return b, w, long_row, cw, RC.circuit(field, b)


@functools.lru_cache(maxsize=None)
def _custom(kind):
    b, w = CIRC.with_custom(kind)
    return b, w, RC.circuit("GL", b)


def both(dev, field, b, circ, w, max_findings=16):
    """-> the device's report, after comparing it with the restatement's"""
    chk = dev.R1csCheck(field, b)
    try:
        rep = chk.run(w, max_findings=max_findings)
    finally:
        chk.free()
    assert rep == RC.check(circ, w, max_findings)
    return rep


# ---- boundaries of the mask, the wave and the workgroup -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("field", CASES.FIELDS)
def test_satisfied(dev, field, n):
    b, w, outs, circ = _products(field, n)
    chk = dev.R1csCheck(field, b)
    assert chk.info == {"n_wires": len(w), "n_constraints": n, "n_custom_uses": 0, "n_public": 1}
    rep = chk.run(w)
    chk.free()
    assert rep["findings"] == [] and not any(rep["n_failing"].values())
    assert rep == RC.check(circ, w)


@pytest.mark.parametrize("n,at", [(1, 0), (64, 63), (65, 64), (257, 0), (257, 63), (257, 64), (257, 256)])
@pytest.mark.parametrize("field", CASES.FIELDS)
def test_one_broken_constraint(dev, field, n, at):
    b, w, outs, circ = _products(field, n)
    rep = both(dev, field, b, circ, CASES.corrupt(w, outs[at], p=circ["p"]))
    assert [f["index"] for f in rep["findings"]] == [at] and rep["n_failing"]["constraint"] == 1


@pytest.mark.parametrize("field", CASES.FIELDS)
def test_200_of_1000_rows_fail(dev, field):
    b, w, outs, circ = _products(field, 1000)
    bad = sorted(random.Random(9).sample(range(1000), 200))
    w = list(w)
    for i in bad: w[outs[i]] = (w[outs[i]] + 1) % circ["p"]
    rep = both(dev, field, b, circ, w, max_findings=16)
    assert [f["index"] for f in rep["findings"]] == bad[:16] and rep["n_failing"]["constraint"] == 200
    assert both(dev, field, b, circ, w, max_findings=0)["n_failing"]["constraint"] == 200


# ---- row shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", CASES.FIELDS)
def test_row_shapes(dev, field):
    b, w, long_row, cw, circ = _shapes(field)
    assert both(dev, field, b, circ, w)["findings"] == []
    (f,) = both(dev, field, b, circ, CASES.corrupt(w, cw, p=circ["p"]))["findings"]
    assert (f["index"], f["a"], f["b"], f["c"]) == (long_row, "1000", "1", "1001")
    # every short row broken at once: one wire of each (the rows of 1, 4, 5 and 9 terms read wires 0..12)
    rep = both(dev, field, b, circ, CASES.corrupt(w, 3, p=circ["p"]))
    assert rep["n_failing"]["constraint"] >= 1


@pytest.mark.parametrize("field", CASES.FIELDS)
def test_one_wire_alone(dev, field):
    b, w, outs, circ = _products(field, 65)
    rep = both(dev, field, b, circ, [2] + list(w[1:]))
    assert rep["findings"] == [{"kind": "one_wire", "value": "2"}] and rep["n_failing"]["one_wire"] == 1 and rep["n_failing"]["constraint"] == 0


# ---- the reference's fixtures ------------------------------------------------------------------------------------------------
def test_reference_r1cs_fixture(dev):
    b = (GOLD / "mycircuit_bls12381.r1cs").read_bytes()
    circ = RC.circuit("BLS12381", b)
    assert both(dev, "BLS12381", b, circ, [1, 33, 3, 11])["findings"] == []
    (f,) = both(dev, "BLS12381", b, circ, [1, 34, 3, 11])["findings"]
    assert f["index"] == 0 and int(f["a"]) * int(f["b"]) % circ["p"] != int(f["c"])


def test_reference_witness_fixture(dev):
    wt = (GOLD / "witness.wtns").read_bytes()
    values, n = dev.wtns_payload(wt, "BN128")
    assert n == 4
    b = CASES.one_constraint("BN128")
    circ = RC.circuit("BN128", b)
    chk = dev.R1csCheck("BN128", b)
    rep = chk.run(values)                                                   # the file's bytes as they are
    assert rep == RC.check(circ, [1, 11210000, 1121, 10000]) and rep["findings"] == []
    p = circ["p"]
    rep = chk.run([1, 11210001, 1121, 10000])
    chk.free()
    (f,) = rep["findings"]
    assert (int(f["a"]), int(f["b"]), int(f["c"])) == (p - 1121, 10000, p - 11210001)
    assert rep == RC.check(circ, [1, 11210001, 1121, 10000])


# ---- custom gates ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cmuladd", "poseidon", "fft4", "evpol4"])
def test_custom_gate_accepted(dev, kind):
    b, w, circ = _custom(kind)
    rep = both(dev, "GL", b, circ, w)
    assert rep["findings"] == [] and not any(rep["n_failing"].values())
    assert sum(rep["checked"][k] for k in RC.GATE_KINDS) == (2 if kind == "fft4" else 1)


@pytest.mark.parametrize("kind,use,signal", [
    ("cmuladd", 0, 0), ("cmuladd", 0, 11), ("poseidon", 0, 0), ("poseidon", 0, 371), ("poseidon", 0, 15 * 12 + 5),
    ("fft4", 0, 0), ("fft4", 0, 23), ("fft4", 1, 0), ("fft4", 1, 23), ("evpol4", 0, 0), ("evpol4", 0, 20)])
def test_custom_gate_one_wrong_signal(dev, kind, use, signal):
    b, w, circ = _custom(kind)
    sig = circ["uses"][use][1]
    rep = both(dev, "GL", b, circ, CASES.corrupt(w, sig[signal]))
    (f,) = rep["findings"]
    assert f["use"] == use and rep["n_failing"]["constraint"] == 0
    if kind == "poseidon" and signal == 15 * 12 + 5:                        # breaks transitions 14 and 15: the finding names 14
        assert (f["row"], f["column"], f["wire"]) == (14, 5, sig[signal])


def test_two_uses_second_bad(dev):
    """two CMulAdd uses and two Poseidon12 uses in one circuit; only the second of each is wrong"""
    rng = random.Random(11)
    b0, w = CIRC.plain_circuit(seed=4)
    r1 = REF.read_r1cs(b0)
    uses = []
    def fresh(vals):
        ids = list(range(len(w), len(w) + len(vals))); w.extend(vals); return ids
    for _ in range(2):
        x = [rng.randrange(REF.P) for _ in range(9)]; m = CIRC.cmul(x[0:3], x[3:6])
        uses.append((0, fresh(x + [(m[i] + x[6 + i]) % REF.P for i in range(3)])))
    for _ in range(2):
        uses.append((1, fresh([v for row in CIRC.poseidon_rows([rng.randrange(REF.P) for _ in range(12)]) for v in row])))
    b = REF.write_r1cs(len(w), 0, 3, len(w) - 4, r1["constraints"], list(CIRC.ALL_TEMPLATES), uses)
    circ = RC.circuit("GL", b)
    assert both(dev, "GL", b, circ, w)["findings"] == []
    bad = CASES.corrupt(CASES.corrupt(w, uses[1][1][10]), uses[3][1][40])
    rep = both(dev, "GL", b, circ, bad)
    assert [(f["kind"], f["use"]) for f in rep["findings"]] == [("cmuladd", 1), ("poseidon12", 3)]
    assert rep["n_failing"]["cmuladd"] == 1 and rep["n_failing"]["poseidon12"] == 1


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors(zk, dev):
    b, w, outs, circ = _products("BN128", 5)
    bg, wg, _, cg = _products("GL", 5)
    def good():
        assert both(dev, "BN128", b, circ, w)["findings"] == [] and both(dev, "GL", bg, cg, wg)["findings"] == []
    chk = dev.R1csCheck("BN128", b)
    with pytest.raises(zk.ZkError, match="the witness has 9 values, the circuit has 10 wires"):
        chk.run(w[:-1])
    good()
    with pytest.raises(zk.ZkError, match="groth16: witness value 3 is not a canonical field element"):
        chk.run(w[:3] + [circ["p"]] + w[4:])
    chk.free(); good()
    chk = dev.R1csCheck("GL", bg)
    with pytest.raises(zk.ZkError, match="witness value 2 is not a canonical field element"):
        chk.run(np.array(wg[:2] + [REF.P] + wg[3:], dtype=np.uint64))
    chk.free(); good()
    with pytest.raises(zk.ZkError, match="field size 8 is not 32 bytes"):
        dev.R1csCheck("BN128", bg)
    good()
    with pytest.raises(zk.ZkError, match="Different prime"):
        dev.R1csCheck("GL", b)
    with pytest.raises(zk.ZkError, match="not the scalar field of the selected curve"):
        dev.R1csCheck("BLS12381", b)
    with pytest.raises(zk.ZkError, match="unknown field"):
        dev.R1csCheck("BN254", b)
    good()
    for field, blob in (("BN128", b), ("GL", bg)):
        with pytest.raises(zk.ZkError, match="truncated file"):
            dev.R1csCheck(field, blob[:-5])
    with pytest.raises(zk.ZkError, match="custom gates in a file over a 32-byte field"):
        dev.R1csCheck("BN128", CASES.write("BN128", 30, [([(1, 1)], [(2, 1)], [(3, 1)])], [("CMulAdd", [])], [(0, list(range(1, 13)))]))
    with pytest.raises(zk.ZkError, match="Invalid custom gate Rescue"):
        dev.R1csCheck("GL", CASES.write("GL", 30, [([(1, 1)], [(2, 1)], [(3, 1)])], [("Rescue", [])], []))
    with pytest.raises(zk.ZkError, match="wire index out of range"):
        dev.R1csCheck("GL", CASES.write("GL", 30, [([(1, 1)], [(2, 1)], [(3, 1)])], [("CMulAdd", [])], [(0, list(range(20, 32)))]))
    with pytest.raises(zk.ZkError, match="wire index out of range"):
        dev.R1csCheck("BN128", CASES.write("BN128", 30, [([(30, 1)], [(2, 1)], [(3, 1)])]))
    good()


# ---- a witness that is already on the device ---------------------------------------------------------------------------------
@pytest.mark.parametrize("field", CASES.FIELDS)
def test_device_witness_gives_the_same_report(zk, dev, field):
    b, w, outs, circ = _products(field, 257)
    bad = CASES.corrupt(w, outs[64], p=circ["p"])
    fs = CASES.SIZE[field]
    chk = dev.R1csCheck(field, b)
    for wit in (w, bad):
        host = np.frombuffer(b"".join(int(v).to_bytes(fs, "little") for v in wit), dtype=np.uint64).copy()
        d = zk.DevArray.from_host(host)
        rep = chk.run(host)
        assert chk.run(d) == rep and rep == RC.check(circ, wit)
        d.free()
    chk.free()


# ---- wtns_check and pil_verify agree on a compressor circuit ---------------------------------------------------------------------
def test_agrees_with_pil_verify(zk, dev):
    import pilc
    c12 = importlib.import_module("eigen_zkvm_amd.compressor12")
    b, w, circ = _custom("cmuladd")
    S = c12.Compressor12Setup.from_r1cs(b, 8)
    pil = pilc.compile_pil("c12.pil", S.pil)
    consts = S.consts_host()
    E = c12.Compressor12Exec(S.exec_text, len(w))
    P = zk.PilCheck(pil)
    out_wire = circ["uses"][0][1][11]
    for wit, ok in ((w, True), (CASES.corrupt(w, out_wire), False)):
        rep = both(dev, "GL", b, circ, wit)
        cm = E.run(np.array(wit, dtype=np.uint64), 1 << S.n_bits).to_host()
        pv = P.run(consts, cm)
        assert (rep["findings"] == []) == ok and (pv["findings"] == []) == ok, (rep["findings"], pv["findings"])
    P.free(); E.free(); S.free()
