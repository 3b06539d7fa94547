"""TEST INFRASTRUCTURE ONLY.  A plain-Python witness check over integers that gives the report of zk_r1cs_check_run
(include/zkgpu.h, "wtns_check"), written from the .r1cs layout (algebraic/src/r1cs_file.rs:50-270) and from the constraints
compressor12_pil.rs states for the four custom gates (restated in tests/c12_setup_circuits.py).  Serial, one row and one use at
a time; nothing here touches the GPU or the product."""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tests"))
import c12_setup_circuits as CIRC  # noqa: E402
import c12_setup_ref as REF  # noqa: E402
import groth16 as G  # noqa: E402

PRIMES = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
          "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
          "GL": REF.P}
GATE_KINDS = ("cmuladd", "poseidon12", "fft4", "evpol4")
N_SIGNALS = {"cmuladd": 12, "poseidon12": 372, "fft4": 24, "evpol4": 21}
FIRST_OUTPUT = {"cmuladd": 9, "poseidon12": 12, "fft4": 12, "evpol4": 18}
_POSEIDON = []                                                            # the matrix and the row constants, read once


def circuit(field, r1cs_bytes):
    """-> {"field", "p", "n_wires", "constraints": [(A, B, C)], "gates": [(name, params)], "uses": [(id, signals)]}; every
    side a list of (wire, coefficient) by ascending wire, as both readers of the library keep it"""
    if field == "GL":
        r = REF.read_r1cs(r1cs_bytes)
        return dict(field=field, p=REF.P, n_wires=r["num_variables"], constraints=r["constraints"], gates=r["custom_gates"], uses=r["custom_gates_uses"])
    prime, r = G.read_r1cs(r1cs_bytes)
    assert prime == PRIMES[field]
    return dict(field=field, p=prime, n_wires=r["n_wires"], constraints=r["constraints"], gates=[], uses=[])


def _resolve(gates):
    """template id -> (kind, params), by name as plonk_setup.rs:102-158 does: the last template of a name is the one that counts"""
    ids, fft = {}, {}
    for i, (name, params) in enumerate(gates):
        if name == "FFT4": fft[i] = params
        else: ids[{"CMulAdd": "cmuladd", "Poseidon12": "poseidon12", "EvPol4": "evpol4"}[name]] = i
    out = {i: ("fft4", p) for i, p in fft.items()}
    out.update({i: (k, []) for k, i in ids.items()})
    return out


def _forced(kind, params, v):
    """the outputs the inputs of one use force, in position order"""
    P = REF.P
    if kind == "cmuladd":
        m = CIRC.cmul(v[0:3], v[3:6])
        return [(m[i] + v[6 + i]) % P for i in range(3)]
    if kind == "evpol4":
        res = v[12:15]
        for c in (9, 6, 3, 0):
            m = CIRC.cmul(res, v[15:18]); res = [(m[i] + v[c + i]) % P for i in range(3)]
        return res
    if kind == "fft4":
        return CIRC.fft4_next_row(v[0:12], params)
    if not _POSEIDON:
        _POSEIDON.extend([CIRC._poseidon_matrix(), REF.project_cposeidon()])
    M, C = _POSEIDON
    out = []                                                              # every transition from the witness' own row j:
    for j in range(30):                                                   # row j + 1 = MDS(sbox(row j + C_j)), partial rounds 4..25
        s = [(v[12 * j + i] + C[12 * j + i]) % P for i in range(12)]
        s = [pow(x, 7, P) if (i == 0 or not 4 <= j < 26) else x for i, x in enumerate(s)]
        out += [sum(M[k * 12 + i] * s[k] for k in range(12)) % P for i in range(12)]
    return out


def check(circ, w, max_findings=16):
    p = circ["p"]
    assert len(w) == circ["n_wires"]
    findings = []
    one_bad = w[0] != 1
    if one_bad and max_findings:
        findings.append({"kind": "one_wire", "value": str(w[0])})
    n_bad = 0
    for i, abc in enumerate(circ["constraints"]):
        a, b, c = (sum(cf * w[j] for j, cf in lc) % p for lc in abc)
        if a * b % p == c:
            continue
        n_bad += 1
        if n_bad <= max_findings:
            findings.append({"kind": "constraint", "index": i, "a": str(a), "b": str(b), "c": str(c),
                             "wires": {k: [[j, str(cf)] for j, cf in lc] for k, lc in zip("abc", abc)}})
    checked = {"constraint": len(circ["constraints"])}
    n_failing = {"one_wire": int(one_bad), "constraint": n_bad}
    kinds = _resolve(circ["gates"])
    per_kind = {k: [] for k in GATE_KINDS}
    for u, (gid, sig) in enumerate(circ["uses"]):
        kind, params = kinds[gid]
        per_kind[kind].append((u, params, sig[:N_SIGNALS[kind]]))
    for kind in GATE_KINDS:
        checked[kind] = len(per_kind[kind]); n_failing[kind] = 0
        for u, params, sig in per_kind[kind]:
            v = [w[s] for s in sig]
            forced = _forced(kind, params, v)
            diff = [k for k, e in enumerate(forced) if e != v[FIRST_OUTPUT[kind] + k]]
            if not diff:
                continue
            n_failing[kind] += 1
            if n_failing[kind] > max_findings:
                continue
            k = diff[0]
            f = {"kind": kind, "use": u}
            if kind == "poseidon12": f.update(row=k // 12, column=k % 12)
            else: f["position"] = k
            f.update(wire=sig[FIRST_OUTPUT[kind] + k], expected=str(forced[k]), value=str(v[FIRST_OUTPUT[kind] + k]))
            findings.append(f)
    return {"field": circ["field"], "n_wires": circ["n_wires"], "n_constraints": len(circ["constraints"]), "checked": checked,
            "n_failing": n_failing, "findings": findings}
