"""HIP-event times of the witness extension of the PLONK prover's R1CS import (zk_plonk_<curve>_r1cs_extend_dev): the lane
kernel against the wave kernel by segment length, the extension of a circom-shaped circuit against round 1 of a proof of that circuit, and,
for context, the plain-Python extension of tests/plonk_r1cs_ref.py.  What profiles/r24/plonk_r1cs.md records.

    python tools/plonk_r1cs_time.py sweep [--rows-log 12 --rows-log 16] [--length 8 ...] [--reps 7] [--warmup 2] [-c BN128]
    python tools/plonk_r1cs_time.py circuit [--constraints-log 20] [--long-rows-log 12] [--terms 254] [--no-proof] [--reps 7]
    python tools/plonk_r1cs_time.py model [--constraints-log 20] [--long-rows-log 12] [--terms 254]          (no device)

sweep: per length L and row count, a circuit of that many product constraints (sum of L wires) * b = out, so every row leaves one segment
of L terms; the same buffer extended by the lane kernel alone and by the wave kernel alone (ZK_PLONK_R1CS_WAVE_MIN, read when a handle's
table goes to the device), compared word for word, then timed between two events on the null stream.  The witness is any field elements.
circuit: 2^constraints-log constraints (k a + k' a2) * b = out_i (the shape of tests/r1cs_check_cases.products) and 2^long-rows-log rows of
`terms` terms, with a witness that satisfies them; the extension alone as above, with the library's threshold, with the lane kernel alone and
with the wave kernel alone; then, unless --no-proof, proofs of the same circuit with the per-round marks of tools/plonk_time.py.
model: the same circuit through tests/plonk_r1cs_ref.py on the host: seconds of Compiled() and of extend()."""
import argparse, importlib, os, pathlib, statistics, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import numpy as np

import plonk_time

ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
PRIME = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
LANE_ONLY, WAVE_ONLY = str(1 << 40), "2"


def rows_block(rng, n_rows, wires_a, wire_b, wire_c):
    """n_rows constraints A * B = C as the bytes of an .r1cs constraint section: A over the (n_rows, L) wires with random coefficients below
    2^252, B = 1 * wire_b, C = 1 * wire_c -> (bytes, the (n_rows, L, 4) u64 coefficient words)"""
    L = wires_a.shape[1]
    term = np.dtype([("w", "<u4"), ("c", "<u8", 4)])
    row = np.dtype([("na", "<u4"), ("a", term, L), ("nb", "<u4"), ("b", term), ("nc", "<u4"), ("c", term)])
    out = np.zeros(n_rows, row)
    coef = rng.integers(0, 1 << 62, size=(n_rows, L, 4), dtype=np.uint64)
    coef[:, :, 3] >>= np.uint64(2)
    coef[:, :, 0] |= np.uint64(1)
    out["na"], out["nb"], out["nc"] = L, 1, 1
    out["a"]["w"], out["a"]["c"] = wires_a, coef
    out["b"]["w"], out["c"]["w"] = wire_b, wire_c
    out["b"]["c"][:, 0] = 1
    out["c"]["c"][:, 0] = 1
    return out.tobytes(), coef


def r1cs_file(curve, n_wires, n_constraints, body):
    import struct
    head = struct.pack("<I", 32) + PRIME[curve].to_bytes(32, "little") + struct.pack("<IIIIQI", n_wires, 0, 1, n_wires - 2, n_wires, n_constraints)
    return b"r1cs" + struct.pack("<II", 1, 2) + struct.pack("<IQ", 1, len(head)) + head + struct.pack("<IQ", 2, len(body)) + body


def segment_circuit(curve, rng, n_rows, L):
    """n_rows rows of L terms over wires 1 .. L + 1 (a window that moves with the row), b = wire L + 2, an output wire each"""
    base = L + 3
    wires = 1 + (np.arange(n_rows, dtype=np.uint32)[:, None] % 2 + np.arange(L, dtype=np.uint32)[None, :])
    body, _ = rows_block(rng, n_rows, wires, L + 2, base + np.arange(n_rows, dtype=np.uint32))
    return r1cs_file(curve, base + n_rows, n_rows, body)


def extend_ms(zk, plonk, fp, curve, data, mode, reps, warmup, d_w=None):
    """-> (median ms, the extended buffer on the host, info).  mode: None (the library's threshold), LANE_ONLY or WAVE_ONLY"""
    if mode is None:
        os.environ.pop("ZK_PLONK_R1CS_WAVE_MIN", None)
    else:
        os.environ["ZK_PLONK_R1CS_WAVE_MIN"] = mode
    c = plonk.R1csCircuit(data, curve)
    own = d_w is None
    if own:
        d_w = fp.powers(3, 5, c.n_vars, curve, dev=True)
    fn = getattr(zk.lib(), "zk_plonk_%s_r1cs_extend_dev" % ABI[curve])
    ev, ts = plonk_time.Events(), []
    for _ in range(warmup + reps):
        ev.mark("start"); zk._check(fn(c._h, d_w.ptr, None)); ev.mark("run")
        ts.append(ev.take()["run"])
    host = d_w.to_host()
    info = c.info
    if own:
        d_w.free()
    c.free()
    os.environ.pop("ZK_PLONK_R1CS_WAVE_MIN", None)
    return statistics.median(ts[warmup:]), host, info


def sweep(a, zk, plonk, fp):
    rng = np.random.default_rng(7)
    lines = ["| rows | terms | lane kernel alone, ms | wave kernel alone, ms | lane / wave |", "|---|---|---|---|---|"]
    for rows_log in a.rows_log or [12, 16]:
        for L in a.length or [4, 8, 16, 32, 64, 128, 254]:
            data = segment_circuit(a.curve, rng, 1 << rows_log, L)
            lane, h1, info = extend_ms(zk, plonk, fp, a.curve, data, LANE_ONLY, a.reps, a.warmup)
            wave, h2, _ = extend_ms(zk, plonk, fp, a.curve, data, WAVE_ONLY, a.reps, a.warmup)
            assert info["n_segments"] == 1 << rows_log and info["max_segment_terms"] == L
            if not np.array_equal(h1, h2):
                raise SystemExit("plonk_r1cs_time: the two kernels differ at %d rows of %d terms" % (1 << rows_log, L))
            lines.append("| 2^%d | %d | %.3f | %.3f | %.2f |" % (rows_log, L, lane, wave, lane / wave))
            print(lines[-1], flush=True)
    return lines


def circom_shaped(curve, constraints_log, long_rows_log, terms, seed=11):
    """-> (r1cs bytes, the witness as a list of integers): 2^constraints_log product rows of two terms and 2^long_rows_log rows of `terms`"""
    p, rng = PRIME[curve], np.random.default_rng(seed)
    n1, n2 = 1 << constraints_log, (1 << long_rows_log) if long_rows_log >= 0 else 0
    ints = lambda words: [int.from_bytes(w.tobytes(), "little") for w in words.reshape(-1, 4).astype("<u8")]
    w = [1] + [int(x) for x in rng.integers(1, 1 << 62, size=4)]
    i = np.arange(n1, dtype=np.uint32)
    wa = np.stack([1 + i % 4, 1 + (i + 1) % 4], axis=1).astype(np.uint32)
    out1 = 5 + i
    body1, coef1 = rows_block(rng, n1, wa, 1 + (i + 2) % 4, out1)
    c1, wa_l = ints(coef1), wa.tolist()
    for r in range(n1):
        w.append((c1[2 * r] * w[wa_l[r][0]] + c1[2 * r + 1] * w[wa_l[r][1]]) * w[1 + (r + 2) % 4] % p)
    body2 = b""
    if n2:
        j = np.arange(n2, dtype=np.uint32)
        wl = (5 + (j[:, None] * 7 + np.arange(terms, dtype=np.uint32)[None, :]) % n1).astype(np.uint32)      # `terms` consecutive outputs of the first part
        body2, coef2 = rows_block(rng, n2, wl, 1, 5 + n1 + j)
        c2, wl_l = ints(coef2), wl.tolist()
        for r in range(n2):
            w.append(sum(c2[terms * r + t] * w[x] for t, x in enumerate(wl_l[r])) * w[1] % p)
    return r1cs_file(curve, len(w), n1 + n2, body1 + body2), w


def circuit(a, zk, plonk, fp):
    g16, kzg_mod = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    t0 = time.time()
    data, w = circom_shaped(a.curve, a.constraints_log, a.long_rows_log, a.terms)
    ww = plonk.canon_words(w, PRIME[a.curve], "witness value")
    lines = []
    c = plonk.R1csCircuit(data, a.curve)
    info = dict(c.info)
    d_w = plonk.extend_words(c, ww)                                                 # the witness in front, as the prover leaves it
    c.free()
    print("circuit made in %.1f s: %s" % (time.time() - t0, info), flush=True)
    res = {}
    for name, mode in (("library threshold (%d)" % zk.lib().zk_plonk_r1cs_wave_min_terms(), None), ("lane kernel alone", LANE_ONLY), ("wave kernel alone", WAVE_ONLY)):
        res[name], host, _ = extend_ms(zk, plonk, fp, a.curve, data, mode, a.reps, a.warmup, d_w=d_w)
        first = host if name.startswith("library") else first
        if not np.array_equal(first, host):
            raise SystemExit("plonk_r1cs_time: %s gives other words" % name)
    d_w.free()
    lines += ["circuit: %(n_constraints)d constraints -> %(n_gates)d gates, %(n_aux)d auxiliaries in %(n_segments)d segments (%(n_segment_terms)d terms, the longest %(max_segment_terms)d)" % info, "",
              "| extension | ms |", "|---|---|"] + ["| %s | %.3f |" % kv for kv in res.items()]
    print("\n".join(lines), flush=True)
    if a.no_proof:
        return lines
    c = plonk.R1csCircuit(data, a.curve)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "t.ptau")
        t0 = time.time()
        plonk_time.device_ptau(zk, fp, a.curve, c.log_n + 1, plonk_time.TAU, path)
        srs = g16.Srs(a.curve, path)
        kzg = kzg_mod.Kzg(srs, plonk.required_powers(c.n))
        srs.free()
        os.unlink(path)
    t1 = time.time()
    key = plonk.PlonkKey(kzg, c)
    zk._check(zk.lib().zk_dev_sync())
    print("file %.1f s, key %.1f s, n = 2^%d" % (t1 - t0, time.time() - t1, c.log_n), flush=True)
    ev, runs = plonk_time.Events(), []
    for i in range(1 + a.reps):
        proof, publics = plonk.prove(key, ww, self_check=False, _mark=ev.mark)
        times = ev.take()
        assert plonk.verify(key.vk, [publics], [proof]) == (plonk.ACCEPTED, None), "a timed proof is not accepted"
        if i:
            runs.append(times)
    names = ["gate check", "round 1", "round 2", "round 3", "round 5"]
    med = {k: statistics.median(t[k] for t in runs) for k in names}
    lines += ["", "proofs of the same circuit, n = 2^%d (median of %d, every proof verified):" % (c.log_n, a.reps), "", "| " + " | ".join(names) + " |", "|" + "---|" * len(names),
              "| " + " | ".join("%.2f" % med[k] for k in names) + " |"]
    key.free(); kzg.free(); c.free()
    return lines


def model_leg(a):
    sys.path.insert(0, str(ROOT / "tests"))
    import plonk_r1cs_ref as model
    data, w = circom_shaped(a.curve, a.constraints_log, a.long_rows_log, a.terms)
    t0 = time.time()
    m = model.Compiled(data, a.curve)
    t1 = time.time()
    full = m.extend(w)
    t2 = time.time()
    ok = a.constraints_log > 12 or not m.failing_gates(full)
    return ["tests/plonk_r1cs_ref.py on the same circuit (%d gates, %d auxiliaries): Compiled() %.1f s, extend() %.2f s%s" % (m.n_gates, m.n_aux, t1 - t0, t2 - t1, "" if ok else "; GATES FAIL")]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("leg", choices=("sweep", "circuit", "model"))
    ap.add_argument("-c", "--curve", default="BN128", choices=tuple(ABI))
    ap.add_argument("--rows-log", dest="rows_log", type=int, action="append"); ap.add_argument("--length", type=int, action="append")
    ap.add_argument("--constraints-log", dest="constraints_log", type=int, default=20); ap.add_argument("--long-rows-log", dest="long_rows_log", type=int, default=12)
    ap.add_argument("--terms", type=int, default=254); ap.add_argument("--no-proof", dest="no_proof", action="store_true")
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", dest="out", default=None)
    a = ap.parse_args(argv)
    if a.leg == "model":
        lines = model_leg(a)
    else:
        import eigen_zkvm_amd as zk
        zk.init(0)
        plonk, fp = importlib.import_module("eigen_zkvm_amd.plonk"), importlib.import_module("eigen_zkvm_amd.frpoly")
        lines = (sweep if a.leg == "sweep" else circuit)(a, zk, plonk, fp)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
