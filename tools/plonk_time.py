"""HIP-event times of the PLONK prover (eigen_zkvm_amd.plonk) per round, and of the fused quotient kernel beside the same
bracket composed from the polynomial layer's public calls.  What profiles/r22/plonk.md records.

    python tools/plonk_time.py [--log-n 16 --log-n 20] [--kernel-log-n 20] [--reps 7] [--warmup 2] [-c BN128] [-o out.md]

Per n = 2^k: the chain circuit x^3 + x + 5 = y filling n - 1 rows, a powers-of-tau file of power k + 1 made on the device with a fixed tau
(test material: the tau is known), the key, then `warmup` + `reps` proofs with fresh blinders; EVERY proof is verified before its times are
kept.  A time is the HIP-event time between the marks prove() sets at its round boundaries on the null stream, so it holds the device work
of the round and the host's gaps between its launches; the median of `reps` is printed.  Round 5's cost of having no linearisation
polynomial -- the 8 openings of fixed polynomials -- is measured as the same Kzg.open_multi with and without them.
For the kernel alone, at 4n = 2^(kernel-log-n + 2) points over 15 distinct input vectors: its time, the bytes it moves (16 vectors of 4n x 32
bytes), and the time of the same bracket from pointwise / terms calls (the vectors k_1 X, k_2 X, Z(wX) and the constant vectors of alpha and
alpha^2 are made outside the timed part, which favours the composed form).  Both results are compared word for word first."""
import argparse, ctypes as C, importlib, os, pathlib, statistics, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import numpy as np

TAU = 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e


class Events:
    """hipEvent timing on the null stream, through the HIP runtime the library itself uses"""

    def __init__(self):
        self.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.marks = []

    def mark(self, name):
        ev = C.c_void_p()
        assert self.hip.hipEventCreate(C.byref(ev)) == 0
        assert self.hip.hipEventRecord(ev, None) == 0
        self.marks.append((name, ev))

    def take(self):
        """-> {name: ms since the mark before it}, and forgets the marks"""
        out = {}
        assert self.hip.hipEventSynchronize(self.marks[-1][1]) == 0
        for (_, e0), (name, e1) in zip(self.marks, self.marks[1:]):
            ms = C.c_float(0)
            assert self.hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            out[name] = out.get(name, 0.0) + ms.value
        for _, ev in self.marks:
            self.hip.hipEventDestroy(ev)
        self.marks = []
        return out


def chain_arrays(log_n, r):
    """plonk_ref.chain's circuit filling n - 1 rows, as arrays: -> (n_vars, public, gates, witness words)"""
    n = 1 << log_n
    steps = (n - 1 - 1 - 2) // 4
    m = 2 + 4 * steps
    words = lambda v: [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]
    table = np.array([words(0), words(1), words(r - 1), words(r - 2), words(r - 5)], dtype=np.uint64)      # 0, 1, -1, -2, -5
    code = {k: np.zeros(m, np.int64) for k in ("qL", "qR", "qO", "qM", "qC")}
    wire = {k: np.zeros(m, np.uint32) for k in "abc"}
    code["qL"][0], code["qC"][0] = 1, 4
    wire["a"][0] = 1
    code["qL"][1], code["qR"][1], code["qO"][1] = 1, 1, 3
    wire["a"][1] = wire["b"][1] = wire["c"][1] = 2
    s = np.arange(steps, dtype=np.int64)
    x, sq, cu, s1, y = 2 + 4 * s, 3 + 4 * s, 4 + 4 * s, 5 + 4 * s, 6 + 4 * s
    for j, (a, b, c, ql, qr, qm) in enumerate(((x, x, sq, 0, 0, 1), (sq, x, cu, 0, 0, 1), (cu, x, s1, 1, 1, 0), (s1, 0 * s + 1, y, 1, 1, 0))):
        rows = 2 + 4 * s + j
        wire["a"][rows], wire["b"][rows], wire["c"][rows] = a, b, c
        code["qL"][rows], code["qR"][rows], code["qM"][rows], code["qO"][rows] = ql, qr, qm, 2
    gates = {k: table[v] for k, v in code.items()}
    gates.update(wire)
    wit = [0, 5, 3]
    xv = 3
    for _ in range(steps):
        a = xv * xv % r; b = a * xv % r; c = (b + xv) % r; xv = (c + 5) % r
        wit += [a, b, c, xv]
    ww = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in wit), dtype="<u8").astype(np.uint64).reshape(-1, 4)
    return len(wit), [len(wit) - 1], gates, ww


def device_ptau(zk, fp, curve, power, tau, path):
    """a powers-of-tau file of `power` with the given tau, alpha = beta = 1: the scalars tau^i on the device (powers), canonical by one
    pointwise product with the plain integer 1, the points by the fixed-base kernel"""
    import make_test_ptau
    abi = make_test_ptau.CURVES[curve]["abi"]
    n8 = make_test_ptau.CURVES[curve]["n8"]
    n = 1 << power
    d = fp.powers(tau, 1, 2 * n - 1, curve, dev=True)
    ones = zk.DevArray.from_host(np.tile(np.array([1, 0, 0, 0], np.uint64), 2 * n - 1))
    fp.pointwise("mul", d, ones, curve, out=d)
    ones.free()
    g1 = zk.mul_generator_fr(d, abi).to_host()[:(2 * n - 1) * n8 // 4].astype("<u8").tobytes()
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    g2 = zk.mul_generator_fr(plonk.View(d, 0, n), abi, group="g2").to_host()[:n * n8 // 2].astype("<u8").tobytes()
    d.free()
    payloads = {2: g1, 3: g2, 4: g1[:2 * n8 * n], 5: g1[:2 * n8 * n], 6: g2[:4 * n8]}
    pathlib.Path(path).write_bytes(make_test_ptau.container(curve, power, payloads))


def time_prover(zk, plonk, fp, curve, log_n, reps, warmup, tmp):
    g16, kzg_mod = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    r, n = plonk.FR[curve], 1 << log_n
    t0 = time.time()
    n_vars, public, gates, ww = chain_arrays(log_n, r)
    circuit = plonk.Circuit(n_vars, public, gates, curve)
    path = os.path.join(tmp, "t%d.ptau" % log_n)
    device_ptau(zk, fp, curve, log_n + 1, TAU, path)
    srs = g16.Srs(curve, path)
    kzg = kzg_mod.Kzg(srs, plonk.required_powers(n))
    srs.free()
    os.unlink(path)
    t1 = time.time()
    key = plonk.PlonkKey(kzg, circuit)
    zk._check(zk.lib().zk_dev_sync())
    t2 = time.time()
    ev, runs = Events(), []
    for i in range(warmup + reps):
        proof, publics = plonk.prove(key, ww, self_check=False, _mark=ev.mark)
        times = ev.take()
        assert plonk.verify(key.vk, [publics], [proof]) == (plonk.ACCEPTED, None), "a timed proof is not accepted"
        if i >= warmup:
            runs.append(times)
    names = ["gate check", "round 1", "round 2", "round 3", "round 5"]
    med = {k: statistics.median(t[k] for t in runs) for k in names}
    med["total"] = statistics.median(sum(t[k] for k in names) for t in runs)
    # round 5 with and without the 8 fixed polynomials: stand-in coefficients of the right lengths, fixed challenges
    src = fp.powers(3, 1, 4 * n, curve, dev=True)
    live = [plonk.View(src, 0, n + 2), plonk.View(src, 8, n + 2), plonk.View(src, 16, n + 2), plonk.View(src, 24, 3 * n + 6), plonk.View(src, 32, n + 3)]
    zeta = 0x1234567
    sets5 = [[zeta]] * 4 + [[zeta, zeta * plonk.omega(curve, log_n) % r]]
    opens = {}
    for name, polys, sets in (("13 polynomials", key.coef + live, [[zeta]] * 8 + sets5), ("5 polynomials", live, sets5)):
        ts = []
        for i in range(warmup + reps):
            ev.mark("start")
            kzg.open_multi(polys, sets, gamma=5, z=7)
            ev.mark("open")
            ts.append(ev.take()["open"])
        opens[name] = statistics.median(ts[warmup:])
    src.free(); key.free(); kzg.free()
    return med, opens, {"circuit and file (host s)": t1 - t0, "key (host s)": t2 - t1}


def time_kernel(zk, plonk, fp, curve, log_n, reps, warmup):
    r, m = plonk.FR[curve], 4 << log_n
    alpha, beta, gamma, k1, k2 = 0x1111, 0x2222, 0x3333, 2, 3
    cols = [fp.powers(5 + 2 * j, 7 + j, m, curve, dev=True) for j in range(15)]
    a, b, c, Z, qL, qR, qO, qM, qC, S1, S2, S3, PI, L1, X = cols
    ev = Events()

    def timed(fn):
        ts = []
        for _ in range(warmup + reps):
            ev.mark("start"); fn(); ev.mark("run")
            ts.append(ev.take()["run"])
        return statistics.median(ts[warmup:])
    out = zk.DevArray(4 * m)
    fused = timed(lambda: plonk.quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve, out=out))
    # the same bracket from the layer's public calls
    k1x, k2x = (fp.pointwise("mul", X, fp.powers(1, k, m, curve, dev=True), curve) for k in (k1, k2))
    Zw = zk.DevArray(4 * m)
    plonk.add_into(curve, Z.ptr + 32 * 4, _zero(zk, Zw, m).ptr, m - 4)
    plonk.add_into(curve, Z.ptr, Zw.ptr + 32 * (m - 4), 4)
    va, va2, ones = fp.powers(1, alpha, m, curve, dev=True), fp.powers(1, alpha * alpha % r, m, curve, dev=True), fp.powers(1, 1, m, curve, dev=True)
    t1, acc = zk.DevArray(4 * m), zk.DevArray(4 * m)
    pw = lambda op, x, y, o: fp.pointwise(op, x, y, curve, out=o)

    def composed():
        pw("mul", a, b, t1); pw("mul", t1, qM, acc)
        for w, q in ((a, qL), (b, qR), (c, qO)):
            pw("mul", w, q, t1); pw("add", acc, t1, acc)
        pw("add", acc, qC, acc); pw("add", acc, PI, acc)
        p1 = fp.terms([a, b, c], [X, k1x, k2x], beta, gamma, curve, dev=True)
        p2 = fp.terms([a, b, c], [S1, S2, S3], beta, gamma, curve, dev=True)
        pw("mul", p1, Z, p1); pw("mul", p2, Zw, p2); pw("sub", p1, p2, p1); pw("mul", p1, va, p1); pw("add", acc, p1, acc)
        pw("sub", Z, ones, t1); pw("mul", t1, L1, t1); pw("mul", t1, va2, t1); pw("add", acc, t1, acc)
        p1.free(); p2.free()
    comp = timed(composed)
    same = np.array_equal(out.to_host(), acc.to_host())
    for d in cols + [out, k1x, k2x, Zw, va, va2, ones, t1, acc]:
        d.free()
    return fused, comp, 16 * m * 32, same


def _zero(zk, d, m):
    zk._check(zk.lib().zk_dev_memset(d.ptr, 0, 32 * m))
    return d


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-c", "--curve", default="BN128", choices=("BN128", "BLS12381"))
    ap.add_argument("--log-n", dest="log_n", type=int, action="append")
    ap.add_argument("--kernel-log-n", dest="kernel_log_n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", dest="out", default=None)
    a = ap.parse_args(argv)
    import eigen_zkvm_amd as zk
    zk.init(0)
    plonk, fp = importlib.import_module("eigen_zkvm_amd.plonk"), importlib.import_module("eigen_zkvm_amd.frpoly")
    lines = ["PLONK prover on %s: HIP-event ms, median of %d after %d warm-ups; every proof verified" % (a.curve, a.reps, a.warmup), ""]
    names = ["gate check", "round 1", "round 2", "round 3", "round 5", "total"]
    lines += ["| n | " + " | ".join(names) + " | open_multi, 13 polynomials | open_multi, 5 polynomials | share of the 8 fixed openings |", "|---|" + "---|" * (len(names) + 3)]
    with tempfile.TemporaryDirectory() as tmp:
        for k in a.log_n or [16, 20]:
            med, opens, host = time_prover(zk, plonk, fp, a.curve, k, a.reps, a.warmup, tmp)
            o13, o5 = opens["13 polynomials"], opens["5 polynomials"]
            lines.append("| 2^%d | " % k + " | ".join("%.2f" % med[x] for x in names) + " | %.2f | %.2f | %.0f %% |" % (o13, o5, 100 * (o13 - o5) / o13))
            print(lines[-1], host, flush=True)
    fused, comp, nbytes, same = time_kernel(zk, plonk, fp, a.curve, a.kernel_log_n, a.reps, a.warmup)
    lines += ["", "zk_plonk_<curve>_quotient_dev alone at 4n = 2^%d:" % (a.kernel_log_n + 2), "",
              "| form | ms | bytes moved | GB/s |", "|---|---|---|---|",
              "| fused kernel | %.3f | %d | %.0f |" % (fused, nbytes, nbytes / fused / 1e6),
              "| composed from pointwise / terms | %.3f | | |" % comp, "",
              "the two results are %s word for word" % ("equal" if same else "DIFFERENT")]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
