"""HIP-event times of the fflonk prover (eigen_zkvm_amd.fflonk) per round beside the PLONK prover's on the same circuit, file
and card in the same session; verification of 1 and 16 proofs of both; and the three-output kernel beside the same three vectors composed
from the PLONK kernel.  What profiles/r25/fflonk.md records.

    python tools/fflonk_time.py [--log-n 16 --log-n 20 | --no-provers] [--kernel-log-n 20] [--reps 7] [--warmup 2] [-c BN128] [-o out.md]

Per n = 2^k: tools/plonk_time.py's chain circuit filling n - 1 rows, ONE powers-of-tau file of power k + 3 made on the device with a fixed tau
(test material: the tau is known; 9n + 18 powers for fflonk, of which PLONK uses 3n + 6), both keys, then `warmup` + `reps` proofs of each
prover with fresh blinders; EVERY proof is verified before its times are kept.  A time is the HIP-event time between the marks prove() sets at
its round boundaries on the null stream, so it holds the device work of the round and the host's gaps between its launches; the median of
`reps` is printed.  Verification is host work and two pairings, so it is wall-clock ms around verify(), the same median.
For the kernel alone, at 4n = 2^(kernel-log-n + 2) points over 15 distinct input vectors: the time of one launch with its three outputs, the
bytes it moves (15 vectors in, 3 out, 4n x 32 bytes each), the two launches the prover makes (out0 alone; out1 and out2), and the same three
vectors from the parent's code: three calls of zk_plonk_<curve>_quotient_dev with alpha = 0, 1 and r - 1 -- Q(0) = G, Q(1) = G + D + L,
Q(-1) = G - D + L -- and the pointwise combinations that separate them, D = (Q(1) - Q(-1)) / 2, L = (Q(1) + Q(-1)) / 2 - G (the constant
vector of 1 / 2 is made outside the timed part, which favours the composed form).  The forms take turns within every repetition.  Both
results are compared word for word."""
import argparse, importlib, os, pathlib, statistics, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import numpy as np

import plonk_time
from plonk_time import TAU, Events

ROUNDS = {"plonk": ["gate check", "round 1", "round 2", "round 3", "round 5"], "fflonk": ["gate check", "round 1", "round 2", "round 4"]}


def _wall(fn, reps, warmup):
    ts = []
    for _ in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts[warmup:])


def time_provers(zk, plonk, fflonk, fp, curve, log_n, reps, warmup, tmp):
    """-> {prover: ({round: ms, "total": ms}, {1: ms, 16: ms} of verify, key seconds)}"""
    g16, kzg_mod = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    r, n = plonk.FR[curve], 1 << log_n
    n_vars, public, gates, ww = plonk_time.chain_arrays(log_n, r)
    circuit = plonk.Circuit(n_vars, public, gates, curve)
    path = os.path.join(tmp, "t%d.ptau" % log_n)
    plonk_time.device_ptau(zk, fp, curve, fflonk.file_power(log_n), TAU, path)
    srs = g16.Srs(curve, path)
    kzg = kzg_mod.Kzg(srs, fflonk.required_powers(n))
    srs.free()
    os.unlink(path)
    out = {}
    for name, mod, make in (("plonk", plonk, plonk.PlonkKey), ("fflonk", fflonk, fflonk.FflonkKey)):
        t0 = time.time()
        key = make(kzg, circuit)
        zk._check(zk.lib().zk_dev_sync())
        t_key = time.time() - t0
        ev, runs, last = Events(), [], None
        for i in range(warmup + reps):
            proof, publics = mod.prove(key, ww, self_check=False, _mark=ev.mark)
            times = ev.take()
            assert mod.verify(key.vk, [publics], [proof]) == (mod.ACCEPTED, None), "a timed proof is not accepted"
            last = (proof, publics)
            if i >= warmup:
                runs.append(times)
        med = {k: statistics.median(t[k] for t in runs) for k in ROUNDS[name]}
        med["total"] = statistics.median(sum(t[k] for k in ROUNDS[name]) for t in runs)
        ver = {}
        for m in (1, 16):
            def check(m=m):
                assert mod.verify(key.vk, [last[1]] * m, [last[0]] * m) == (mod.ACCEPTED, None), "a timed batch is not accepted"
            ver[m] = _wall(check, reps, warmup)
        out[name] = (med, ver, t_key)
        key.free()
    kzg.free()
    return out


def time_kernel(zk, plonk, fflonk, fp, curve, log_n, reps, warmup):
    r, m = plonk.FR[curve], 4 << log_n
    beta, gamma, k1, k2 = 0x2222, 0x3333, 2, 3
    cols = [fp.powers(5 + 2 * j, 7 + j, m, curve, dev=True) for j in range(15)]
    outs = [zk.DevArray(4 * m) for _ in range(3)]
    parent, q0, q1, qm, t = (zk.DevArray(4 * m) for _ in range(5))
    half = fp.powers(1, pow(2, -1, r), m, curve, dev=True)
    pw = lambda op, x, y, o: fp.pointwise(op, x, y, curve, out=o)

    def composed():                                                                    # the same three vectors from the parent's kernel and the layer's public calls
        for alpha, q in ((0, q0), (1, q1), (r - 1, qm)):
            plonk.quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve, out=q)
        pw("add", q1, qm, t); pw("sub", q1, qm, qm); pw("mul", qm, half, qm)          # qm = D
        pw("mul", t, half, t); pw("sub", t, q0, t)                                     # t = L, q0 = G
    forms = {"fused": lambda: fflonk.quotients(cols, log_n, beta, gamma, k1, k2, curve, outs=outs),
             "first": lambda: fflonk.quotients(cols, log_n, 0, 0, k1, k2, curve, outs=[outs[0], None, None], want=(True, False, False)),
             "second": lambda: fflonk.quotients(cols, log_n, beta, gamma, k1, k2, curve, outs=[None, outs[1], outs[2]], want=(False, True, True)),
             "parent": lambda: plonk.quotient(cols, log_n, 0x1111, beta, gamma, k1, k2, curve, out=parent),
             "composed": composed}
    ev, ts = Events(), {k: [] for k in forms}
    for i in range(warmup + reps):                                                     # the forms take turns, so that none is timed on a colder card than another
        for name, fn in forms.items():
            ev.mark("start"); fn(); ev.mark("run")
            ts[name].append(ev.take()["run"])
    ms = {k: statistics.median(v[warmup:]) for k, v in ts.items()}
    same = all(np.array_equal(x.to_host(), y.to_host()) for x, y in zip(outs, (q0, t, qm)))
    for d in cols + outs + [parent, q0, q1, qm, t, half]:
        d.free()
    return ms, 18 * m * 32, same


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-c", "--curve", default="BN128", choices=("BN128", "BLS12381"))
    ap.add_argument("--log-n", dest="log_n", type=int, action="append")
    ap.add_argument("--kernel-log-n", dest="kernel_log_n", type=int, default=20, help="0: skip the kernel's part")
    ap.add_argument("--no-provers", dest="no_provers", action="store_true", help="the kernel's part alone")
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", dest="out", default=None)
    a = ap.parse_args(argv)
    import eigen_zkvm_amd as zk
    zk.init(0)
    plonk, fflonk, fp = (importlib.import_module("eigen_zkvm_amd." + m) for m in ("plonk", "fflonk", "frpoly"))
    lines = ["fflonk and PLONK provers on %s: HIP-event ms per round, median of %d after %d warm-ups; every proof verified.  verify: wall-clock ms" % (a.curve, a.reps, a.warmup), ""]
    lines += ["| n | prover | gate check | round 1 | round 2 | round 3 | last round (opening) | total | verify 1 | verify 16 | key (s) |", "|---|" + "---|" * 10]
    with tempfile.TemporaryDirectory() as tmp:
        for k in ([] if a.no_provers else a.log_n if a.log_n is not None else [16, 20]):
            res = time_provers(zk, plonk, fflonk, fp, a.curve, k, a.reps, a.warmup, tmp)
            for name in ("plonk", "fflonk"):
                med, ver, t_key = res[name]
                cells = [med["gate check"], med["round 1"], med["round 2"], med.get("round 3"), med.get("round 5", med.get("round 4")), med["total"], ver[1], ver[16]]
                lines.append("| 2^%d | %s | " % (k, name) + " | ".join("-" if c is None else "%.2f" % c for c in cells) + " | %.2f |" % t_key)
                print(lines[-1], flush=True)
            lines.append("| 2^%d | fflonk / plonk | | | | | | %.2f | %.2f | %.2f | |" % (k, res["fflonk"][0]["total"] / res["plonk"][0]["total"], res["fflonk"][1][1] / res["plonk"][1][1],
                                                                                     res["fflonk"][1][16] / res["plonk"][1][16]))
            print(lines[-1], flush=True)
    same = True
    if a.kernel_log_n:
        ms, nbytes, same = time_kernel(zk, plonk, fflonk, fp, a.curve, a.kernel_log_n, a.reps, a.warmup)
        lines += ["", "zk_fflonk_<curve>_quotients_dev alone at 4n = 2^%d:" % (a.kernel_log_n + 2), "",
                  "| form | ms | bytes moved | GB/s |", "|---|---|---|---|",
                  "| one launch, three outputs | %.3f | %d | %.0f |" % (ms["fused"], nbytes, nbytes / ms["fused"] / 1e6),
                  "| round 1's launch: out0 alone | %.3f | %d | %.0f |" % (ms["first"], 10 * nbytes // 18, 10 * nbytes // 18 / ms["first"] / 1e6),
                  "| round 2's launch: out1 and out2 | %.3f | %d | %.0f |" % (ms["second"], 11 * nbytes // 18, 11 * nbytes // 18 / ms["second"] / 1e6),
                  "| zk_plonk_<curve>_quotient_dev, one call (one folded output) | %.3f | %d | %.0f |" % (ms["parent"], 16 * nbytes // 18, 16 * nbytes // 18 / ms["parent"] / 1e6),
                  "| composed: three such calls (alpha = 0, 1, r - 1) and five pointwise calls | %.3f | | |" % ms["composed"], "",
                  "(bytes: distinct vectors of 4n x 32 bytes read or written -- 15 + 3; out0 alone reads a, b, c, the five selectors and PI: 9 + 1; out1 and out2 read a, b, c, Z, "
                  "the three S_sigma, L_1, X: 9 + 2; the parent's call 15 + 1)", "", "the two results are %s word for word" % ("equal" if same else "DIFFERENT")]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
