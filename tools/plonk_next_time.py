"""HIP-event times of the PLONK prover with a next-row term (eigen_zkvm_amd.plonk_next): the new quotient kernel beside
plonk.py's over the same arrays, a whole proof per round beside plonk.py's on the same gate table, and circom-shaped circuits under the two
import rules.  What profiles/r31/plonk_next.md records.

    python tools/plonk_next_time.py [--section kernel|proof|circuits|counts|all] [--kernel-log-n 16 --kernel-log-n 20] [--log-n 16 --log-n 20]
                                    [--constraints-log 20 --long-rows-log 12 --terms 254] [--rows17-log 14] [--reps 7] [--warmup 2] [-c BN128] [-o out.md]

Timing as tools/plonk_time.py does it: HIP events on the null stream, the median of `reps` after `warmup` (smallest and largest beside it
for the kernels), a powers-of-tau file made on the device with a fixed tau (test material), EVERY proof verified before its times are kept.
  kernel    zk_plonk_<curve>_next_quotient_dev beside zk_plonk_<curve>_quotient_dev at 4n points: the same 15 vectors, q_N a sixteenth; the
            bytes moved are 17 vectors against 16.  With q_N = 0 the two outputs are compared word for word first.
  proof     plonk_time's chain circuit filling n - 1 rows, proved by plonk.py and, with q_N = 0, by plonk_next.py, per round.
  circuits  tools/plonk_r1cs_time.py's circom-shaped circuit (2^constraints-log product rows, 2^long-rows-log rows of `terms` terms) and a
            circuit of 2^rows17-log rows of 17 terms, each compiled under the rule of fan-in 2 (plonk.py) and under the chain rule
            (plonk_next.py): gates, auxiliaries, n, the extension of the witness alone and the proof.
  counts    the circuits' gates, auxiliaries and n under both rules alone: the compile is host work and needs no device."""
import argparse, importlib, os, pathlib, statistics, sys, tempfile, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import numpy as np

import plonk_r1cs_time, plonk_time
from plonk_time import TAU, Events, chain_arrays, device_ptau

ROUNDS = ["gate check", "round 1", "round 2", "round 3", "round 5"]


def _spread(ev, fn, reps, warmup):
    """-> (median, smallest, largest) of `reps` after `warmup`"""
    ts = []
    for _ in range(warmup + reps):
        ev.mark("start"); fn(); ev.mark("run")
        ts.append(ev.take()["run"])
    return statistics.median(ts[warmup:]), min(ts[warmup:]), max(ts[warmup:])


def time_kernels(zk, plonk, pn, fp, curve, log_n, reps, warmup):
    m = 4 << log_n
    alpha, beta, gamma, k1, k2 = 0x1111, 0x2222, 0x3333, 2, 3
    cols = [fp.powers(5 + 2 * j, 7 + j, m, curve, dev=True) for j in range(16)]
    zero = zk.DevArray(4 * m, zero=True)
    out, out2 = zk.DevArray(4 * m), zk.DevArray(4 * m)
    plonk.quotient(cols[:15], log_n, alpha, beta, gamma, k1, k2, curve, out=out)
    pn.quotient(cols[:15] + [zero], log_n, alpha, beta, gamma, k1, k2, curve, out=out2)
    same = np.array_equal(out.to_host(), out2.to_host())
    ev = Events()
    parent = _spread(ev, lambda: plonk.quotient(cols[:15], log_n, alpha, beta, gamma, k1, k2, curve, out=out), reps, warmup)
    new = _spread(ev, lambda: pn.quotient(cols, log_n, alpha, beta, gamma, k1, k2, curve, out=out2), reps, warmup)
    for d in cols + [zero, out, out2]:
        d.free()
    return parent, new, same


def _kzg(zk, fp, curve, log_n, need, tmp):
    g16, kzg_mod = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    path = os.path.join(tmp, "t%d.ptau" % log_n)
    device_ptau(zk, fp, curve, log_n + 1, TAU, path)
    srs = g16.Srs(curve, path)
    kzg = kzg_mod.Kzg(srs, need)
    srs.free()
    os.unlink(path)
    return kzg


def time_proofs(zk, mod, key, witness, reps, warmup):
    """-> {round: median ms, "total": ...}; every proof verified before its times are kept"""
    ev, runs = Events(), []
    for i in range(warmup + reps):
        proof, publics = mod.prove(key, witness, self_check=False, _mark=ev.mark)
        times = ev.take()
        assert mod.verify(key.vk, [publics], [proof]) == (mod.ACCEPTED, None), "a timed proof is not accepted"
        if i >= warmup:
            runs.append(times)
    med = {k: statistics.median(t[k] for t in runs) for k in ROUNDS}
    med["total"] = statistics.median(sum(t[k] for k in ROUNDS) for t in runs)
    return med


def proof_section(zk, plonk, pn, fp, curve, log_n, reps, warmup, tmp):
    n = 1 << log_n
    n_vars, public, gates, ww = chain_arrays(log_n, plonk.FR[curve])
    circuit = plonk.Circuit(n_vars, public, gates, curve)
    kzg = _kzg(zk, fp, curve, log_n, pn.required_powers(n), tmp)
    out = {}
    for name, mod, make in (("plonk.py", plonk, plonk.PlonkKey), ("plonk_next.py, q_N = 0", pn, pn.NextKey)):
        key = make(kzg, circuit)
        out[name] = time_proofs(zk, mod, key, ww, reps, warmup)
        key.free()
    kzg.free()
    return out


def counts(plonk, pn, curve, data):
    out = {}
    for name, cls in (("fan-in 2 (plonk.py)", plonk.R1csCircuit), ("chain (plonk_next.py)", pn.NextR1csCircuit)):
        c = cls(data, curve)
        out[name] = (c.info["n_gates"], c.info["n_aux"], c.log_n, c.info["n_segments"], c.info["max_segment_terms"])
        c.free()
    return out


def circuit_section(zk, plonk, pn, fp, curve, data, w, reps, warmup, tmp):
    """-> {rule: (gates, auxiliaries, log n, extension ms, {round: ms})}; one file, of the larger table's power, serves both rules"""
    ww = plonk.canon_words(w, plonk.FR[curve], "witness value")
    legs = [("fan-in 2 (plonk.py)", plonk, plonk.R1csCircuit(data, curve), plonk.PlonkKey), ("chain (plonk_next.py)", pn, pn.NextR1csCircuit(data, curve), pn.NextKey)]
    top = max(c.log_n for _, _, c, _ in legs)
    kzg = _kzg(zk, fp, curve, top, pn.required_powers(1 << top), tmp)
    fn = getattr(zk.lib(), "zk_plonk_%s_r1cs_extend_dev" % plonk_r1cs_time.ABI[curve])
    out = {}
    for name, mod, c, make in legs:
        ev = Events()
        d = plonk.extend_words(c, ww)
        ext = _spread(ev, lambda: zk._check(fn(c._h, d.ptr, None)), reps, warmup)[0]
        d.free()
        key = make(kzg, c)
        med = time_proofs(zk, mod, key, ww, reps, warmup)
        out[name] = (c.info["n_gates"], c.info["n_aux"], c.log_n, ext, med)
        key.free(); c.free()
        print(name, out[name], flush=True)
    kzg.free()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-c", "--curve", default="BN128", choices=("BN128", "BLS12381"))
    ap.add_argument("--section", default="all", choices=("kernel", "proof", "circuits", "counts", "all"))
    ap.add_argument("--kernel-log-n", dest="kernel_log_n", type=int, action="append"); ap.add_argument("--log-n", dest="log_n", type=int, action="append")
    ap.add_argument("--constraints-log", dest="constraints_log", type=int, default=20); ap.add_argument("--long-rows-log", dest="long_rows_log", type=int, default=12)
    ap.add_argument("--terms", type=int, default=254); ap.add_argument("--rows17-log", dest="rows17_log", type=int, default=14)
    ap.add_argument("--only-circuit", dest="only_circuit", type=int, default=None, help="0: the circom-shaped circuit alone; 1: the rows of 17 terms alone")
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", dest="out", default=None)
    a = ap.parse_args(argv)
    import eigen_zkvm_amd as zk
    plonk, pn, fp = (importlib.import_module("eigen_zkvm_amd." + x) for x in ("plonk", "plonk_next", "frpoly"))
    want = lambda s: a.section in (s, "all")
    lines = ["PLONK with a next-row term on %s: HIP-event ms, median of %d after %d warm-ups; every proof verified" % (a.curve, a.reps, a.warmup), ""]
    shaped = [("2^%d product rows + 2^%d rows of %d terms" % (a.constraints_log, a.long_rows_log, a.terms), (a.constraints_log, a.long_rows_log, a.terms)),
              ("2^%d rows of 17 terms" % a.rows17_log, (5, a.rows17_log, 17))]
    if a.only_circuit is not None:
        shaped = shaped[a.only_circuit:a.only_circuit + 1]
    if a.section == "counts":                                                          # host work alone
        lines += ["| circuit | rule | gates | auxiliaries | n | segments | longest |", "|---|---|---|---|---|---|---|"]
        for title, args in shaped:
            data, _ = plonk_r1cs_time.circom_shaped(a.curve, *args)
            for rule, (g, x, k, s, t) in counts(plonk, pn, a.curve, data).items():
                lines.append("| %s | %s | %d | %d | 2^%d | %d | %d |" % (title, rule, g, x, k, s, t))
                print(lines[-1], flush=True)
    else:
        zk.init(0)
    ok = True
    if want("kernel"):
        lines += ["the quotient kernels at 4n points, median (smallest .. largest):", "", "| 4n | zk_plonk_quotient_dev, ms | GB/s of 16 vectors | zk_plonk_next_quotient_dev, ms | GB/s of 17 vectors | ratio of the medians | q_N = 0 gives the same words |",
                  "|---|---|---|---|---|---|---|"]
        for k in a.kernel_log_n or [16, 20]:
            p, q, same = time_kernels(zk, plonk, pn, fp, a.curve, k, a.reps, a.warmup)
            m = 4 << k
            lines.append("| 2^%d | %.3f (%.3f .. %.3f) | %.0f | %.3f (%.3f .. %.3f) | %.0f | %.3f | %s |" % (k + 2, *p, 16 * m * 32 / p[0] / 1e6, *q, 17 * m * 32 / q[0] / 1e6, q[0] / p[0], "yes" if same else "NO"))
            print(lines[-1], flush=True)
            ok = ok and same
        lines.append("")
    with tempfile.TemporaryDirectory() as tmp:
        if want("proof"):
            lines += ["a proof of the chain circuit in n - 1 rows, per round:", "", "| n | prover | " + " | ".join(ROUNDS) + " | total |", "|---|---|" + "---|" * (len(ROUNDS) + 1)]
            for k in a.log_n or [16, 20]:
                for name, med in proof_section(zk, plonk, pn, fp, a.curve, k, a.reps, a.warmup, tmp).items():
                    lines.append("| 2^%d | %s | " % (k, name) + " | ".join("%.2f" % med[x] for x in ROUNDS + ["total"]) + " |")
                    print(lines[-1], flush=True)
            lines.append("")
        if want("circuits"):
            lines += ["circom-shaped circuits under the two import rules:", "", "| circuit | rule | gates | auxiliaries | n | extension, ms | " + " | ".join(ROUNDS) + " | total |",
                      "|---|---|---|---|---|---|" + "---|" * (len(ROUNDS) + 1)]
            for title, args in shaped:
                t0 = time.time()
                data, w = plonk_r1cs_time.circom_shaped(a.curve, *args)
                print("%s made in %.1f s" % (title, time.time() - t0), flush=True)
                for rule, (g, x, k, ext, med) in circuit_section(zk, plonk, pn, fp, a.curve, data, w, a.reps, a.warmup, tmp).items():
                    lines.append("| %s | %s | %d | %d | 2^%d | %.3f | " % (title, rule, g, x, k, ext) + " | ".join("%.2f" % med[y] for y in ROUNDS + ["total"]) + " |")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
