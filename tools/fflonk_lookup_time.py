"""HIP-event times of the fflonk prover with lookups (eigen_zkvm_amd.fflonk_lookup): the four-output kernel beside the two
calls that made the same four vectors before it, a whole proof per round beside fflonk.py's and plonk_lookup.py's on the same circuit, file
and card in the same session, and the use case the argument is for.  What profiles/r28/fflonk_lookup.md records.

    python tools/fflonk_lookup_time.py [--log-n 16 --log-n 20 | --no-provers] [--kernel-log-n 20] [--range-values-log 14 --range-bits 16 | --no-range]
                                       [--reps 7] [--warmup 2] [-c BN128] [-o out.md]

Timing as tools/fflonk_time.py and tools/plonk_lookup_time.py do it: HIP events on the null stream, the median of `reps` after `warmup`, a
powers-of-tau file made on the device with a fixed tau (test material), EVERY proof verified before its times are kept.
  the kernel alone  at 4n = 2^(kernel-log-n + 2) points over 21 distinct input vectors: one launch of zk_fflonk_<curve>_lookup_quotients_dev
                    with its four outputs, against zk_fflonk_<curve>_quotients_dev, a zero-fill of the fourth vector and
                    zk_plonk_<curve>_lookup_quotient_dev with alpha = 1 on it.  The forms take turns within every repetition; both results are
                    compared word for word.  Bytes are counted as element-streams of 4n x 32 bytes, loads and stores: 23 + 4 = 27 for the one
                    launch (Z and Phi are read twice), 16 + 3, 1 and 10 + 1 + 1 = 32 for the three calls.
  a proof           per n = 2^k: tools/plonk_lookup_time.py's circuit (plonk_time's chain in n / 2 rows and n / 4 lookups into a range table
                    of n / 2 rows) under this prover and under plonk_lookup.py, and the same gates without their lookups under fflonk.py; ONE
                    file of power k + 3 for the three
  the use case      2^v values each proved below 2^b: one lookup row per value into range_table(b) under this prover (n forced by the table),
                    against bit decomposition under fflonk.py (2b rows per value), at the n each needs"""
import argparse, importlib, os, pathlib, statistics, sys, tempfile
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import numpy as np

import plonk_lookup_time as plt
import plonk_time
from plonk_time import TAU, Events

ROUNDS = {"fflonk lookup": ["gate check", "lookup check", "round 1", "round 2", "round 4"], "fflonk": ["gate check", "round 1", "round 2", "round 4"],
          "plonk lookup": ["gate check", "lookup check", "round 1", "round 2", "round 3", "round 5"]}
COLUMNS = ["gate check", "lookup check", "round 1", "round 2", "round 3", "opening"]
LOOKUP_COLS = [0, 1, 2, 15, 16, 17, 18, 19, 20]            # a, b, c, q_K, t1, t2, t3, M, Phi among the 21 columns


class Files:
    """one Kzg handle per file power, made on first use (the largest file is asked for twice) and kept until close()"""

    def __init__(self, zk, fp, curve, tmp):
        self.zk, self.fp, self.curve, self.tmp, self.made = zk, fp, curve, tmp, {}

    def get(self, power):
        if power not in self.made:
            g16, kzg_mod = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
            path = os.path.join(self.tmp, "t%d.ptau" % power)
            plonk_time.device_ptau(self.zk, self.fp, self.curve, power, TAU, path)
            srs = g16.Srs(self.curve, path)
            self.made[power] = kzg_mod.Kzg(srs)
            srs.free()
            os.unlink(path)
        return self.made[power]

    def close(self):
        for h in self.made.values():
            h.free()
        self.made = {}


def time_kernel(zk, fl, fflonk, pl, fp, curve, log_n, reps, warmup):
    """-> ({form: ms}, bytes of one element-stream, the two results equal)"""
    m = 4 << log_n
    sc = [0x2222, 0x3333, 2, 3, 0x4444, 0x5555]
    cols = [fp.powers(5 + 2 * j, 7 + j, m, curve, dev=True) for j in range(21)]
    fused, apart = [zk.DevArray(4 * m) for _ in range(4)], [zk.DevArray(4 * m) for _ in range(4)]
    look = [cols[j] for j in LOOKUP_COLS]

    def zero():
        zk._check(zk.lib().zk_dev_memset(apart[3].ptr, 0, 32 * m))
    steps = {"three": lambda: fflonk.quotients(cols[:15], log_n, *sc[:4], curve, outs=apart[:3]), "zero-fill": zero,
             "lookup": lambda: pl.lookup_quotient(look, log_n, 1, sc[4], sc[5], apart[3], curve)}

    def two_calls():
        for fn in steps.values():
            fn()
    forms = {"fused": lambda: fl.quotients(cols, log_n, *sc, curve, outs=fused), "two calls": two_calls}
    ev, ts = Events(), {k: [] for k in list(forms) + list(steps)}
    for i in range(warmup + reps):                                                     # the forms take turns, so that none is timed on a colder card than another
        for name, fn in list(forms.items()) + list(steps.items()):                     # the steps once more each on their own, in their order: the accumulator is zero again
            ev.mark("start"); fn(); ev.mark("run")
            ts[name].append(ev.take()["run"])
    ms = {k: statistics.median(v[warmup:]) for k, v in ts.items()}
    ms["spread"] = {k: (min(ts[k][warmup:]), max(ts[k][warmup:])) for k in forms}
    same = all(np.array_equal(x.to_host(), y.to_host()) for x, y in zip(fused, apart))
    for d in cols + fused + apart:
        d.free()
    return ms, m * 32, same


def time_proofs(zk, mod, key, ww, reps, warmup, names):
    return plt.time_proofs(zk, mod, key, ww, reps, warmup, names)


def _row(name, med):
    cells = [med.get("gate check"), med.get("lookup check"), med.get("round 1"), med.get("round 2"), med.get("round 3"), med.get("round 5", med.get("round 4")), med["total"]]
    return "| %s | " % name + " | ".join("-" if c is None else "%.2f" % c for c in cells) + " |"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-c", "--curve", default="BN128", choices=("BN128", "BLS12381"))
    ap.add_argument("--log-n", dest="log_n", type=int, action="append")
    ap.add_argument("--kernel-log-n", dest="kernel_log_n", type=int, default=20, help="0: skip the kernel's part")
    ap.add_argument("--no-provers", dest="no_provers", action="store_true", help="skip the proofs per round")
    ap.add_argument("--range-values-log", dest="values_log", type=int, default=14); ap.add_argument("--range-bits", dest="bits", type=int, default=16)
    ap.add_argument("--no-range", dest="no_range", action="store_true", help="skip the use case")
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", dest="out", default=None)
    a = ap.parse_args(argv)
    import eigen_zkvm_amd as zk
    zk.init(0)
    fl, fflonk, pl, fp = (importlib.import_module("eigen_zkvm_amd." + m) for m in ("fflonk_lookup", "fflonk", "plonk_lookup", "frpoly"))
    cv, r = a.curve, fl.FR[a.curve]
    lines = ["fflonk with lookups on %s: HIP-event ms, median of %d after %d warm-ups; every proof verified" % (cv, a.reps, a.warmup), ""]

    def say(*ls):
        lines.extend(ls)
        print("\n".join(ls), flush=True)
    same = True
    if a.kernel_log_n:
        ms, stream, same = time_kernel(zk, fl, fflonk, pl, fp, cv, a.kernel_log_n, a.reps, a.warmup)
        rate = lambda streams, t: "%.0f" % (streams * stream / t / 1e6)
        say("zk_fflonk_<curve>_lookup_quotients_dev alone at 4n = 2^%d:" % (a.kernel_log_n + 2), "", "| form | ms (min .. max) | element-streams | bytes | GB/s |", "|---|---|---|---|---|",
            "| one launch, four outputs | %.3f (%.3f .. %.3f) | 27 | %d | %s |" % (ms["fused"], *ms["spread"]["fused"], 27 * stream, rate(27, ms["fused"])),
            "| two calls and a zero-fill, timed together | %.3f (%.3f .. %.3f) | 32 | %d | %s |" % (ms["two calls"], *ms["spread"]["two calls"], 32 * stream, rate(32, ms["two calls"])),
            "| - zk_fflonk_<curve>_quotients_dev | %.3f | 19 | %d | %s |" % (ms["three"], 19 * stream, rate(19, ms["three"])),
            "| - the zero-fill | %.3f | 1 | %d | %s |" % (ms["zero-fill"], stream, rate(1, ms["zero-fill"])),
            "| - zk_plonk_<curve>_lookup_quotient_dev, alpha = 1 | %.3f | 12 | %d | %s |" % (ms["lookup"], 12 * stream, rate(12, ms["lookup"])), "",
            "one launch / two calls = %.3f; the two results are %s word for word" % (ms["fused"] / ms["two calls"], "equal" if same else "DIFFERENT"), "")
    with tempfile.TemporaryDirectory() as tmp:
        files = Files(zk, fp, cv, tmp)
        for k in ([] if a.no_provers else a.log_n if a.log_n is not None else [16, 20]):
            n = 1 << k
            kzg = files.get(fl.file_power(k))
            n_vars, public, gates, table, ww = plt.lookup_circuit_arrays(k, r, k - 1, n // 4, n // 2)
            circuit = fl.LookupCircuit(n_vars, public, gates, table, cv)
            plain = fflonk.Circuit(n_vars, public, {g: v for g, v in gates.items() if g != "qK"}, cv)
            assert circuit.n == n == plain.n
            say("n = 2^%d, a proof per round (the same gates; fflonk.py without their lookups):" % k, "", "| prover | " + " | ".join(COLUMNS) + " | total |", "|---|" + "---|" * (len(COLUMNS) + 1))
            for name, mod, make, c in (("fflonk lookup", fl, fl.FflonkLookupKey, circuit), ("fflonk", fflonk, fflonk.FflonkKey, plain), ("plonk lookup", pl, pl.LookupKey, circuit)):
                key = make(kzg, c)
                say(_row(name, time_proofs(zk, mod, key, ww, a.reps, a.warmup, ROUNDS[name])))
                key.free()
            say("")
        if not a.no_range:
            nv, bits = 1 << a.values_log, a.bits
            n_vars, public, gates, table, ww = plt.lookup_circuit_arrays(bits, r, 3, nv, 1 << bits)
            circuit = fl.LookupCircuit(n_vars, public, gates, table, cv)
            kzg = files.get(fl.file_power(circuit.log_n))
            key = fl.FflonkLookupKey(kzg, circuit)
            lk = time_proofs(zk, fl, key, ww, a.reps, a.warmup, ROUNDS["fflonk lookup"])
            key.free()
            n_vars, public, gates, ww = plt.bits_circuit_arrays(nv, bits, r)
            plain = fflonk.Circuit(n_vars, public, gates, cv)
            kzg = files.get(fflonk.file_power(plain.log_n))
            key = fflonk.FflonkKey(kzg, plain)
            pk = time_proofs(zk, fflonk, key, ww, a.reps, a.warmup, ROUNDS["fflonk"])
            key.free()
            say("2^%d values each proved below 2^%d:" % (a.values_log, bits), "", "| form | gates | n | file power | proof ms |", "|---|---|---|---|---|",
                "| one lookup row per value, this prover | %d | 2^%d | %d | %.2f |" % (circuit.n_gates, circuit.log_n, fl.file_power(circuit.log_n), lk["total"]),
                "| bit decomposition, fflonk.py | %d | 2^%d | %d | %.2f |" % (plain.n_gates, plain.log_n, fflonk.file_power(plain.log_n), pk["total"]), "")
        files.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
