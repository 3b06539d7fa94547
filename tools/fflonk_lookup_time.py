"""HIP-event times of the fflonk prover with lookups (eigen_zkvm_amd.fflonk_lookup): the four-output kernel beside the two
calls that made the same four vectors before it, a whole proof per round beside fflonk.py's and plonk_lookup.py's on the same circuit, file
and card in the same session, and the use case the argument is for.  What profiles/r28/fflonk_lookup.md records.

    python tools/fflonk_lookup_time.py [--log-n 16 --log-n 20 | --no-provers] [--kernel-log-n 20] [--range-values-log 14 --range-bits 16 | --no-range]
                                       [--section base|tagged|all] [--rounds 3] [--reps 7] [--warmup 2] [-c BN128] [-o out.md]

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
                    against bit decomposition under fflonk.py (2b rows per value), at the n each needs
The tagged section (--section tagged, or all; eigen_zkvm_amd.fflonk_lookup_tagged; what profiles/r30/fflonk_lookup_tagged.md
records), per n = 2^k of --log-n (16 and 20 unless given):
  the kernel alone  zk_fflonk_<curve>_lookup_tagged_quotients_dev beside zk_fflonk_<curve>_lookup_quotients_dev over the same arrays (the
                    tagged launch reads one more, Tg), taking turns within every repetition, at 4n points: 24 + 4 = 28 element-streams
                    against 27.  The whole measurement is made --rounds times (3): the medians' own spread from run to run stands beside them.
  a proof           tools/plonk_lookup_time.py's tagged circuit (n / 8 range lookups and n / 8 XOR lookups into two tables of n / 4 rows
                    each) under fflonk_lookup_tagged.py and under plonk_lookup.py's tagged protocol, beside the single-table circuit of the
                    base section under fflonk_lookup.py; ONE file of power k + 3 for the three
  the use case      2^14 eight-bit range checks and 2^12 four-bit XORs as ONE tagged fflonk proof, against one single-table fflonk proof
                    for each"""
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


def time_tagged_kernel(zk, flt, fl, fp, curve, log_n, reps, warmup, rounds):
    """-> ({form: [(median, min, max) per round]}, bytes of one element-stream, outputs 0 .. 2 of the two kernels equal)"""
    m = 4 << log_n
    sc = [0x2222, 0x3333, 2, 3, 0x4444, 0x5555]
    cols = [fp.powers(5 + 2 * j, 7 + j, m, curve, dev=True) for j in range(22)]
    outs = {"tagged": [zk.DevArray(4 * m) for _ in range(4)], "single table": [zk.DevArray(4 * m) for _ in range(4)]}
    forms = {"tagged": lambda: flt.quotients(cols, log_n, *sc, curve, outs=outs["tagged"]), "single table": lambda: fl.quotients(cols[:21], log_n, *sc, curve, outs=outs["single table"])}
    ev, res = Events(), {k: [] for k in forms}
    for _ in range(rounds):
        ts = {k: [] for k in forms}
        for i in range(warmup + reps):                                                 # the two take turns, so that neither is timed on a colder card
            for name, fn in forms.items():
                ev.mark("start"); fn(); ev.mark("run")
                ts[name].append(ev.take()["run"])
        for k, v in ts.items():
            res[k].append((statistics.median(v[warmup:]), min(v[warmup:]), max(v[warmup:])))
    same = all(np.array_equal(x.to_host(), y.to_host()) for x, y in zip(outs["tagged"][:3], outs["single table"][:3]))
    for d in cols + outs["tagged"] + outs["single table"]:
        d.free()
    return res, m * 32, same


def time_proofs_spread(zk, mod, key, ww, reps, warmup, names):
    """plonk_lookup_time.time_proofs with the smallest and the largest total beside the medians, under the key spread"""
    ev, runs = Events(), []
    for i in range(warmup + reps):
        proof, publics = mod.prove(key, ww, self_check=False, _mark=ev.mark)
        times = ev.take()
        assert mod.verify(key.vk, [publics], [proof]) == (mod.ACCEPTED, None), "a timed proof is not accepted"
        if i >= warmup:
            runs.append(times)
    med = {k: statistics.median(t[k] for t in runs) for k in names}
    totals = [sum(t[k] for k in names) for t in runs]
    med["total"], med["spread"] = statistics.median(totals), (min(totals), max(totals))
    return med


def tagged_section(a, zk, fl, pl, fp, cv, r, files, say):
    """-> whether outputs 0 .. 2 of the two kernels were equal at every size"""
    flt = importlib.import_module("eigen_zkvm_amd.fflonk_lookup_tagged")
    same = True
    for k in a.log_n if a.log_n is not None else [16, 20]:
        n = 1 << k
        res, stream, eq = time_tagged_kernel(zk, flt, fl, fp, cv, k, a.reps, a.warmup, a.rounds)
        same = same and eq
        say("the tagged kernel beside its sibling at 4n = 2^%d, the same arrays, %d rounds of %d after %d: ms, median (smallest .. largest) per round:" % (k + 2, a.rounds, a.reps, a.warmup), "",
            "| kernel | " + " | ".join("round %d" % (i + 1) for i in range(a.rounds)) + " | medians' spread | element-streams | GB/s at the middle median |", "|---|" + "---|" * (a.rounds + 3))
        mid = {}
        for name, streams in (("single table", 27), ("tagged", 28)):
            meds = sorted(t[0] for t in res[name])
            mid[name] = statistics.median(meds)
            say("| %s | " % ("fl_quotients_kernel (21 columns)" if name == "single table" else "flt_quotients_kernel (22 columns)") + " | ".join("%.3f (%.3f .. %.3f)" % t for t in res[name]) +
                " | %.3f .. %.3f | %d | %.0f |" % (meds[0], meds[-1], streams, streams * stream / mid[name] / 1e6))
        say("", "tagged / single table = %.3f (28 / 27 streams = %.3f); outputs 0 .. 2 of the two are %s word for word" % (mid["tagged"] / mid["single table"], 28 / 27, "equal" if eq else "DIFFERENT"), "")
        if a.no_provers:
            continue
        kzg = files.get(fl.file_power(k))
        made = []
        n_vars, public, gates, tables, ww = plt.mixed_circuit_arrays(r, k - 1, n // 8, k - 2, n // 8, (k - 2) // 2, True)
        tagged = fl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables)
        n_vars1, public1, gates1, table1, ww1 = plt.lookup_circuit_arrays(k, r, k - 1, n // 4, n // 2)
        single = fl.LookupCircuit(n_vars1, public1, gates1, table1, cv)
        assert tagged.n == n == single.n and tagged.n_table == n // 2 == single.n_table
        say("n = 2^%d, a proof per round, n / 4 selected rows, n / 2 table rows:" % k, "", "| prover | " + " | ".join(COLUMNS) + " | total (smallest .. largest) |", "|---|" + "---|" * (len(COLUMNS) + 1))
        for name, mod, make, c, w, rounds in (("fflonk lookup tagged, two tables", flt, flt.FflonkLookupTaggedKey, tagged, ww, ROUNDS["fflonk lookup"]),
                                              ("fflonk lookup, single table", fl, fl.FflonkLookupKey, single, ww1, ROUNDS["fflonk lookup"]),
                                              ("plonk lookup tagged, two tables", pl, pl.LookupKey, tagged, ww, ROUNDS["plonk lookup"])):
            key = make(kzg, c)
            med = time_proofs_spread(zk, mod, key, w, a.reps, a.warmup, rounds)
            key.free()
            say(_row(name, med)[:-2] + " (%.2f .. %.2f) |" % med["spread"])
        say("")
    if not a.no_range:
        n_range, n_xor, out = 1 << 14, 1 << 12, []
        for name, args, is_tagged in (("one tagged fflonk proof: 2^14 range checks and 2^12 XORs", (n_range, 8, n_xor, 4), True),
                                      ("single-table fflonk: the 2^14 range checks", (n_range, 8, 0, 4), False), ("single-table fflonk: the 2^12 XORs", (0, 8, n_xor, 4), False)):
            n_vars, public, gates, tables, ww = plt.mixed_circuit_arrays(r, 3, *args, is_tagged)
            circuit = fl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables) if is_tagged else fl.LookupCircuit(n_vars, public, gates, tables, cv)
            mod = flt if is_tagged else fl
            key = (flt.FflonkLookupTaggedKey if is_tagged else fl.FflonkLookupKey)(files.get(fl.file_power(circuit.log_n)), circuit)
            out.append((name, circuit, time_proofs_spread(zk, mod, key, ww, a.reps, a.warmup, ROUNDS["fflonk lookup"])))
            key.free()
        say("2^14 eight-bit range checks and 2^12 four-bit XORs under fflonk:", "", "| form | gates | table rows | n | proof ms (smallest .. largest) |", "|---|---|---|---|---|")
        say(*["| %s | %d | %d | 2^%d | %.2f (%.2f .. %.2f) |" % (name, c.n_gates, c.n_table, c.log_n, med["total"], *med["spread"]) for name, c, med in out])
        two = out[1][2]["total"] + out[2][2]["total"]
        say("| the two single-table proofs together | | | | %.2f |" % two, "", "two unlinked proofs / one tagged proof = %.2f" % (two / out[0][2]["total"]), "")
    return same


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
    ap.add_argument("--section", choices=("all", "base", "tagged"), default="base", help="base: what profiles/r28 records; tagged: the tagged lookups under fflonk beside the single-table ones")
    ap.add_argument("--rounds", type=int, default=3, help="the tagged section's kernel measurement is made this many times")
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
    base = a.section != "tagged"
    if base and a.kernel_log_n:
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
        for k in ([] if a.no_provers or not base else a.log_n if a.log_n is not None else [16, 20]):
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
        if base and not a.no_range:
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
        if a.section != "base":
            same = tagged_section(a, zk, fl, pl, fp, cv, r, files, say) and same
        files.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
