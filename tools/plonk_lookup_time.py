"""HIP-event times of the PLONK prover with lookups (eigen_zkvm_amd.plonk_lookup): the new device steps alone, a whole
proof per round beside the plain PLONK prover's on the same box, the running sum beside the running product, and the use case the
argument is for.  What profiles/r27/plonk_lookup.md records.

    python tools/plonk_lookup_time.py [--log-n 16 --log-n 20] [--range-values-log 14 --range-bits 16] [--reps 7] [--warmup 2] [-c BN128] [-o out.md]

Timing as tools/plonk_time.py does it: HIP events on the null stream, the median of `reps` after `warmup`, a powers-of-tau file made on the
device with a fixed tau (test material), EVERY proof verified before its times are kept.  Per n = 2^k:
  the steps alone   the table's build (n rows); the count with every row selected, the lookups spread evenly over the n table rows and all
                    on one row; terms + batch_inverse + summands + prefix_sum; the added quotient launch on 4n points
  a proof           plonk_time's chain circuit in n / 2 rows and n / 4 lookups into a range table of n / 2 rows, per round, next to
                    tools/plonk_time.py's figures for the plain prover at the same n in the same process
  the scans         prefix_sum against prefix_product over the same n elements
The use case: 2^v values each proved below 2^b, once with one lookup row per value into range_table(b) (n forced by the table), once by bit
decomposition through the plain prover (per value b boolean gates and b gates that add the bits up: 2b rows), at the n each needs."""
import argparse, importlib, os, pathlib, statistics, sys, tempfile
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import numpy as np

import plonk_time
from plonk_time import TAU, Events, chain_arrays, device_ptau


def _words(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def _small(a):
    """non-negative integers below 2^63 as (len, 4) u64 canonical words"""
    out = np.zeros((len(a), 4), np.uint64)
    out[:, 0] = a
    return out


def _kzg(zk, fp, curve, log_n, need, tmp):
    g16, kzg_mod = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    path = os.path.join(tmp, "t%d.ptau" % log_n)
    device_ptau(zk, fp, curve, log_n + 1, TAU, path)
    srs = g16.Srs(curve, path)
    kzg = kzg_mod.Kzg(srs, need)
    srs.free()
    os.unlink(path)
    return kzg


def _timed(ev, fn, reps, warmup):
    ts = []
    for _ in range(warmup + reps):
        ev.mark("start"); fn(); ev.mark("run")
        ts.append(ev.take()["run"])
    return statistics.median(ts[warmup:])


def time_steps(zk, pl, fp, curve, log_n, reps, warmup):
    """the new device steps alone at n = 2^log_n -> {name: ms}"""
    n, ev, out = 1 << log_n, Events(), {}
    mont = importlib.import_module("eigen_zkvm_amd.plonk_arith").mont_dev
    idx = np.arange(n, dtype=np.uint64)
    t1, zero, one = mont(curve, _small(idx)), mont(curve, _small(0 * idx)), mont(curve, _small(0 * idx + 1))
    spread = mont(curve, _small((idx * np.uint64(0x9E3779B1)) % np.uint64(n)))             # a permutation of the table's rows
    hot = mont(curve, _small(0 * idx + 12345 % n))
    made = []

    def build():
        made.append(pl.LookupTable(t1, zero, zero, n, curve))
    out["table build"] = _timed(ev, build, reps, warmup)
    tab = made[-1]
    m = zk.DevArray(4 * n)
    for name, a in (("count, spread", spread), ("count, one row", hot)):
        out[name] = _timed(ev, lambda: pl.count(tab, a, zero, zero, one, n, out=m), reps, warmup)
        _, bad, _ = pl.count(tab, a, zero, zero, one, n, out=m)
        assert bad == 0
    pl.count(tab, spread, zero, zero, one, n, out=m)                                       # every table row once: the sum below closes

    def sum_steps():
        d = pl.terms([spread, zero, zero, t1, zero, zero], n, 0x1111, 0x2222, curve)
        fp.batch_inverse(d, curve, out=d)
        s = pl.summands(d, one, m, n, curve)
        _, last = fp.prefix_sum(s, curve, out=s)
        assert last == 0
        d.free(); s.free()
    out["terms + inverse + summands + prefix_sum"] = _timed(ev, sum_steps, reps, warmup)
    cols = [fp.powers(5 + 2 * j, 7 + j, 4 * n, curve, dev=True) for j in range(10)]
    out["lookup_quotient (4n points)"] = _timed(ev, lambda: pl.lookup_quotient(cols[:9], log_n, 0x1111, 0x2222, 0x3333, cols[9], curve), reps, warmup)
    out["bytes of lookup_quotient"] = 11 * 4 * n * 32
    v = cols[0]
    out["prefix_sum"] = _timed(ev, lambda: fp.prefix_sum(plonk_view(v, n), curve, out=cols[1]), reps, warmup)
    out["prefix_product"] = _timed(ev, lambda: fp.prefix_product(plonk_view(v, n), curve, out=cols[1]), reps, warmup)
    for t in made:
        t.free()
    for d in cols + [t1, zero, one, spread, hot, m]:
        d.free()
    return out


def plonk_view(d, n):
    return importlib.import_module("eigen_zkvm_amd.plonk_arith").View(d, 0, n)


def lookup_circuit_arrays(log_n, r, chain_log, n_lookups, table_rows):
    """plonk_time's chain in 2^chain_log rows, then n_lookups range lookups (a = a fresh variable, b = c = variable 0) into the table
    (v, 0, 0), v < table_rows -> (n_vars, public, gates with qK, table words, witness words)"""
    n_vars, public, gates, ww = chain_arrays(chain_log, r)
    m = len(gates["a"])
    zeros = np.zeros((n_lookups, 4), np.uint64)
    for k in ("qL", "qR", "qO", "qM", "qC"):
        gates[k] = np.concatenate([gates[k], zeros])
    gates["a"] = np.concatenate([gates["a"], np.arange(n_vars, n_vars + n_lookups, dtype=np.uint32)])
    gates["b"] = np.concatenate([gates["b"], np.zeros(n_lookups, np.uint32)])
    gates["c"] = np.concatenate([gates["c"], np.zeros(n_lookups, np.uint32)])
    gates["qK"] = np.concatenate([np.zeros((m, 4), np.uint64), _small(np.ones(n_lookups, np.uint64))])
    vals = (np.arange(n_lookups, dtype=np.uint64) * np.uint64(0x9E3779B1)) % np.uint64(table_rows)
    table = np.zeros((table_rows, 3, 4), np.uint64)
    table[:, 0, 0] = np.arange(table_rows, dtype=np.uint64)
    return n_vars + n_lookups, public, gates, table, np.concatenate([ww, _small(vals)])


def bits_circuit_arrays(n_values, bits, r):
    """n_values values below 2^bits by bit decomposition: per value `bits` boolean gates b b - b = 0 and `bits` gates
    acc_(j+1) = acc_j + 2^j b_j, the last of them onto the value's own variable -> (n_vars, public, gates, witness words).
    Variable 0 is zero (acc_0), the value's variable is public for value 0."""
    k = bits
    vals = (np.arange(n_values, dtype=np.uint64) * np.uint64(0x9E3779B1)) % np.uint64(1 << bits)
    j = np.arange(k, dtype=np.uint64)
    bit = (vals[:, None] >> j[None, :]) & np.uint64(1)                                     # (n_values, k)
    acc = np.cumsum(bit << j[None, :], axis=1, dtype=np.uint64)                            # acc_(j+1)
    per = 2 * k                                                                            # variables per value: k bits, k - 1 partial sums, the value
    base = 1 + per * np.arange(n_values, dtype=np.int64)
    b_var = base[:, None] + np.arange(k)[None, :]
    acc_var = base[:, None] + k + np.arange(k)[None, :]                                    # acc_1 .. acc_k; acc_k is the value
    prev = np.concatenate([np.zeros((n_values, 1), np.int64), acc_var[:, :-1]], axis=1)
    pw = _words([1 << i for i in range(k)] + [r - 1, 0, 1])                                # selector values: 2^j, -1, 0, 1
    NEG, ZERO, ONE = k, k + 1, k + 2
    rows = n_values * per
    code = {s: np.full(rows, ZERO, np.int64) for s in ("qL", "qR", "qO", "qM", "qC")}
    wire = {w: np.zeros(rows, np.uint32) for w in "abc"}
    bo = (np.arange(n_values)[:, None] * per + np.arange(k)[None, :]).reshape(-1)          # boolean rows
    ad = bo + k                                                                            # adding rows
    flat = lambda x: x.reshape(-1)
    wire["a"][bo] = wire["b"][bo] = flat(b_var)
    code["qM"][bo], code["qL"][bo] = ONE, NEG
    wire["a"][ad], wire["b"][ad], wire["c"][ad] = flat(prev), flat(b_var), flat(acc_var)
    code["qL"][ad], code["qO"][ad] = ONE, NEG
    code["qR"][ad] = flat(np.tile(np.arange(k), (n_values, 1)))
    gates = {s: pw[v] for s, v in code.items()}
    gates.update(wire)
    wit = np.zeros(1 + per * n_values, np.uint64)
    wit[flat(b_var)] = flat(bit)
    wit[flat(acc_var)] = flat(acc)
    return len(wit), [int(acc_var[0, -1])], gates, _small(wit)


def time_proofs(zk, mod, key, ww, reps, warmup, names):
    ev, runs = Events(), []
    for i in range(warmup + reps):
        proof, publics = mod.prove(key, ww, self_check=False, _mark=ev.mark)
        times = ev.take()
        assert mod.verify(key.vk, [publics], [proof]) == (mod.ACCEPTED, None), "a timed proof is not accepted"
        if i >= warmup:
            runs.append(times)
    med = {k: statistics.median(t[k] for t in runs) for k in names}
    med["total"] = statistics.median(sum(t[k] for k in names) for t in runs)
    return med


LOOKUP_ROUNDS = ["gate check", "lookup check", "round 1", "round 2", "round 3", "round 5"]
PLAIN_ROUNDS = ["gate check", "round 1", "round 2", "round 3", "round 5"]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-c", "--curve", default="BN128", choices=("BN128", "BLS12381"))
    ap.add_argument("--log-n", dest="log_n", type=int, action="append")
    ap.add_argument("--range-values-log", dest="values_log", type=int, default=14); ap.add_argument("--range-bits", dest="bits", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("-o", dest="out", default=None)
    a = ap.parse_args(argv)
    import eigen_zkvm_amd as zk
    zk.init(0)
    pl, plonk, fp = (importlib.import_module("eigen_zkvm_amd." + m) for m in ("plonk_lookup", "plonk", "frpoly"))
    cv, r = a.curve, pl.FR[a.curve]
    lines = ["PLONK with lookups on %s: HIP-event ms, median of %d after %d warm-ups; every proof verified" % (cv, a.reps, a.warmup), ""]

    def say(*ls):
        lines.extend(ls)
        print("\n".join(ls), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        for k in a.log_n or [16, 20]:
            n = 1 << k
            st = time_steps(zk, pl, fp, cv, k, a.reps, a.warmup)
            say("n = 2^%d, the steps alone:" % k, "", "| step | ms |", "|---|---|")
            say(*["| %s | %.3f |" % (name, st[name]) for name in ("table build", "count, spread", "count, one row", "terms + inverse + summands + prefix_sum",
                                                                 "lookup_quotient (4n points)", "prefix_sum", "prefix_product")])
            say("", "lookup_quotient moves %d bytes: %.0f GB/s" % (st["bytes of lookup_quotient"], st["bytes of lookup_quotient"] / st["lookup_quotient (4n points)"] / 1e6), "")
            kzg = _kzg(zk, fp, cv, k, pl.required_powers(n), tmp)
            n_vars, public, gates, table, ww = lookup_circuit_arrays(k, r, k - 1, n // 4, n // 2)
            key = pl.LookupKey(kzg, pl.LookupCircuit(n_vars, public, gates, table, cv))
            assert key.n == n
            lk = time_proofs(zk, pl, key, ww, a.reps, a.warmup, LOOKUP_ROUNDS)
            key.free()
            n_vars, public, gates, ww = chain_arrays(k, r)
            key = plonk.PlonkKey(kzg, plonk.Circuit(n_vars, public, gates, cv))
            pk = time_proofs(zk, plonk, key, ww, a.reps, a.warmup, PLAIN_ROUNDS)
            key.free(); kzg.free()
            say("n = 2^%d, a proof per round:" % k, "", "| prover | " + " | ".join(LOOKUP_ROUNDS) + " | total |", "|---|" + "---|" * (len(LOOKUP_ROUNDS) + 1))
            say("| with lookups | " + " | ".join("%.2f" % lk[x] for x in LOOKUP_ROUNDS + ["total"]) + " |")
            say("| plain (plonk.py) | " + " | ".join("%.2f" % pk[x] if x in pk else "" for x in LOOKUP_ROUNDS + ["total"]) + " |", "")
        # the use case
        nv, bits = 1 << a.values_log, a.bits
        n_vars, public, gates, table, ww = lookup_circuit_arrays(bits, r, 3, nv, 1 << bits)
        circuit = pl.LookupCircuit(n_vars, public, gates, table, cv)
        kzg = _kzg(zk, fp, cv, circuit.log_n, pl.required_powers(circuit.n), tmp)
        key = pl.LookupKey(kzg, circuit)
        lk = time_proofs(zk, pl, key, ww, a.reps, a.warmup, LOOKUP_ROUNDS)
        key.free(); kzg.free()
        n_vars, public, gates, ww = bits_circuit_arrays(nv, bits, r)
        plain = plonk.Circuit(n_vars, public, gates, cv)
        kzg = _kzg(zk, fp, cv, plain.log_n, plonk.required_powers(plain.n), tmp)
        key = plonk.PlonkKey(kzg, plain)
        pk = time_proofs(zk, plonk, key, ww, a.reps, a.warmup, PLAIN_ROUNDS)
        key.free(); kzg.free()
        say("2^%d values each proved below 2^%d:" % (a.values_log, bits), "", "| form | gates | n | proof ms |", "|---|---|---|---|",
            "| one lookup row per value | %d | 2^%d | %.2f |" % (circuit.n_gates, circuit.log_n, lk["total"]),
            "| bit decomposition, plain prover | %d | 2^%d | %.2f |" % (plain.n_gates, plain.log_n, pk["total"]), "")
    text = "\n".join(lines) + "\n"
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
