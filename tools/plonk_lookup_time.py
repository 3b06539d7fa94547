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
decomposition through the plain prover (per value b boolean gates and b gates that add the bits up: 2b rows), at the n each needs.
The tagged section (--section tagged, or all; what profiles/r29/plonk_lookup_tagged.md records), per n = 2^k:
  kernel by kernel  the tagged table build, count, terms and quotient beside their three-column forms over the same arrays in the same
                    run: median, smallest and largest of the repetitions, and the ratio of the medians
  a proof           n / 4 lookups into two tagged tables of n / 4 rows each (a range table, an XOR table) beside the single-table proof
                    above: the same number of selected rows and of table rows
The tagged use case: 2^14 eight-bit range checks and 2^12 four-bit XORs as ONE tagged proof, against one single-table proof for each."""
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


def _spread(ev, fn, reps, warmup):
    """-> (median, smallest, largest) of `reps` after `warmup`"""
    ts = []
    for _ in range(warmup + reps):
        ev.mark("start"); fn(); ev.mark("run")
        ts.append(ev.take()["run"])
    return statistics.median(ts[warmup:]), min(ts[warmup:]), max(ts[warmup:])


def time_tagged_steps(zk, pl, fp, curve, log_n, reps, warmup):
    """the tagged kernels beside their three-column forms at n = 2^log_n, over the same arrays: four tables of n / 4 rows, the tag of a
    looked-up row in q_K -> [(step, (median, min, max) plain, (median, min, max) tagged)]"""
    n, ev, rows = 1 << log_n, Events(), []
    mont = importlib.import_module("eigen_zkvm_amd.plonk_arith").mont_dev
    idx = np.arange(n, dtype=np.uint64)
    tag_of = lambda rows_: np.uint64(1) + rows_ // np.uint64(n // 4)
    s_idx, h_idx = (idx * np.uint64(0x9E3779B1)) % np.uint64(n), 0 * idx + np.uint64(12345 % n)
    t1, zero, one, t0 = mont(curve, _small(idx)), mont(curve, _small(0 * idx)), mont(curve, _small(0 * idx + 1)), mont(curve, _small(tag_of(idx)))
    spread, hot, qk_s, qk_h = mont(curve, _small(s_idx)), mont(curve, _small(h_idx)), mont(curve, _small(tag_of(s_idx))), mont(curve, _small(tag_of(h_idx)))
    made = []
    plain = _spread(ev, lambda: made.append(pl.LookupTable(t1, zero, zero, n, curve)), reps, warmup)
    tab = made[-1]
    tagged = _spread(ev, lambda: made.append(pl.LookupTable(t1, zero, zero, n, curve, tag=t0)), reps, warmup)
    ttab = made[-1]
    rows.append(("table_new (n rows)", plain, tagged))
    m = zk.DevArray(4 * n)
    for name, a, q in (("count, spread", spread, qk_s), ("count, one row", hot, qk_h)):
        plain = _spread(ev, lambda: pl.count(tab, a, zero, zero, one, n, out=m), reps, warmup)
        tagged = _spread(ev, lambda: pl.count(ttab, a, zero, zero, q, n, out=m), reps, warmup)
        assert pl.count(tab, a, zero, zero, one, n, out=m)[1] == 0 and pl.count(ttab, a, zero, zero, q, n, out=m)[1] == 0
        rows.append((name, plain, tagged))
    def run_terms(cols, tagged):
        pl.terms(cols, n, 0x1111, 0x2222, curve, tagged=tagged).free()
    rows.append(("terms (2n lanes)", _spread(ev, lambda: run_terms([spread, zero, zero, t1, zero, zero], False), reps, warmup),
                 _spread(ev, lambda: run_terms([spread, zero, zero, qk_s, t1, zero, zero, t0], True), reps, warmup)))
    cols = [fp.powers(5 + 2 * j, 7 + j, 4 * n, curve, dev=True) for j in range(11)]
    rows.append(("lookup_quotient (4n points)", _spread(ev, lambda: pl.lookup_quotient(cols[:9], log_n, 0x1111, 0x2222, 0x3333, cols[10], curve), reps, warmup),
                 _spread(ev, lambda: pl.lookup_quotient(cols[:10], log_n, 0x1111, 0x2222, 0x3333, cols[10], curve, tagged=True), reps, warmup)))
    for t in made:
        t.free()
    for d in cols + [t1, zero, one, t0, spread, hot, qk_s, qk_h, m]:
        d.free()
    return rows


def mixed_circuit_arrays(r, chain_log, n_range, range_bits, n_xor, xor_bits, tagged):
    """plonk_time's chain in 2^chain_log rows, then n_range range lookups (a = a fresh variable, b = c = variable 0) into (v, 0, 0),
    v < 2^range_bits, and n_xor lookups (three fresh variables) into (x, y, x ^ y), x, y < 2^xor_bits.  tagged: the two tables apart, q_K
    = 1 and 2; else q_K = 1 and the one table that is asked for (n_range = 0 or n_xor = 0) -> (n_vars, public, gates, table words or
    the list of the two, witness words)"""
    n_vars, public, gates, ww = chain_arrays(chain_log, r)
    m, nl = len(gates["a"]), n_range + n_xor
    for k in ("qL", "qR", "qO", "qM", "qC"):
        gates[k] = np.concatenate([gates[k], np.zeros((nl, 4), np.uint64)])
    v0 = n_vars + n_range
    xv = v0 + 3 * np.arange(n_xor, dtype=np.uint32)
    gates["a"] = np.concatenate([gates["a"], np.arange(n_vars, v0, dtype=np.uint32), xv])
    gates["b"] = np.concatenate([gates["b"], np.zeros(n_range, np.uint32), xv + np.uint32(1)])
    gates["c"] = np.concatenate([gates["c"], np.zeros(n_range, np.uint32), xv + np.uint32(2)])
    sel = np.concatenate([np.ones(n_range, np.uint64), np.full(n_xor, 2 if tagged else 1, np.uint64)])
    gates["qK"] = np.concatenate([np.zeros((m, 4), np.uint64), _small(sel)])
    vals = (np.arange(n_range, dtype=np.uint64) * np.uint64(0x9E3779B1)) % np.uint64(1 << range_bits)
    x = (np.arange(n_xor, dtype=np.uint64) * np.uint64(0x9E3779B1)) % np.uint64(1 << xor_bits)
    y = (np.arange(n_xor, dtype=np.uint64) * np.uint64(0x85EBCA6B)) % np.uint64(1 << xor_bits)
    xor_vars = np.stack([x, y, x ^ y], axis=1).reshape(-1)
    t_range = np.zeros((1 << range_bits, 3, 4), np.uint64)
    t_range[:, 0, 0] = np.arange(1 << range_bits, dtype=np.uint64)
    side = np.arange(1 << xor_bits, dtype=np.uint64)
    gx, gy = np.repeat(side, 1 << xor_bits), np.tile(side, 1 << xor_bits)
    t_xor = np.zeros((1 << (2 * xor_bits), 3, 4), np.uint64)
    t_xor[:, 0, 0], t_xor[:, 1, 0], t_xor[:, 2, 0] = gx, gy, gx ^ gy
    tables = [t_range, t_xor] if tagged else (t_range if n_range else t_xor)
    return n_vars + n_range + 3 * n_xor, public, gates, tables, np.concatenate([ww, _small(vals), _small(xor_vars)])


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


def base_sections(a, zk, pl, plonk, fp, cv, r, tmp, say):
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


def tagged_sections(a, zk, pl, fp, cv, r, tmp, say):
    fmt = lambda t: "%.3f (%.3f .. %.3f)" % t
    for k in a.log_n or [16, 20]:
        n = 1 << k
        say("n = 2^%d, the tagged kernels beside their three-column forms: ms, median (smallest .. largest):" % k, "", "| step | three columns | tagged | ratio |", "|---|---|---|---|")
        say(*["| %s | %s | %s | %.2f |" % (name, fmt(p), fmt(t), t[0] / p[0]) for name, p, t in time_tagged_steps(zk, pl, fp, cv, k, a.reps, a.warmup)], "")
        kzg = _kzg(zk, fp, cv, k, pl.required_powers(n), tmp)
        res = []
        for tagged in (False, True):
            if tagged:
                n_vars, public, gates, tables, ww = mixed_circuit_arrays(r, k - 1, n // 8, k - 2, n // 8, (k - 2) // 2, True)
                circuit = pl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables)
            else:
                n_vars, public, gates, table, ww = lookup_circuit_arrays(k, r, k - 1, n // 4, n // 2)
                circuit = pl.LookupCircuit(n_vars, public, gates, table, cv)
            key = pl.LookupKey(kzg, circuit)
            assert key.n == n and key.tagged == tagged and circuit.n_table == n // 2 and int((circuit.gates["qK"][:, 0] != 0).sum()) == n // 4
            res.append(time_proofs(zk, pl, key, ww, a.reps, a.warmup, LOOKUP_ROUNDS))
            key.free()
        kzg.free()
        say("n = 2^%d, a proof per round, n / 4 selected rows, n / 2 table rows:" % k, "", "| protocol | " + " | ".join(LOOKUP_ROUNDS) + " | total |", "|---|" + "---|" * (len(LOOKUP_ROUNDS) + 1))
        for name, t in zip(("single table", "tagged, two tables"), res):
            say("| %s | " % name + " | ".join("%.2f" % t[x] for x in LOOKUP_ROUNDS + ["total"]) + " |")
        say("")
    # the use case: range checks and XORs in one circuit
    n_range, n_xor = 1 << 14, 1 << 12
    out = []
    for name, args, tagged in (("one tagged proof: 2^14 range checks and 2^12 XORs", (n_range, 8, n_xor, 4), True), ("single table: the 2^14 range checks", (n_range, 8, 0, 4), False),
                               ("single table: the 2^12 XORs", (0, 8, n_xor, 4), False)):
        n_vars, public, gates, tables, ww = mixed_circuit_arrays(r, 3, *args, tagged)
        circuit = pl.LookupCircuit(n_vars, public, gates, curve=cv, tables=tables) if tagged else pl.LookupCircuit(n_vars, public, gates, tables, cv)
        kzg = _kzg(zk, fp, cv, circuit.log_n, pl.required_powers(circuit.n), tmp)
        key = pl.LookupKey(kzg, circuit)
        out.append((name, circuit, time_proofs(zk, pl, key, ww, a.reps, a.warmup, LOOKUP_ROUNDS)["total"]))
        key.free(); kzg.free()
    say("2^14 eight-bit range checks and 2^12 four-bit XORs:", "", "| form | gates | table rows | n | proof ms |", "|---|---|---|---|---|")
    say(*["| %s | %d | %d | 2^%d | %.2f |" % (name, c.n_gates, c.n_table, c.log_n, ms) for name, c, ms in out])
    say("| the two single-table proofs together | | | | %.2f |" % (out[1][2] + out[2][2]), "")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("-c", "--curve", default="BN128", choices=("BN128", "BLS12381"))
    ap.add_argument("--log-n", dest="log_n", type=int, action="append")
    ap.add_argument("--range-values-log", dest="values_log", type=int, default=14); ap.add_argument("--range-bits", dest="bits", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--section", choices=("all", "base", "tagged"), default="all", help="base: what profiles/r27 records; tagged: the tagged lookups beside the single-table ones")
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
        if a.section != "tagged":
            base_sections(a, zk, pl, plonk, fp, cv, r, tmp, say)
        if a.section != "base":
            tagged_sections(a, zk, pl, fp, cv, r, tmp, say)
    text = "\n".join(lines) + "\n"
    if a.out:
        pathlib.Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
