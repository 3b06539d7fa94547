"""TEST INFRASTRUCTURE ONLY.  In-memory circuits for the compressor12 setup tests: random R1CS with all four constraint
kinds of r1cs2plonk.rs:199-218, uses of the four custom gates, and small circuits that come with a satisfying witness."""
import random

import c12_setup_ref as REF

P = REF.P
ALL_TEMPLATES = [("CMulAdd", []), ("Poseidon12", []), ("EvPol4", []), ("FFT4", [3, 5, 7, 4]), ("FFT4", [11, 13, 17, 2])]


def random_r1cs(seed, n_constraints, n_pub_in=3, n_wires=None, custom=(), gate_keys=None):
    """-> (bytes, dict for the restatement).  custom: names out of Poseidon12 / CMulAdd / FFT4_4 / FFT4_2 / EvPol4.
    Coefficients come from a small pool so that gates share keys: rows are shared only between equal coefficient sets, and
    the reference counts its rows (plonk_setup.rs:54-78) as if at most one half row stayed empty.  A circuit whose gates
    arrive in an order that leaves more of them empty makes the reference index past its s_map (a panic); such a draw is
    outside the reference's domain and the next salt is taken."""
    for salt in range(400):
        b, r = _random_r1cs(seed * 1000 + salt, n_constraints, n_pub_in, n_wires, custom, gate_keys)
        if _fits(r): return b, r
    raise AssertionError("no circuit inside the reference's domain in 400 draws")


def _fits(r):
    """the reference's row count (plonk_setup.rs:54-78) against the rows its packing loop (:271-360) opens, keys only"""
    pg, _ = REF.r1cs2plonk(r)
    uses = {}
    for g in pg: uses[g[3:8]] = uses.get(g[3:8], 0) + 1
    counted = (sum((u - 1) // 2 + 1 for u in uses.values()) - 1) // 2 + 1
    partial, half, rows = {}, 0, 0
    for g in pg:
        k = g[3:8]
        if k in partial:
            partial[k] += 1
            if partial[k] == 2: half += 1; del partial[k]
            elif partial[k] == 4: del partial[k]
        elif half: half -= 1; partial[k] = 3
        else: rows += 1; partial[k] = 1
    return rows <= counted


def _random_r1cs(seed, n_constraints, n_pub_in, n_wires, custom, gate_keys):
    rng = random.Random(seed)
    n_wires = n_wires or max(n_pub_in + 2, n_constraints // 2 + n_pub_in + 2)
    pool = gate_keys or [1]
    wire = lambda: rng.randrange(1, n_wires)
    coef = lambda: rng.choice(pool)

    def lc(n, with_const=False):
        ws = rng.sample(range(1, n_wires), min(n, n_wires - 1))
        out = [(w, coef()) for w in ws]
        if with_const: out.append((0, coef()))
        rng.shuffle(out)                                                # the reader sorts by wire
        return out

    cons = []
    for i in range(n_constraints):
        kind = i % 6
        if kind == 0: cons.append((lc(1), lc(1), lc(1)))                                   # a multiplication
        elif kind == 1: cons.append((lc(2, True), lc(3), lc(2, True)))                      # a multiplication whose sides are sums
        elif kind == 2: cons.append(([], [], lc(rng.randrange(1, 7), rng.random() < 0.5))) # A = 0: a sum of up to 6 terms
        elif kind == 3: cons.append(([(0, coef())], lc(2), lc(2)))                         # k * B
        elif kind == 4: cons.append((lc(3, True), [(0, coef())], lc(1)))                   # A * k
        else: cons.append((lc(1), [(wire(), 0)], lc(4)))                                   # a zero coefficient: B is "0"
    gates, uses = [], []
    if custom:
        gates = list(ALL_TEMPLATES)
        ids = {"CMulAdd": 0, "Poseidon12": 1, "EvPol4": 2, "FFT4_4": 3, "FFT4_2": 4}
        n_sig = {"CMulAdd": 12, "Poseidon12": 372, "EvPol4": 21, "FFT4_4": 24, "FFT4_2": 24}
        for name in custom:
            uses.append((ids[name], [rng.choice([0, wire()]) if rng.random() < 0.1 else wire() for _ in range(n_sig[name])]))
    b = REF.write_r1cs(n_wires, 0, n_pub_in, n_wires - 1 - n_pub_in, cons, gates, uses)
    return b, REF.read_r1cs(b)


def plain_circuit(n_mul=20, n_sum=9, n_pub_in=3, seed=1):
    """A satisfiable circuit of multiplications and sums: -> (r1cs bytes, witness list).  Wires 1..n_pub_in are public."""
    rng = random.Random(seed)
    w = [1] + [rng.randrange(P) for _ in range(n_pub_in + 3)]
    cons = []
    for _ in range(n_mul):                                              # (a + k) * (b) = c with c a new wire
        a, b = rng.randrange(1, len(w)), rng.randrange(1, len(w))
        k = rng.choice([0, 5])
        w.append((w[a] + k) * w[b] % P)
        cons.append(([(a, 1)] + ([(0, k)] if k else []), [(b, 1)], [(len(w) - 1, 1)]))
    for _ in range(n_sum):                                              # sum of five wires + constant - new wire = 0
        ws = rng.sample(range(1, len(w)), 5)
        cs = [1 for _ in ws]
        k = 7
        w.append((sum(c * w[x] for c, x in zip(cs, ws)) + k) % P)
        cons.append(([], [], [(x, c) for c, x in zip(cs, ws)] + [(0, k), (len(w) - 1, P - 1)]))
    return REF.write_r1cs(len(w), 0, n_pub_in, len(w) - 1 - n_pub_in, cons), w


def cmul(a, b):
    """product in the cubic extension x^3 = x - 1 (the CMulAdd gate's Karatsuba form evaluates this)"""
    A = (a[0] + a[1]) * (b[0] + b[1]); B = (a[0] + a[2]) * (b[0] + b[2]); C = (a[1] + a[2]) * (b[1] + b[2])
    D = a[0] * b[0]; E = a[1] * b[1]; F = a[2] * b[2]
    return [(C + D - E - F) % P, (A + C - 2 * E - D) % P, (B - D + E) % P]


def _poseidon_matrix():
    """ZK_POSEIDON_M of csrc/poseidon_gl_constants.h: out[i] = sum_j M[j * 12 + i] * state[j]"""
    import pathlib, re
    text = (pathlib.Path(__file__).resolve().parent.parent / "eigen-zkvm_amd" / "csrc" / "poseidon_gl_constants.h").read_text()
    body = text.split("ZK_POSEIDON_M[144]")[1].split("};")[0]
    m = [int(x, 16) for x in re.findall(r"0x[0-9a-fA-F]+", body)]
    assert len(m) == 144
    return m


def poseidon_rows(state):
    """the 31 row states of one Poseidon12 use: row j + 1 = MDS(sbox(row j + C_j)), full rounds 0..3 and 26..29, partial between"""
    M, C = _poseidon_matrix(), REF.project_cposeidon()
    rows = [list(state)]
    for j in range(30):
        s = [(rows[-1][i] + C[12 * j + i]) % P for i in range(12)]
        s = [pow(v, 7, P) if (i == 0 or not 4 <= j < 26) else v for i, v in enumerate(s)]
        rows.append([sum(M[k * 12 + i] * s[k] for k in range(12)) % P for i in range(12)])
    return rows


def fft4_next_row(a, params):
    """the row an FFT4 use forces below `a` (12 values = four cubic-extension elements), from the template's parameters"""
    first_w, inc_w, scale, typ = params
    C = [0] * 12
    if typ == 4:
        C[0:6] = [scale, scale * first_w ** 2, scale * first_w, scale * first_w ** 3, scale * first_w * inc_w, scale * first_w ** 3 * inc_w]
    else:
        C[6:9] = [scale, scale * first_w, scale * first_w * inc_w]
    out = []
    for q, (s1, c2, s2, c3, s3, x4, x5, c5, s5) in enumerate([(1, 2, 1, 3, 1, 0, 3, 7, 1), (-1, 4, 1, 5, -1, 0, 3, 7, -1),
                                                               (1, 2, -1, 3, -1, 6, 9, 8, 1), (-1, 4, -1, 5, 1, 6, 9, 8, -1)]):
        for c in range(3):
            out.append((C[0] * a[c] + s1 * C[1] * a[3 + c] + s2 * C[c2] * a[6 + c] + s3 * C[c3] * a[9 + c]
                        + C[6] * a[x4 + c] + s5 * C[c5] * a[x5 + c]) % P)
    return out


def with_custom(kind, seed=2):
    """plain_circuit plus custom-gate uses on fresh wires, with the witness the gates force:
    cmuladd   a[9..12) = a[0..3) * a[3..6) + a[6..9)
    poseidon  31 rows of round states
    fft4      one use of each type: 12 inputs, 12 outputs
    evpol4    Horner over the coefficients a[0..12) at x, started from an accumulator"""
    rng = random.Random(seed)
    b, w = plain_circuit(seed=seed)
    r1 = REF.read_r1cs(b)
    uses = []

    def fresh(vals):
        ids = list(range(len(w), len(w) + len(vals)))
        w.extend(vals)
        return ids

    rnd = lambda n: [rng.randrange(P) for _ in range(n)]
    if kind == "cmuladd":
        x = rnd(9); m = cmul(x[0:3], x[3:6])
        uses.append((0, fresh(x + [(m[i] + x[6 + i]) % P for i in range(3)])))
    elif kind == "poseidon":
        uses.append((1, fresh([v for row in poseidon_rows(rnd(12)) for v in row])))
    elif kind == "fft4":
        for gid in (3, 4):
            a = rnd(12)
            uses.append((gid, fresh(a + fft4_next_row(a, ALL_TEMPLATES[gid][1]))))
    elif kind == "evpol4":
        coef, acc, x = rnd(12), rnd(3), rnd(3)
        res = acc
        for c in (9, 6, 3, 0):
            m = cmul(res, x); res = [(m[i] + coef[c + i]) % P for i in range(3)]
        uses.append((2, fresh(coef + acc + x + res)))
    else:
        raise ValueError(kind)
    return REF.write_r1cs(len(w), 0, 3, len(w) - 4, r1["constraints"], list(ALL_TEMPLATES), uses), w


def with_cmuladd(seed=2):
    return with_custom("cmuladd", seed)
