"""TEST INFRASTRUCTURE ONLY.  In-memory circuits with their witnesses for the wtns_check tests, over any of the three fields:
the writer is tests/c12_setup_ref.py's (it takes the field size and the prime)."""
import random

import c12_setup_ref as REF
import r1cs_check_ref as RC

FIELDS = ("BN128", "BLS12381", "GL")
SIZE = {"BN128": 32, "BLS12381": 32, "GL": 8}


def write(field, n_wires, cons, gates=(), uses=(), n_pub_in=1):
    return REF.write_r1cs(n_wires, 0, n_pub_in, n_wires - 1 - n_pub_in, cons, gates, uses, field_size=SIZE[field], prime=RC.PRIMES[field])


def wtns_bytes(field, w):
    """the .wtns file of a witness (iden3 binary format, version 2)"""
    import struct
    fs, p = SIZE[field], RC.PRIMES[field]
    return (b"wtns" + struct.pack("<II", 2, 2) + struct.pack("<IQ", 1, 4 + fs + 4) + struct.pack("<I", fs) + p.to_bytes(fs, "little")
            + struct.pack("<I", len(w)) + struct.pack("<IQ", 2, len(w) * fs) + b"".join(int(v).to_bytes(fs, "little") for v in w))


def products(field, n, seed=1):
    """n constraints (k a + k') * b = out_i over four input wires; every constraint has an output wire of its own that nothing else
    reads, so a wrong out_i breaks constraint i alone.  Wire 0 is not used.  -> (r1cs bytes, witness, [out wire of constraint i])"""
    p = RC.PRIMES[field]
    rng = random.Random(seed)
    w = [1] + [rng.randrange(p) for _ in range(4)]
    cons, outs = [], []
    for _ in range(n):
        a, a2, b = rng.randrange(1, 5), rng.randrange(1, 5), rng.randrange(1, 5)
        k, k2 = rng.randrange(1, p), rng.choice([1, p - 1, 7])
        lc_a = sorted({a: k, a2: k2}.items())
        w.append(sum(c * w[j] for j, c in lc_a) * w[b] % p)
        outs.append(len(w) - 1)
        cons.append((lc_a, [(b, 1)], [(outs[-1], 1)]))
    return write(field, len(w), cons), w, outs


def shapes(field, seed=3):
    """rows of 0 / 1 / 4 / 5 / 9 terms a side (both sides of the renormalisation cadence of 4; the first is A = B = C = empty),
    (p - 1) (p - 1) = 1, a row over wires that hold 0, and one row of 1000 terms with every coefficient and every wire p - 1.
    -> (r1cs bytes, witness, index of the long row, its c wire)"""
    p = RC.PRIMES[field]
    rng = random.Random(seed)
    w = [1] + [rng.randrange(p) for _ in range(12)]
    cons = []
    ev = lambda lc: sum(c * w[j] for j, c in lc) % p
    for t in (0, 1, 4, 5, 9):
        lc = lambda k: sorted((j, rng.choice([1, p - 1, rng.randrange(1, p)])) for j in rng.sample(range(0, 13), k))
        a, b, c = lc(t), lc(t), lc(max(t - 1, 0))
        if t:
            k = rng.randrange(1, p)
            w.append((ev(a) * ev(b) - ev(c)) * pow(k, -1, p) % p)
            c = c + [(len(w) - 1, k)]
        cons.append((a, b, c))
    w.append(p - 1); m1 = len(w) - 1
    cons.append(([(m1, 1)], [(m1, 1)], [(0, 1)]))                        # (p - 1)^2 = 1
    w.append(0); z = len(w) - 1
    cons.append(([(z, 5)], [(1, 1)], [(z, 3)]))                          # 0 = 0 over a wire that holds 0
    first = len(w)
    w.extend([p - 1] * 1000)
    w.append(1000 % p); cw = len(w) - 1
    cons.append(([(j, p - 1) for j in range(first, first + 1000)], [(0, 1)], [(cw, 1)]))   # 1000 x (p - 1)(p - 1) = 1000
    return write(field, len(w), cons), w, len(cons) - 1, cw


def one_constraint(field):
    """the shape of the reference's mycircuit (c <== a * b as circom writes it: -a * b = -c) -> r1cs bytes; witness [1, c, a, b]"""
    p = RC.PRIMES[field]
    return REF.write_r1cs(4, 1, 0, 2, [([(2, p - 1)], [(3, 1)], [(1, p - 1)])], field_size=SIZE[field], prime=p)


def corrupt(w, wire, delta=1, p=None):
    out = list(w)
    out[wire] = (out[wire] + delta) % (p or REF.P)
    return out
