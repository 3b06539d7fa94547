"""TEST INFRASTRUCTURE ONLY.  The yardstick of the R1CS import of the PLONK prover in plain Python integers: the compile
rule -- an .r1cs file -> a gate table of fan-in 2, the constraint every gate came from, and the segments that define the auxiliary
variables -- and the extension of a witness by those segments.  It reads the file itself and shares no code with the package.  No test.

The rule.  Wire w is variable w; auxiliaries follow from n_wires in the order they are emitted; wire 0 (the constant 1) is never a gate
operand with a non-zero selector: its terms become constants.  A side is normalised (equal wires added, zeros dropped, wire 0 taken out as
the constant k, the signals by ascending wire).  reduce(sig, keep) folds the first m = len - keep + 1 signals into m - 1 auxiliaries, each
a PREFIX of the side's sum over original wires, x_j = sum_{i <= j + 1} c_i w[s_i]: gate 1 is (c_1, c_2, -1, 0, 0) on (s_1, s_2, x_1), gate
j >= 2 is (1, c_(j+1), -1, 0, 0) on (x_(j-1), s_(j+1), x_j); one segment (the first auxiliary, the m terms) per fold.  A constraint
A B = C with a side A or B that has no signal is linear: L = kA B_sig - C_sig (or kB A_sig - C_sig), normalised again, k0 = kA kB - kC;
nothing is left -> no gate when k0 = 0 and a refusal otherwise; else reduce(L, 3) and one gate (c_1, c_2, c_3, 0, k0).  Every other
constraint is a product: reduce(A, 1), reduce(B, 1), reduce(C, 1), then qM = fA fB, qL = fA kB, qR = kA fB, qO = -fC, qC = kA kB - kC."""
import pathlib
import struct

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
FIELDS = ("BN128", "BLS12381")
R = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
SELECTORS = ("qL", "qR", "qO", "qM", "qC")
WIRES = ("a", "b", "c")


class Refused(Exception):
    pass


def read_r1cs(data):
    """-> (prime, n_wires, n_pub_out, n_pub_in, [(A, B, C)]) with every side a list of (wire, coefficient) in file order"""
    assert data[:4] == b"r1cs"
    n_sec = struct.unpack_from("<I", data, 8)[0]
    secs, o = {}, 12
    for _ in range(n_sec):
        t, sz = struct.unpack_from("<IQ", data, o)
        secs[t] = data[o + 12:o + 12 + sz]
        o += 12 + sz
    head = secs[1]
    fs = struct.unpack_from("<I", head)[0]
    prime = int.from_bytes(head[4:4 + fs], "little")
    n_wires, n_out, n_in, _, _, n_cons = struct.unpack_from("<IIIIQI", head, 4 + fs)
    body, o, cons = secs[2], 0, []
    for _ in range(n_cons):
        sides = []
        for _ in range(3):
            nv = struct.unpack_from("<I", body, o)[0]
            o += 4
            lc = []
            for _ in range(nv):
                lc.append((struct.unpack_from("<I", body, o)[0], int.from_bytes(body[o + 4:o + 4 + fs], "little")))
                o += 4 + fs
            sides.append(lc)
        cons.append(tuple(sides))
    return prime, n_wires, n_out, n_in, cons


def normalise(side, p):
    """-> (the signals by ascending wire with non-zero coefficients, the constant k)"""
    acc = {}
    for w, c in side:
        acc[w] = (acc.get(w, 0) + c) % p
    k = acc.pop(0, 0)
    return sorted((w, c) for w, c in acc.items() if c), k


class Compiled:
    """n_wires, n_public, n_constraints, n_vars, n_aux; gates: qL .. qC (integers below p) and a, b, c (variable ids); origin[g]: the
    constraint of gate g; public: the variable ids 1 .. l; segments: [(first auxiliary id, [(wire, coefficient)])]"""

    def __init__(self, data, field):
        self.field, self.p = field, R[field]
        p = self.p
        prime, self.n_wires, n_out, n_in, cons = read_r1cs(data)
        if prime != p:
            raise Refused("the file is over another field")
        self.n_public, self.n_constraints = n_out + n_in, len(cons)
        self.public = list(range(1, self.n_public + 1))
        self.gates = {k: [] for k in SELECTORS + WIRES}
        self.origin, self.segments = [], []
        self.n_vars = self.n_wires
        for i, sides in enumerate(cons):
            for side in sides:
                for w, _ in side:
                    if w >= self.n_wires:
                        raise Refused("constraint %d: wire %d of %d" % (i, w, self.n_wires))
            (A, kA), (B, kB), (C, kC) = (normalise(s, p) for s in sides)
            if not A or not B:
                kk, S = (kA, B) if not A else (kB, A)
                L, _ = normalise([(w, kk * c) for w, c in S] + [(w, -c) for w, c in C], p)
                k0 = (kA * kB - kC) % p
                if not L:
                    if k0:
                        raise Refused("constraint %d is 0 = %d" % (i, k0))
                    continue
                L = self._reduce(i, L, 3)
                L = L + [(0, 0)] * (3 - len(L))
                self._emit(i, L[0][0], L[1][0], L[2][0], qL=L[0][1], qR=L[1][1], qO=L[2][1], qC=k0)
            else:
                (sA, fA), = self._reduce(i, A, 1)
                (sB, fB), = self._reduce(i, B, 1)
                sC, fC = self._reduce(i, C, 1)[0] if C else (0, 0)
                self._emit(i, sA, sB, sC, qM=fA * fB, qL=fA * kB, qR=kA * fB, qO=-fC, qC=kA * kB - kC)
        if self.n_vars >= 1 << 32:
            raise Refused("n_vars does not fit 32 bits")
        self.n_aux = self.n_vars - self.n_wires
        self.n_gates = len(self.origin)

    def _emit(self, i, a, b, c, qL=0, qR=0, qO=0, qM=0, qC=0):
        for k, v in zip(SELECTORS, (qL, qR, qO, qM, qC)):
            self.gates[k].append(v % self.p)
        for k, v in zip(WIRES, (a, b, c)):
            self.gates[k].append(v)
        self.origin.append(i)

    def _reduce(self, i, sig, keep):
        if len(sig) <= keep:
            return sig
        m = len(sig) - keep + 1
        first = self.n_vars
        self.segments.append((first, sig[:m]))
        self._emit(i, sig[0][0], sig[1][0], first, qL=sig[0][1], qR=sig[1][1], qO=-1)
        for j in range(2, m):
            self._emit(i, first + j - 2, sig[j][0], first + j - 1, qL=1, qR=sig[j][1], qO=-1)
        self.n_vars += m - 1
        return [(first + m - 2, 1)] + sig[m:]

    def extend(self, witness):
        """n_wires values -> n_vars values: every auxiliary is a prefix of its segment's sum over the original wires"""
        assert len(witness) == self.n_wires
        out = [int(v) % self.p for v in witness] + [0] * self.n_aux
        for first, terms in self.segments:
            acc = 0
            for j, (s, c) in enumerate(terms):
                acc = (acc + c * out[s]) % self.p
                if j:
                    out[first + j - 1] = acc
        return out

    def failing_gates(self, values):
        """the gates the n_vars values do not satisfy (no public rows here: those hold by construction)"""
        g, p, bad = self.gates, self.p, []
        for i in range(self.n_gates):
            a, b, c = values[g["a"][i]], values[g["b"][i]], values[g["c"][i]]
            if (g["qL"][i] * a + g["qR"][i] * b + g["qO"][i] * c + g["qM"][i] * a * b + g["qC"][i]) % p:
                bad.append(i)
        return bad

    def tables(self):
        """what the library's tables call copies out, as plain lists: the five selectors, a, b, c, origin, then the segment table as
        (first auxiliary per segment, the offsets of the segments' terms, the wire and the coefficient of every term)"""
        ptr, wires, coefs = [0], [], []
        for _, terms in self.segments:
            wires += [s for s, _ in terms]
            coefs += [c for _, c in terms]
            ptr.append(len(wires))
        return {**self.gates, "origin": list(self.origin), "seg_first": [f for f, _ in self.segments], "seg_ptr": ptr, "seg_wire": wires, "seg_coef": coefs}


def circuits(field):
    """the circuits the CPU tests walk: (name, r1cs bytes, witness, [(an output wire, its constraint)])"""
    import r1cs_check_cases as cases
    data, w, outs = cases.products(field, 37)
    yield "products", data, w, [(o, i) for i, o in enumerate(outs)]
    data, w, long_row, cw = cases.shapes(field)
    yield "shapes", data, w, [(cw, long_row)]
    yield "one_constraint", cases.one_constraint(field), [1, 6, 2, 3], [(1, 0)]
    if field == "BN128":
        yield "multiplier", (GOLDEN / "plonk" / "multiplier.r1cs").read_bytes(), [1, 11210000, 1121, 10000], [(1, 0)]
    else:
        yield "mycircuit", (GOLDEN / "groth16" / "mycircuit_bls12381.r1cs").read_bytes(), [1, 11210000, 1121, 10000], [(1, 0)]
