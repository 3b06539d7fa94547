"""Derives and checks the constants of csrc/pairing.hip (the optimal ate pairing of BN254 and BLS12-381 on the device) and emits
csrc/pairing_consts.hip.h.  Plain Python integers throughout.

Tower: Fq2 = Fq[u]/(u^2 + 1), Fq12 = Fq2[w]/(w^6 - xi); xi = 9 + u with a D-type twist (BN254), xi = 1 + u with an M-type twist
(BLS12-381).  An Fq12 element is its six Fq2 coefficients of w^0 .. w^5.  The constants:
  gamma_j[k] = xi^(k (q^j - 1) / 6), j = 1, 2, 3: the q^j-power Frobenius map is (conjugate^j of the coefficient of w^k) * gamma_j[k]
  the hard part of the final exponent, (q^4 - q^2 + 1) / r, as 4-bit digits
  the Miller loop counts 6t + 2 (BN254) and |x| (BLS12-381)
Field elements are emitted as 29-bit limbs of x R' mod q (R' = 2^(29 NR)), the internal form of fe29_impl.hip.h.

The file also carries `Model`, the algorithm of the kernels step by step (Jacobian line steps on the twist, sparse line products,
inversion through the norm to Fq2, Granger-Scott squarings, windowed hard part): `python tools/pairing_constants.py --check` runs it
against bilinearity and against the plain q^12-power definition; the kernels are a transcription of it.

python tools/pairing_constants.py            # prints the header
python tools/pairing_constants.py --write    # rewrites eigen-zkvm_amd/csrc/pairing_consts.hip.h
python tools/pairing_constants.py --check    # the model's self checks (a minute)"""
import pathlib
import sys

LB = 29


class Curve:
    def __init__(self, name, ns, q, r, xi, dtype, loop, bn, b, nr, g1, g2):
        self.name, self.ns, self.q, self.r, self.xi, self.dtype, self.loop, self.bn, self.b, self.nr = name, ns, q, r, xi, dtype, loop, bn, b, nr
        self.g1, self.g2 = g1, g2
        assert q % 4 == 3 and (q - 1) % 6 == 0
        self.hard = (q ** 4 - q ** 2 + 1) // r
        assert self.hard * r == q ** 4 - q ** 2 + 1
        self.gamma = {j: [self.f2pow(xi, k * (q ** j - 1) // 6) for k in range(6)] for j in (1, 2, 3)}
        for j in (1, 2, 3):                                   # gamma_j[1]^6 = xi^(q^j - 1), and the powers are consistent
            assert self.f2pow(self.gamma[j][1], 6) == self.f2mul(self.f2pow(xi, q ** j), self.f2inv(xi))
            for k in range(1, 6):
                assert self.gamma[j][k] == self.f2mul(self.gamma[j][k - 1], self.gamma[j][1])
        assert all(g[1] == 0 for g in self.gamma[2])           # xi^((q^2 - 1)/6) lies in Fq
        assert self.gamma[2][3] == (q - 1, 0)                  # w^3 -> -w^3 under the q^2 map
        # twist: y^2 = x^3 + b / xi (D) or b xi (M)
        self.bt = self.f2mul((b, 0), self.f2inv(xi)) if dtype else self.f2mul((b, 0), xi)

    # ---- Fq2 ----
    def f2add(self, a, b): return ((a[0] + b[0]) % self.q, (a[1] + b[1]) % self.q)
    def f2sub(self, a, b): return ((a[0] - b[0]) % self.q, (a[1] - b[1]) % self.q)
    def f2neg(self, a): return ((-a[0]) % self.q, (-a[1]) % self.q)
    def f2conj(self, a): return (a[0], (-a[1]) % self.q)
    def f2mul(self, a, b): return ((a[0] * b[0] - a[1] * b[1]) % self.q, (a[0] * b[1] + a[1] * b[0]) % self.q)
    def f2scale(self, a, s): return (a[0] * s % self.q, a[1] * s % self.q)
    def f2inv(self, a):
        n = pow(a[0] * a[0] + a[1] * a[1], -1, self.q)
        return (a[0] * n % self.q, (-a[1]) * n % self.q)
    def f2pow(self, a, e):
        r_ = (1, 0)
        while e:
            if e & 1: r_ = self.f2mul(r_, a)
            a = self.f2mul(a, a); e >>= 1
        return r_

    # ---- the twist, affine, for the checks ----
    def g2_add(self, P, Q):
        if P is None: return Q
        if Q is None: return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if self.f2add(y1, y2) == (0, 0): return None
            l = self.f2mul(self.f2scale(self.f2mul(x1, x1), 3), self.f2inv(self.f2scale(y1, 2)))
        else:
            l = self.f2mul(self.f2sub(y2, y1), self.f2inv(self.f2sub(x2, x1)))
        x3 = self.f2sub(self.f2sub(self.f2mul(l, l), x1), x2)
        return (x3, self.f2sub(self.f2mul(l, self.f2sub(x1, x3)), y1))
    def g2_mul(self, k, P):
        R = None
        while k:
            if k & 1: R = self.g2_add(R, P)
            P = self.g2_add(P, P); k >>= 1
        return R
    def g1_add(self, P, Q):
        q = self.q
        if P is None: return Q
        if Q is None: return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % q == 0: return None
            l = 3 * x1 * x1 * pow(2 * y1, -1, q) % q
        else:
            l = (y2 - y1) * pow(x2 - x1, -1, q) % q
        x3 = (l * l - x1 - x2) % q
        return (x3, (l * (x1 - x3) - y1) % q)
    def g1_mul(self, k, P):
        R = None
        while k:
            if k & 1: R = self.g1_add(R, P)
            P = self.g1_add(P, P); k >>= 1
        return R


BN254 = Curve("BN254", "bn254", 21888242871839275222246405745257275088696311157297823662689037894645226208583,
              21888242871839275222246405745257275088548364400416034343698204186575808495617, (9, 1), True,
              6 * 4965661367192848881 + 2, True, 3, 9, (1, 2),
              ((10857046999023057135944570762232829481370756359578518086990519993285655852781, 11559732032986387107991004021392285783925812861821192530917403151452391805634),
               (8495653923123431417604973247489272438418190587263600148770280649306958101930, 4082367875863433681332203403145435568316851327593401208105741076214120093531)))
BLS12_381 = Curve("BLS12-381", "bls12_381", 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab,
                  0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, (1, 1), False, 0xd201000000010000, False, 4, 14,
                  (0x17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb,
                   0x08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1),
                  ((0x024aa2b2f08f0a91260805272dc51051c6e47ad4fa403b02b4510b647ae3d1770bac0326a805bbefd48056c8c121bdb8,
                    0x13e02b6052719f607dacd3a088274f65596bd0d09920b61ab5da61bbdc7f5049334cf11213945d57e5ac7d055d042b7e),
                   (0x0ce5d527727d6e118cc9cdc6da2e351aadfd9baa8cbdd3a76d429a695160d12c923ac9cc3baca289e193548608b82801,
                    0x0606c4a02ea734cc32acd2b02bc28b99cb3e287e85a763af267492ab572e99ab3f370d275cec1da1aaa9075ff05f79be)))
CURVES = (BN254, BLS12_381)


class Model:
    """The kernels' algorithm on Python integers.  An Fq12 element is a list of six Fq2 pairs (the coefficients of w^0 .. w^5)."""
    def __init__(self, C):
        self.C = C

    def one(self): return [(1, 0)] + [(0, 0)] * 5
    def mul(self, a, b):                                       # coefficient k: sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j
        C, out = self.C, []
        for k in range(6):
            lo, hi = (0, 0), (0, 0)
            for i in range(6):
                t = C.f2mul(a[i], b[(k - i) % 6])
                if i <= k: lo = C.f2add(lo, t)
                else: hi = C.f2add(hi, t)
            out.append(C.f2add(lo, C.f2mul(C.xi, hi)))
        return out
    def conj6(self, a): return [a[k] if k % 2 == 0 else self.C.f2neg(a[k]) for k in range(6)]   # w -> -w: the q^6 map
    def frob2(self, a): return [self.C.f2scale(a[k], self.C.gamma[2][k][0]) for k in range(6)]
    def frob(self, a, j): return [self.C.f2mul(self.C.f2conj(a[k]) if j % 2 else a[k], self.C.gamma[j][k]) for k in range(6)]
    def inv(self, f):
        """f^-1 = fbar A B / (N A B) with fbar = conj6(f), N = f fbar in Fq6, A = N^(q^2), B = N^(q^4): N A B is the norm to Fq2"""
        C = self.C
        fbar = self.conj6(f)
        n = self.mul(f, fbar)
        a = self.frob2(n)
        ab = self.mul(a, self.frob2(a))
        t = self.mul(n, ab)
        assert all(t[k] == (0, 0) for k in range(1, 6))
        ti = C.f2inv(t[0])
        return [C.f2mul(x, ti) for x in self.mul(fbar, ab)]
    def cyc_sqr(self, a):
        """Granger-Scott: in the cyclotomic subgroup, with Fq4 = Fq2[s]/(s^2 - xi), s = w^3, and the pairs (a0, a3), (a1, a4), (a2, a5):
        lane k < 3 forms t_k = a_k^2 + xi a_{k+3}^2, lane k + 3 forms t_{k+3} = 2 a_k a_{k+3}; then
        a0' = 3 t0 - 2 a0, a3' = 3 t3 + 2 a3, a2' = 3 t1 - 2 a2, a5' = 3 t4 + 2 a5, a1' = 3 xi t5 + 2 a1, a4' = 3 t2 - 2 a4"""
        C = self.C
        t = [None] * 6
        for k in range(3):
            t[k] = C.f2add(C.f2mul(a[k], a[k]), C.f2mul(C.xi, C.f2mul(a[k + 3], a[k + 3])))
            t[k + 3] = C.f2scale(C.f2mul(a[k], a[k + 3]), 2)
        src = [t[0], C.f2mul(C.xi, t[5]), t[1], t[3], t[2], t[4]]
        sign = [-1, 1, -1, 1, -1, 1]
        return [C.f2add(C.f2scale(src[k], 3), C.f2scale(a[k], 2 * sign[k])) for k in range(6)]

    def line_dbl(self, T):
        """one doubling step on the Jacobian T = (X, Y, Z): ([2]T, the line's (cY, cX, c0))"""
        C = self.C
        m, s, sc = C.f2mul, C.f2sub, C.f2scale
        X, Y, Z = T
        A, B, ZZ = m(X, X), m(Y, Y), m(Z, Z)
        S = sc(m(X, B), 4); M = sc(A, 3)
        X3 = s(m(M, M), sc(S, 2)); Z3 = sc(m(Y, Z), 2)
        Y3 = s(m(M, s(S, X3)), sc(m(B, B), 8))
        return (X3, Y3, Z3), (m(Z3, ZZ), C.f2neg(m(M, ZZ)), s(m(M, X), sc(B, 2)))
    def line_add(self, T, x2, y2):
        """one addition step: (T + (x2, y2), the line's (cY, cX, c0))"""
        C = self.C
        m, s, sc = C.f2mul, C.f2sub, C.f2scale
        X, Y, Z = T
        ZZ = m(Z, Z)
        H, Rr = s(m(x2, ZZ), X), s(m(y2, m(ZZ, Z)), Y)
        HH = m(H, H); HHH = m(H, HH); V = m(X, HH)
        X3 = s(s(m(Rr, Rr), HHH), sc(V, 2)); Z3 = m(Z, H)
        Y3 = s(m(Rr, s(V, X3)), m(Y, HHH))
        return (X3, Y3, Z3), (Z3, C.f2neg(Rr), s(m(Rr, x2), m(y2, Z3)))
    def lines(self, Q):
        """the line coefficients (cY, cX, c0) of every step of the loop for the twist point Q = (x, y): Jacobian steps, no inversion"""
        C = self.C
        m, sc = C.f2mul, C.f2scale
        xq, yq = Q
        T = (xq, yq, (1, 0))
        out = []
        def dbl():
            nonlocal T
            T, ln = self.line_dbl(T)
            out.append(ln)
        def add(x2, y2):
            nonlocal T
            T, ln = self.line_add(T, x2, y2)
            out.append(ln)
        for i in range(C.loop.bit_length() - 2, -1, -1):
            dbl()
            if (C.loop >> i) & 1: add(xq, yq)
        if C.bn:
            g1, g2 = C.gamma[1], C.gamma[2]
            add(m(C.f2conj(xq), g1[2]), m(C.f2conj(yq), g1[3]))                 # pi(Q)
            add(sc(xq, g2[2][0]), C.f2neg(sc(yq, g2[3][0])))                    # -pi^2(Q)
        return out
    def line_mul(self, f, ln, P):
        """f times the sparse line value: D-type cY yP + cX xP w + c0 w^3; M-type c0 + cX xP w^2 + cY yP w^3"""
        C = self.C
        cy, cx, c0 = C.f2scale(ln[0], P[1]), C.f2scale(ln[1], P[0]), ln[2]
        sp = {0: cy, 1: cx, 3: c0} if C.dtype else {0: c0, 2: cx, 3: cy}
        out = []
        for k in range(6):
            acc = (0, 0)
            for p, v in sp.items():
                t = C.f2mul(f[(k - p) % 6], v)
                acc = C.f2add(acc, t if p <= k else C.f2mul(C.xi, t))
            out.append(acc)
        return out
    def miller(self, pairs):
        """product of the Miller values of (P in G1, Q on the twist) pairs; None = infinity contributes 1"""
        C = self.C
        pairs = [(P, self.lines(Q)) for P, Q in pairs if P is not None and Q is not None]
        f, step = self.one(), 0
        for i in range(C.loop.bit_length() - 2, -1, -1):
            f = self.mul(f, f)
            for P, ln in pairs: f = self.line_mul(f, ln[step], P)
            step += 1
            if (C.loop >> i) & 1:
                for P, ln in pairs: f = self.line_mul(f, ln[step], P)
                step += 1
        for _ in range(2 if C.bn else 0):
            for P, ln in pairs: f = self.line_mul(f, ln[step], P)
            step += 1
        return f if C.bn else self.conj6(f)                   # BLS12-381: x < 0
    def final_exp(self, f):
        C = self
        g = self.mul(self.conj6(f), self.inv(f))               # f^(q^6 - 1)
        g = self.mul(self.frob2(g), g)                         # ^(q^2 + 1): now in the cyclotomic subgroup
        tab = [self.one(), g]
        for d in range(2, 16): tab.append(self.mul(tab[-1], g))
        digits = hard_digits(self.C)
        r_ = tab[digits[0]]
        for d in digits[1:]:
            for _ in range(4): r_ = self.cyc_sqr(r_)
            if d: r_ = self.mul(r_, tab[d])
        return r_
    def pairing(self, P, Q): return self.final_exp(self.miller([(P, Q)]))
    def pow(self, a, e):
        r_ = self.one()
        while e:
            if e & 1: r_ = self.mul(r_, a)
            a = self.mul(a, a); e >>= 1
        return r_


def hard_digits(C):
    e, d = C.hard, []
    while e:
        d.append(e & 15); e >>= 4
    return d[::-1]


def limbs(C, v):
    v = v * (1 << (LB * C.nr)) % C.q
    return [(v >> (LB * i)) & ((1 << LB) - 1) for i in range(C.nr)]


def render():
    o = ["// GENERATED by tools/pairing_constants.py --write: do not edit.  Constants of the pairing (pairing.hip / pairing_impl.hip.h):",
         "// gamma_j[k] = xi^(k (q^j - 1)/6) as 29-bit limbs of x R' mod q (c0 then c1), the hard part (q^4 - q^2 + 1)/r of the final exponent",
         "// as 4-bit digits, most significant first, eight to a word, and the Miller loop counts.  tests/test_pairing_constants.py recomputes them.",
         "#pragma once", "namespace zk {"]
    for C in CURVES:
        dg = hard_digits(C)
        pad = dg + [0] * (-len(dg) % 8)
        words = [sum(pad[8 * i + j] << (4 * j) for j in range(8)) for i in range(len(pad) // 8)]
        o.append("namespace %s {" % C.ns)
        o.append("constexpr unsigned long long PAIR_LOOP_LO = 0x%xull;   // %s = 0x%x: its low 64 bits, and the bits above" % (C.loop & (2 ** 64 - 1), "6t + 2" if C.bn else "|x|", C.loop))
        o.append("constexpr unsigned PAIR_LOOP_HI = %du;" % (C.loop >> 64))
        o.append("constexpr int PAIR_LOOP_BITS = %d;" % C.loop.bit_length())
        o.append("constexpr bool PAIR_BN = %s, PAIR_DTYPE = %s;" % (str(C.bn).lower(), str(C.dtype).lower()))
        o.append("constexpr int PAIR_XI0 = %d;   // xi = PAIR_XI0 + u" % C.xi[0])
        o.append("static __device__ const unsigned PAIR_R[8] = {%s};   // the group order r, 32-bit words" % ", ".join("0x%08xu" % ((C.r >> (32 * i)) & 0xFFFFFFFF) for i in range(8)))
        o.append("constexpr int PAIR_HARD_DIGITS = %d;" % len(dg))
        o.append("static __device__ const unsigned PAIR_HARD[%d] = {%s};" % (len(words), ", ".join("0x%08xu" % w for w in words)))
        for j in (1, 2, 3):
            o.append("static __device__ const unsigned PAIR_GAMMA%d[6][%d] = {" % (j, 2 * C.nr))
            for k in range(6):
                g = C.gamma[j][k]
                o.append("    {%s}," % ", ".join("0x%08xu" % x for x in limbs(C, g[0]) + limbs(C, g[1])))
            o.append("};")
        bt = limbs(C, C.bt[0]) + limbs(C, C.bt[1])
        o.append("static __device__ const unsigned PAIR_TWIST_B[%d] = {%s};   // b' of the twist y^2 = x^3 + b'" % (2 * C.nr, ", ".join("0x%08xu" % x for x in bt)))
        o.append("static __device__ const unsigned PAIR_G1_B[%d] = {%s};   // b of y^2 = x^3 + b" % (C.nr, ", ".join("0x%08xu" % x for x in limbs(C, C.b))))
        o.append("}  // namespace %s" % C.ns)
    o.append("}  // namespace zk")
    return "\n".join(o) + "\n"


def check():
    import random
    rng = random.Random(1)
    for C in CURVES:
        M = Model(C)
        x, y = C.g2
        assert C.f2sub(C.f2mul(y, y), C.f2mul(x, C.f2mul(x, x))) == C.bt, "G2 generator is not on the twist"
        assert C.g2_mul(C.r, C.g2) is None and C.g1_mul(C.r, C.g1) is None
        e = M.pairing(C.g1, C.g2)
        assert e != M.one() and M.pow(e, C.r) == M.one()
        a, b = rng.randrange(1, C.r), rng.randrange(1, C.r)
        assert M.pairing(C.g1_mul(a, C.g1), C.g2_mul(b, C.g2)) == M.pow(e, a * b % C.r)
        f = M.miller([(C.g1, C.g2)])                              # the exact exponent, the long way
        g = M.mul(M.conj6(f), M.inv(f)); g = M.mul(M.frob2(g), g)
        assert M.mul(f, M.inv(f)) == M.one() and M.frob(f, 1) == M.pow(f, C.q) and M.frob(f, 2) == M.frob2(f) and M.frob(f, 3) == M.pow(f, C.q ** 3)
        assert M.cyc_sqr(g) == M.mul(g, g) and M.pow(g, C.hard) == e
        neg = (C.g1[0], C.q - C.g1[1])
        assert M.final_exp(M.miller([(C.g1, C.g2), (neg, C.g2)])) == M.one()
        print(C.name, "model ok")


if __name__ == "__main__":
    if "--check" in sys.argv:
        check()
    elif "--write" in sys.argv:
        (pathlib.Path(__file__).resolve().parent.parent / "eigen-zkvm_amd" / "csrc" / "pairing_consts.hip.h").write_text(render())
    else:
        sys.stdout.write(render())
