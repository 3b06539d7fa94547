"""The yardstick of the scalar-field polynomial layer (tests/frpoly_ref.py) against itself, without a GPU: identities that hold for any
correct implementation and tie its functions to each other."""
import random

import frpoly_ref as ref


def test_running_products_and_inverses():
    rng = random.Random(21)
    for curve, r in ref.R.items():
        for n in (0, 1, 2, 17):
            v = [rng.randrange(r) for _ in range(n)]
            ex, total = ref.prefix_products(v, r)
            inc, total2 = ref.prefix_products(v, r, inclusive=True)
            assert total == total2 and len(ex) == len(inc) == n
            assert ex == [1] * min(n, 1) + inc[:-1] and (not n or inc[-1] == total)
            inv, nz, first = ref.inverses(v, r)
            assert all(x * y % r == 1 for x, y in zip(v, inv) if x) and nz == v.count(0) and first is None
        inv, nz, first = ref.inverses([5, 0, 7, 0], r)
        assert inv[1] == inv[3] == 0 and (nz, first) == (2, 1) and inv[0] * 5 % r == 1
        assert ref.prefix_products([3, 0, 4], r) == ([1, 3, 0], 0)
        assert ref.prefix_products([r - 1] * 4, r, inclusive=True) == ([r - 1, 1, r - 1, 1], 1)


def test_pointwise_powers_terms_grand_product():
    rng = random.Random(22)
    for curve, r in ref.R.items():
        a = [rng.randrange(r) for _ in range(9)]; b = [rng.randrange(1, r) for _ in range(9)]
        assert ref.pointwise("sub", ref.pointwise("add", a, b, r), b, r) == a
        assert ref.pointwise("mul", ref.pointwise("mul", a, b, r), ref.inverses(b, r)[0], r) == a
        w = ref.root_of_unity(curve, 3)
        p = ref.powers(w, 5, 9, r)
        assert p[0] == 5 and p[8] == 5 and p[4] == r - 5 and ref.powers(0, 3, 3, r) == [3, 0, 0]
        beta, gamma = rng.randrange(r), rng.randrange(r)
        t = ref.terms([a, b], [b, a], beta, gamma, r)
        assert t[2] == (a[2] + beta * b[2] + gamma) * (b[2] + beta * a[2] + gamma) % r
        assert ref.terms([a], None, beta, gamma, r) == [(x + gamma) % r for x in a]
        perm = list(a); rng.shuffle(perm)                       # a permutation closes, one changed element does not
        nz = [(x + gamma) % r for x in a]; dz = [(x + gamma) % r for x in perm]
        z, last = ref.grand_product(nz, dz, r)
        assert z[0] == 1 and last == 1 and all(z[i + 1] * dz[i] % r == z[i] * nz[i] % r for i in range(8))
        nz[3] = (nz[3] + 1) % r
        assert ref.grand_product(nz, dz, r)[1] != 1


def test_product_and_division_by_zh():
    rng = random.Random(23)
    for curve, r in ref.R.items():
        a = [rng.randrange(r) for _ in range(5)]; b = [rng.randrange(r) for _ in range(3)]
        c = ref.poly_mul(a, b, r)
        x = rng.randrange(r)
        assert len(c) == 7 and ref.poly_eval(c, x, r) == ref.poly_eval(a, x, r) * ref.poly_eval(b, x, r) % r
        assert ref.poly_mul(b, a, r) == c and ref.poly_mul([0], a, r) == [0] * 5
        for log_n in (0, 1, 3):
            N = 1 << log_n
            zh = [r - 1] + [0] * (N - 1) + [1]
            for n_p in (0, 1, N - 1, N, N + 1, 3 * N - 1, 4 * N):
                p = [rng.randrange(r) for _ in range(max(n_p, 0))]
                q, rem = ref.divmod_zh(p, log_n, r)
                assert len(q) == max(len(p) - N, 0) and len(rem) == N
                back = ref.poly_mul(q, zh, r) if q else []
                back = [(x + y) % r for x, y in zip(back + [0] * N, rem + [0] * len(back))][:max(len(p), N)]
                assert back[:len(p)] == p and not any(back[len(p):])            # q (X^N - 1) + rem == p
                assert rem == [sum(p[j::N]) % r for j in range(N)]                # the strided sums of the issue's definition
            q, rem = ref.divmod_zh(ref.poly_mul(a, zh, r), log_n, r)
            assert q == a and not any(rem)


def test_coset_factors():
    for curve, r in ref.R.items():
        f = ref.coset_factors(curve, 4, 2)
        w = ref.root_of_unity(curve, 4)
        assert len(f) == 16 and f[:4] == f[4:8] == f[12:]                        # m / N distinct factors
        for i in (0, 1, 5):
            x = 7 * pow(w, i, r) % r                                            # the i-th point of the coset 7 H_m
            assert f[i] * (pow(x, 4, r) - 1) % r == 1
        assert ref.coset_factors(curve, 3, 3) == [pow(pow(7, 8, r) - 1, -1, r)] * 8
        v = ref.mont_words([1, r - 1], r)
        assert ref.words_ints(v) == [(1 << 256) % r, (r - 1) * (1 << 256) % r]
