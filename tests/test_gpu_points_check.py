"""zk_points_check_* (csrc/key_check_impl.hip.h) against the plain-Python classification of tests/key_check_ref.py, per curve and
group, both forms (the endomorphism tests and [r]P = O bit by bit) on every input with equal output: subgroup points, curve points
outside the subgroup, points of exact small prime order l for every prime l < 2^32 that divides the cofactor (where a test that is
only "true on random points" goes wrong), points off the curve, coordinates q and q + 1, infinity; counts and first indices across a
wave boundary and a ragged tail."""
import importlib, math, pathlib, random, sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
import key_check_ref as K  # noqa: E402
CASES = [(cv, tag, g) for cv, tag in (("bn254", "BN128"), ("bls12_381", "BLS12381")) for g in (0, 1)]


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def dev(zk):
    return importlib.import_module("eigen_zkvm_amd.groth16")


@pytest.fixture(scope="module")
def g16(orc):
    return {cv: G.Groth16Oracle(orc, cv) for cv in ("bn254", "bls12_381")}


def _is_prime(n):
    if n < 2: return False
    for p in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % p == 0: return n == p
    d, s = n - 1, 0
    while d % 2 == 0: d //= 2; s += 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, n)
        if x in (1, n - 1): continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1: break
        else: return False
    return True


def small_prime_factors(h):
    """every prime below 2^32 that divides h: trial division to 2^16, then Pollard's rho on what is left (a factor below 2^32 shows
    after about 2^16 steps; the budget is 2^17 per start)"""
    out, m = [], h
    for p in range(2, 1 << 16):
        if m % p == 0:
            out.append(p)
            while m % p == 0: m //= p
    for c in (1, 3):
        while m > 1 and not _is_prime(m):
            x = y = 2; d = 1
            for _ in range(1 << 17):
                x = (x * x + c) % m; y = (y * y + c) % m; y = (y * y + c) % m
                d = math.gcd(abs(x - y), m)
                if d != 1: break
            if d in (1, m) or not _is_prime(d) or d >= 1 << 32: break
            out.append(d)
            while m % d == 0: m //= d
    if 1 < m < 1 << 32 and _is_prime(m): out.append(m)
    return sorted(out)


_POOL = {}


def pool(g16, cv, tag, g):
    """-> (ok rows, [(row, class)]) of Montgomery u64 word rows, made once per curve and group"""
    if (tag, g) in _POOL: return _POOL[(tag, g)]
    C, o = K.CURVES[tag], g16[cv]
    nl = o.nl
    row = lambda coords: np.concatenate([o.fq_mont_words(c) for c in coords])
    raw = lambda coords: np.concatenate([np.array(G._words(c, nl), np.uint64) for c in coords])   # words as they are: no reduction
    Gen = C.gen[g]
    good = [Gen, C.neg(Gen), C.mul(Gen, 2), C.mul(Gen, C.r - 1), C.mul(Gen, 0xdeadbeefcafe)]
    ok = [row(C.coords(p, g)) for p in good]
    for p in good: assert C.classify(C.coords(p, g), g) is None
    bad, rng = [], random.Random(7 + g)
    curve_pts, x = [], 1
    while len(curve_pts) < 4:                                                # the curve equation at small x, nothing cleared
        p = C.lift_x((x, 1 if g else 0), g); x += 1
        if p: curve_pts.append(p)
    for p in curve_pts: bad.append((row(C.coords(p, g)), C.classify(C.coords(p, g), g)))
    primes = small_prime_factors(C.cofactor[g])
    if tag == "BLS12381": assert {3, 11, 10177, 859267, 52437899}.issubset(primes) if g == 0 else {13, 23, 2713, 11953, 262069}.issubset(primes)
    if tag == "BN128" and g == 1: assert {10069, 5864401}.issubset(primes)
    for l in primes:
        xx, t = 1, None
        m = C.order(g)
        while m % l == 0: m //= l                                            # (l^2 divides some cofactors, and the l-part need not be cyclic)
        while t is None and xx < 200:                                        # a curve point with an l-part, brought down to order exactly l
            p = C.lift_x((xx, 1 if g else 0), g); xx += 1
            if p: t = C.mul(p, m)
        while t is not None and C.mul(t, l) is not None: t = C.mul(t, l)
        assert t is not None and C.mul(t, l) is None
        bad.append((row(C.coords(t, g)), "not_in_subgroup"))
    nc = 4 if g else 2
    off = list(C.coords(Gen, g)); off[-1] = (off[-1] + 1) % C.q
    bad.append((row(off), "not_on_curve"))
    bad.append((row([5] * nc), C.classify(tuple([5] * nc), g)))
    for v in (C.q, C.q + 1):
        for k in (0, nc - 1):
            c = [int(w) for w in C.coords(Gen, g)]
            r_ = row(c).reshape(nc, nl).copy(); r_[k] = raw([v])
            bad.append((r_.reshape(-1), "coordinate_range"))
    bad.append((np.zeros(nc * nl, np.uint64), "infinity"))
    if tag == "BN128" and g == 0: assert all(k != "not_in_subgroup" for _, k in bad)
    _POOL[(tag, g)] = (ok, bad)
    return ok, bad


def expect(classes):
    out = {k: [0, None] for k in K.CLASSES}
    for i, k in enumerate(classes):
        if k:
            out[k][0] += 1
            if out[k][1] is None: out[k][1] = i
    return {k: tuple(v) for k, v in out.items()}


def both(dev, rows, tag, g):
    a = np.concatenate(rows) if rows else np.zeros(0, np.uint64)
    endo = dev.points_check(a, tag, "g2" if g else "g1", plain=False)
    plain = dev.points_check(a, tag, "g2" if g else "g1", plain=True)
    assert endo == plain
    return endo


@pytest.mark.parametrize("cv,tag,g", CASES)
def test_every_input_one_by_one_and_together(dev, g16, cv, tag, g):
    ok, bad = pool(g16, cv, tag, g)
    for r_ in ok: assert both(dev, [r_], tag, g) == expect([None])          # n = 1
    for r_, k in bad: assert both(dev, [r_], tag, g) == expect([k]), k
    rows = ok + [r_ for r_, _ in bad]
    assert both(dev, rows, tag, g) == expect([None] * len(ok) + [k for _, k in bad])
    assert both(dev, [], tag, g) == expect([])                              # n = 0: nothing to do


@pytest.mark.parametrize("cv,tag,g", CASES)
def test_counts_and_first_indices_across_a_wave_boundary_and_a_tail(zk, dev, g16, cv, tag, g):
    ok, bad = pool(g16, cv, tag, g)
    n = 131
    by = {}
    for r_, k in bad:
        if k: by.setdefault(k, r_)
    kinds = [k for k in K.CLASSES if k in by]
    for pos in ([0], [63], [64], [n - 1], [63, 64], [0, 63, 64, n - 1], [1, 62, 65, 129]):
        rows = [ok[i % len(ok)] for i in range(n)]; cls = [None] * n
        for j, p in enumerate(pos):
            k = kinds[(j + len(pos)) % len(kinds)]; rows[p] = by[k]; cls[p] = k
        assert both(dev, rows, tag, g) == expect(cls), pos
    for k in kinds:                                                        # one class everywhere in the last wave and a half
        rows = [ok[0]] * 40 + [by[k]] * (n - 40)
        assert both(dev, rows, tag, g) == expect([None] * 40 + [k] * (n - 40))
    d = zk.DevArray.from_host(np.concatenate([ok[0]] * 64 + [by[kinds[-1]]]))   # the device form
    assert dev.points_check(d, tag, "g2" if g else "g1") == expect([None] * 64 + [kinds[-1]])
