"""The kernels of PLONK's lookup argument (csrc/plonk_lookup_impl.hip.h) word for word against Python integers, over both
fields: the running sum, the hash table with the count of multiplicities, the denominators, the summand and the quotient's term.  An input
element is the 256-bit integer its words are (any value below 2^256, not only below r) and stands for words / 2^256 mod r; every output word
vector must be the canonical Montgomery representative.  Exact: no tolerance anywhere."""
import importlib, random

import numpy as np
import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")
TOP = (1 << 256) - 1


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


@pytest.fixture(scope="module")
def frpoly(zk):
    return importlib.import_module("eigen_zkvm_amd.frpoly")


def _dev(zk, words):
    """integers below 2^256, taken as the words themselves"""
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype="<u8").astype(np.uint64)
    return zk.DevArray.from_host(a if a.size else np.zeros(4, np.uint64))


def _host(d, n):
    b = d.to_host()[:4 * n].astype("<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


# ---- the running sum ------------------------------------------------------------------------------------------------------------------------
_SUMS = {}


def _sum_case(cv, n):
    """(the words, their inclusive running sums mod r), made once per (field, n): the words of element i stand for words / 2^256, so the
    Montgomery words of a sum are the sum of the words mod r"""
    if (cv, n) not in _SUMS:
        r = ref.R[cv]
        raw = np.random.default_rng(0x5a0 + n + len(cv)).integers(0, 1 << 63, size=4 * n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        b = raw.astype("<u8").tobytes()
        words = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
        for i, w in ((0, TOP), (n - 1, TOP), (n // 2, r), (n // 3, r - 1)):
            if n:
                words[i] = w
        incl, acc = [], 0
        for w in words:
            acc = (acc + w) % r
            incl.append(acc)
        _SUMS[(cv, n)] = (words, incl)
    return _SUMS[(cv, n)]


@pytest.mark.parametrize("n", (0, 1, 7, 2048, 2049, 4097, 2048 * 512 + 3))
@pytest.mark.parametrize("cv", CURVES)
def test_prefix_sum_word_for_word(zk, frpoly, cv, n):
    r = ref.R[cv]
    rinv = pow(1 << 256, -1, r)
    words, incl = _sum_case(cv, n)
    total = (incl[-1] if n else 0) * rinv % r
    if n == 0:
        assert frpoly.prefix_sum([], cv) == ([], 0) and frpoly.prefix_sum([], cv, inclusive=True, total_only=True) == (None, 0)
        return
    d = _dev(zk, words)
    try:
        assert frpoly.prefix_sum(d, cv, total_only=True) == (None, total)                  # the total alone: nothing is written
        out, tot = frpoly.prefix_sum(d, cv, inclusive=True)
        assert tot == total and _host(out, n) == incl
        out.free()
        same, tot = frpoly.prefix_sum(d, cv, out=d)                                        # exclusive, in place
        assert same is d and tot == total and _host(d, n) == [0] + incl[:-1]
    finally:
        d.free()


@pytest.mark.parametrize("cv", CURVES)
def test_prefix_sum_edge_operands(zk, frpoly, cv):
    r = ref.R[cv]
    rinv = pow(1 << 256, -1, r)
    for n in (9, 2049, 4100):
        for w in (TOP, (r - 1 << 256) % r, 0, r):                                          # every operand 2^256 - 1; every value r - 1; zero as 0 and as r
            d = _dev(zk, [w] * n)
            out, tot = frpoly.prefix_sum(d, cv, inclusive=True)
            assert _host(out, n) == [(i + 1) * w % r for i in range(n)] and tot == n * w * rinv % r
            out.free(); d.free()
    assert frpoly.prefix_sum([r - 1, r - 1, 1, 5], cv) == ([0, r - 1, r - 2, r - 1], 4)   # integers in, integers out


# ---- the hash table and the count -----------------------------------------------------------------------------------------------------------
def _hash(r, row):
    """the header's hash of a row of three VALUES: FNV-1a over the 24 u32 words of the canonical Montgomery representatives"""
    h = 0x811c9dc5
    for v in row:
        w = (v << 256) % r
        for j in range(8):
            h = ((h ^ ((w >> (32 * j)) & 0xffffffff)) * 0x01000193) & 0xffffffff
    return h ^ (h >> 16)


def _count(zk, pl, cv, table, rows, sel, enc=lambda i, j, w: w):
    """table: rows of three values; rows: n tuples of three values; sel: n selector values -> (m as words, bad, first) from the device.
    enc(i, j, w) may re-encode word w of column j of row i (w + r where that fits)"""
    r = ref.R[cv]
    mont = lambda v: (v << 256) % r
    n = len(rows)
    t = [_dev(zk, [mont(row[j]) for row in table]) for j in range(3)]
    cols = [_dev(zk, [enc(i, j, mont(row[j])) for i, row in enumerate(rows)]) for j in range(3)]
    qk = _dev(zk, [mont(s) for s in sel])
    tab = pl.LookupTable(*t, len(table), cv)
    for d in t:                                                                            # the handle keeps nothing of the columns
        d.free()
    try:
        m, bad, first = pl.count(tab, *cols, qk, n)
        try:
            return _host(m, n), bad, first
        finally:
            m.free()
    finally:
        tab.free(); qk.free()
        for d in cols:
            d.free()


def _want_count(r, table, rows, sel):
    first_of = {}
    for j, row in enumerate(table):
        first_of.setdefault(tuple(v % r for v in row), j)
    m, bad = [0] * len(rows), []
    for i, (row, s) in enumerate(zip(rows, sel)):
        if s % r:
            j = first_of.get(tuple(v % r for v in row))
            if j is None:
                bad.append(i)
            else:
                m[j] += 1
    return [(c << 256) % r for c in m], len(bad), (bad[0] if bad else None)


@pytest.mark.parametrize("T", (1, 5, 2048, 2049))
@pytest.mark.parametrize("cv", CURVES)
def test_count_random_tables(zk, pl, cv, T):
    r, rng = ref.R[cv], random.Random(0x5b0 + T + len(cv))
    n = 4096 if T > 5 else 600
    table = [tuple(rng.randrange(r) for _ in range(3)) for _ in range(T)]
    rows = [table[rng.randrange(T)] for _ in range(n)]
    sel = [rng.randrange(2) for _ in range(n)]
    sel[0] = sel[n - 1] = 1
    assert _count(zk, pl, cv, table, rows, sel) == _want_count(r, table, rows, sel)
    # misses: exact count and first row, selected rows only
    broken = list(rows)
    at = sorted(rng.sample(range(n), 7)) + [n - 1]
    for i in at:
        broken[i] = (broken[i][0], broken[i][1], (broken[i][2] + 1) % r)
    want = _want_count(r, table, broken, sel)
    assert want[1] == sum(1 for i in set(at) if sel[i]) and want[1] >= 1
    assert _count(zk, pl, cv, table, broken, sel) == want
    # no row selected: nothing is looked up, not even the rows that would miss
    assert _count(zk, pl, cv, table, broken, [0] * n) == ([0] * n, 0, None)


@pytest.mark.parametrize("cv", CURVES)
def test_count_keys_and_encodings(zk, pl, cv):
    r = ref.R[cv]
    # keys that differ only in t3, only in the top word of t1; one row three times: the smallest index takes the count
    table = [(7, 8, 9), (7, 8, 10), (7 + (1 << 224), 8, 9), (3, 3, 3), (1, 2, 3), (3, 3, 3), (3, 3, 3), (0, 0, 0)]
    rows = [(7, 8, 10), (7, 8, 9), (7 + (1 << 224), 8, 9), (3, 3, 3), (3, 3, 3), (7, 8, 9), (0, 0, 0), (3, 3, 3), (7, 9, 8), (1, 2, 3)]
    sel = [1] * len(rows)
    got = _count(zk, pl, cv, table, rows, sel)
    assert got == _want_count(r, table, rows, sel)
    assert got[0][:8] == [(c << 256) % r for c in (2, 1, 1, 3, 1, 0, 0, 1)] and got[1:] == (1, 8)
    # one value stored as v and as v + r: the same key, in the table and in the rows
    lift = lambda i, j, w: w + r if w + r <= TOP and (i + j) % 2 == 0 else w
    assert _count(zk, pl, cv, table, rows, sel, enc=lift) == got
    mont = lambda v: (v << 256) % r
    small = [v for v in range(2000) if mont(v) + r <= TOP][:4]
    t = [_dev(zk, [mont(small[0]) + r, mont(small[1]), mont(small[0])]), _dev(zk, [mont(small[2])] * 3), _dev(zk, [mont(small[3]) + r, mont(small[3]), mont(small[3])])]
    cols = [_dev(zk, [mont(small[0]), mont(small[0]) + r, mont(small[1])] + [0] * 5), _dev(zk, [mont(small[2]) + r] * 3 + [0] * 5), _dev(zk, [mont(small[3])] * 3 + [0] * 5)]
    qk = _dev(zk, [mont(1), mont(1) + r if mont(1) + r <= TOP else mont(1), mont(1)] + [r, 0, 0, 0, 0])      # q_K = 0 written as r selects nothing
    tab = pl.LookupTable(*t, 3, cv)
    try:
        m, bad, first = pl.count(tab, *cols, qk, 8)
        assert (_host(m, 8), bad, first) == ([mont(2), mont(1)] + [0] * 6, 0, None)        # table rows 0 and 2 are one key: row 0 counts
        m.free()
    finally:
        tab.free(); qk.free()
        for d in t + cols:
            d.free()


@pytest.mark.parametrize("cv", CURVES)
def test_count_every_row_on_one_counter(zk, pl, cv):
    r, n = ref.R[cv], 4096
    table = [(v, 0, 0) for v in range(256)]                                                # a range table: the case the wave's combining is for
    for hot in (0, 200):
        got = _count(zk, pl, cv, table, [(hot, 0, 0)] * n, [1] * n)
        assert got == ([((n if j == hot else 0) << 256) % r for j in range(n)], 0, None)
    rows = [(i % 3, 0, 0) for i in range(n)]                                               # three counters inside every wave
    assert _count(zk, pl, cv, table, rows, [1] * n) == _want_count(r, table, rows, [1] * n)
    rows = [(i % 7 + 250, 0, 0) for i in range(n)]                                         # more counters than rounds of combining, one of them a miss
    assert _count(zk, pl, cv, table, rows, [1] * n) == _want_count(r, table, rows, [1] * n)


@pytest.mark.parametrize("cv", CURVES)
def test_count_probing_wraps(zk, pl, cv):
    """T = 5 gives 16 slots; rows chosen by the documented hash so that one starts at slot 14 and four at slot 15: they fill 14, 15, 0, 1, 2"""
    r = ref.R[cv]
    at15 = [v for v in range(1, 4000) if _hash(r, (v, 0, 0)) & 15 == 15][:4]
    at14 = [v for v in range(1, 4000) if _hash(r, (v, 0, 0)) & 15 == 14][:1]
    assert len(at15) == 4 and len(at14) == 1
    table = [(v, 0, 0) for v in at15[:2] + at14 + at15[2:]]
    absent = next(v for v in range(4000, 8000) if _hash(r, (v, 0, 0)) & 15 == 15)          # walks 15, 0, 1, 2 and ends on the empty slot 3
    rows = [(v, 0, 0) for v in at15 + at14 + at15[::-1] + [absent, at15[3]]]
    sel = [1] * len(rows)
    want = _want_count(r, table, rows, sel)
    assert want[1:] == (1, 9)
    assert _count(zk, pl, cv, table, rows, sel) == want


def test_table_refusals(zk, pl):
    d = _dev(zk, [1, 2, 3])
    try:
        with pytest.raises(pl.ZkError, match="at least one row"):
            pl.LookupTable(d, d, d, 0, "BN128")
        with pytest.raises(pl.ZkError, match="holds 4 elements"):
            pl.LookupTable(d, d, d, 4, "BN128")
        tab = pl.LookupTable(d, d, d, 3, "BN128")
        big = _dev(zk, [0, 0])
        with pytest.raises(pl.ZkError, match="the table has 3 rows, the multiplicities only 2"):
            pl.count(tab, big, big, big, big, 2)
        with pytest.raises(pl.ZkError, match="over another field"):
            zk._check(zk.lib().zk_plonk_bls12_381_lookup_count_dev(tab._h, big.ptr, big.ptr, big.ptr, big.ptr, 2, big.ptr, None, None, 0))
        tab.free(); big.free()
    finally:
        d.free()


# ---- the denominators, the summand, the quotient's term -------------------------------------------------------------------------------------
def _columns(r, rng, names, m, kind):
    if kind == "top":
        return {k: [TOP] * m for k in names}
    if kind == "wide":                                                                     # words >= r but < 2^256, the ends at the extremes
        cols = {k: [rng.randrange(r, 1 << 256) for _ in range(m)] for k in names}
        for k in names:
            cols[k][0], cols[k][1], cols[k][m - 1] = TOP, r, TOP
        return cols
    return {k: [(rng.randrange(r) << 256) % r for _ in range(m)] for k in names}


@pytest.mark.parametrize("log_n", (3, 5))
@pytest.mark.parametrize("cv", CURVES)
def test_terms_and_summands_word_for_word(zk, pl, cv, log_n):
    r, n, rng = ref.R[cv], 1 << log_n, random.Random(0x5c0 + log_n + len(cv))
    rinv = pow(1 << 256, -1, r)
    names = ("a", "b", "c", "t1", "t2", "t3")
    for kind, scalars in (("top", (r - 1, r - 1)), ("wide", (r - 1, rng.randrange(r))), ("random", (rng.randrange(r), rng.randrange(r))), ("random", (0, 0))):
        eta, delta = scalars
        cols = _columns(r, rng, names, n, kind)
        ds = [_dev(zk, cols[k]) for k in names]
        out = pl.terms(ds, n, eta, delta, cv)
        val = {k: [w * rinv % r for w in cols[k]] for k in names}
        want = [((delta + val[x][i] + eta * val[y][i] + eta * eta * val[z][i]) << 256) % r for x, y, z in (names[:3], names[3:]) for i in range(n)]
        assert _host(out, 2 * n) == want, kind
        out.free()
        for d in ds:
            d.free()
        sc = _columns(r, rng, ("inv0", "inv1", "qK", "m"), n, kind)
        inv, qk, m = _dev(zk, sc["inv0"] + sc["inv1"]), _dev(zk, sc["qK"]), _dev(zk, sc["m"])
        out = pl.summands(inv, qk, m, n, cv)
        want = [((sc["qK"][i] * sc["inv0"][i] - sc["m"][i] * sc["inv1"][i]) * rinv) % r for i in range(n)]
        assert _host(out, n) == want, kind
        for d in (inv, qk, m, out):
            d.free()


@pytest.mark.parametrize("log_n", (3, 5))
@pytest.mark.parametrize("cv", CURVES)
def test_lookup_quotient_word_for_word(zk, pl, cv, log_n):
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x5d0 + log_n + len(cv))
    rinv = pow(1 << 256, -1, r)
    names = ("a", "b", "c", "qK", "t1", "t2", "t3", "M", "Phi")
    wrap = {k: [(1 << 256) % r] * m for k in names}
    wrap["Phi"] = [((i + 2) << 256) % r for i in range(m)]                                  # Phi alone distinct at the wrap: 4n - 4 .. 4n - 1 read Phi at 0 .. 3
    cases = [("top", _columns(r, rng, names + ("acc",), m, "top"), (r - 1, r - 1, r - 1)),
             ("wide", _columns(r, rng, names + ("acc",), m, "wide"), (r - 1, rng.randrange(r), r - 1)),
             ("random", _columns(r, rng, names + ("acc",), m, "random"), tuple(rng.randrange(r) for _ in range(3))),
             ("alpha = 0", _columns(r, rng, names + ("acc",), m, "random"), (0, rng.randrange(r), rng.randrange(r))),
             ("wrap", dict(wrap, acc=[0] * m), tuple(rng.randrange(r) for _ in range(3)))]
    for kind, cols, (alpha, eta, delta) in cases:
        ds = [_dev(zk, cols[k]) for k in names]
        acc = _dev(zk, cols["acc"])
        assert pl.lookup_quotient(ds, log_n, alpha, eta, delta, acc, cv) is acc
        val = {k: [w * rinv % r for w in cols[k]] for k in names + ("acc",)}
        want = []
        for i in range(m):
            v = {"a": val["a"][i], "b": val["b"][i], "c": val["c"][i], "qK": val["qK"][i], "T1": val["t1"][i], "T2": val["t2"][i], "T3": val["t3"][i], "M": val["M"][i],
                 "Phi": val["Phi"][i], "Phiw": val["Phi"][(i + 4) % m]}
            want.append(((val["acc"][i] + pow(alpha, 3, r) * pl.lookup_term(cv, v, eta, delta)) << 256) % r)
        got = _host(acc, m)
        assert got[m - 4:] == want[m - 4:], kind
        assert got == want, kind
        for d in ds + [acc]:
            d.free()


def test_kernel_refusals(zk, pl):
    r = ref.R["BN128"]
    cols = [_dev(zk, [0] * 32) for _ in range(10)]
    try:
        with pytest.raises(pl.ZkError, match="the accumulator overlaps column 8"):
            pl.lookup_quotient(cols[:9], 3, 1, 2, 3, cols[8], "BN128")
        with pytest.raises(pl.ZkError, match="eta is not below"):
            pl.lookup_quotient(cols[:9], 3, 1, r, 3, cols[9], "BN128")
        with pytest.raises(pl.ZkError, match="every column of the quotient holds 4n = 64"):
            pl.lookup_quotient(cols[:9], 4, 1, 2, 3, cols[9], "BN128")
        with pytest.raises(pl.ZkError, match="takes 9 columns"):
            pl.lookup_quotient(cols[:8], 3, 1, 2, 3, cols[9], "BN128")
        with pytest.raises(pl.ZkError, match="take 6 columns"):
            pl.terms(cols[:5], 8, 1, 2, "BN128")
        with pytest.raises(pl.ZkError, match="delta is not below"):
            pl.terms(cols[:6], 8, 1, r, "BN128")
    finally:
        for d in cols:
            d.free()
