"""The kernels of the tagged lookups (csrc/plonk_lookup_tagged_impl.hip.h) word for word against Python integers: the hash
table over (T0, t1, t2, t3) with the weighted count, the four-column denominators and the quotient's term.  An input element is the 256-bit
integer its words are and stands for words / 2^256 mod r; every output word vector must be the canonical Montgomery representative.
Exact: no tolerance anywhere.  Shapes: n = 8 and 16 with every edge case (one tuple in two tables, a duplicate inside a table, a tuple of
the other table as a miss, unselected rows holding table tuples, padding rows, operands 0 and r - 1), n = 256 (more targets in a wave
than rounds of combining; a whole wave on one counter of tag 3), n = 4096 = T (two tiles of the running sum's size), BLS12-381 at n = 16,
and K = 65535 under a count that carries the product past 32 bits."""
import ctypes, importlib, random

import numpy as np
import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
TOP = (1 << 256) - 1


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


def _dev(zk, words):
    """integers below 2^256, taken as the words themselves"""
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype="<u8").astype(np.uint64)
    return zk.DevArray.from_host(a)


def _host(d, n):
    b = d.to_host()[:4 * n].astype("<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _count(zk, pl, cv, table, rows, enc=lambda i, j, w: w):
    """table: rows (tag, t1, t2, t3); rows: n tuples (qK, a, b, c) -> (m as words, bad, first) from the device"""
    r = ref.R[cv]
    mont = lambda v: (v << 256) % r
    t = [_dev(zk, [mont(row[j]) for row in table]) for j in range(4)]
    cols = [_dev(zk, [enc(i, j, mont(row[j])) for i, row in enumerate(rows)]) for j in range(4)]
    tab = pl.LookupTable(t[1], t[2], t[3], len(table), cv, tag=t[0])
    for d in t:
        d.free()
    try:
        assert tab.tagged
        m, bad, first = pl.count(tab, cols[1], cols[2], cols[3], cols[0], len(rows))
        try:
            return _host(m, len(rows)), bad, first
        finally:
            m.free()
    finally:
        tab.free()
        for d in cols:
            d.free()


def _want_count(r, table, rows):
    """m_j = tag_j x (the selected rows equal to tagged row j), the first index of a repeated tagged row taking all; the misses"""
    first_of = {}
    for j, row in enumerate(table):
        first_of.setdefault(tuple(v % r for v in row), j)
    m, bad = [0] * len(rows), []
    for i, row in enumerate(rows):
        if row[0] % r:
            j = first_of.get(tuple(v % r for v in row))
            if j is None:
                bad.append(i)
            else:
                m[j] += table[j][0]
    return [(c << 256) % r for c in m], len(bad), (bad[0] if bad else None)


def _edge_case(r, n):
    """the padded table and the n rows of the small cases"""
    table = [(1, 5, 0, 0), (1, 7, 0, 0), (2, 5, 0, 0), (2, r - 1, 0, r - 1), (2, 9, 9, 9), (2, 9, 9, 9), (3, 0, 0, 0)]
    table += [table[-1]] * (n - len(table))                                                # padding rows: the last row again, tag included
    rows = [(1, 5, 0, 0), (2, 5, 0, 0), (1, 5, 0, 0),                                      # one tuple in two tables: counted apart
            (2, 9, 9, 9),                                                                  # a duplicate inside table 2: row 4 takes it
            (1, 9, 9, 9),                                                                  # table 2's tuple under tag 1: a miss, row 4
            (0, 5, 0, 0),                                                                  # qK = 0 over a table tuple: not counted
            (3, 0, 0, 0),                                                                  # the padded row: the smallest index, 6, takes it
            (2, r - 1, 0, r - 1)]
    if n > 8:
        rows += [(3, 5, 0, 0), (0, 1, 2, 3), (2, 9, 9, 9), (3, 0, 0, 0), (1, 7, 0, 0), (2, 7, 0, 0), (0, 0, 0, 0), (2, r - 1, 0, r - 1)]    # two more misses: 8, 13
    return table, rows


@pytest.mark.parametrize("cv,n", (("BN128", 8), ("BN128", 16), ("BLS12381", 16)))
def test_count_edge_cases(zk, pl, cv, n):
    r = ref.R[cv]
    table, rows = _edge_case(r, n)
    want = _want_count(r, table, rows)
    mont = lambda v: (v << 256) % r
    if n == 8:
        assert want == ([mont(c) for c in (2, 0, 2, 2, 2, 0, 3, 0)], 1, 4)
    else:
        assert want[0][:7] == [mont(c) for c in (2, 1, 2, 4, 4, 0, 6)] and not any(want[0][7:]) and want[1:] == (3, 4)
    got = _count(zk, pl, cv, table, rows)
    assert got == want
    lift = lambda i, j, w: w + r if w + r <= TOP and (i + j) % 2 == 0 else w                # v and v + r are one key, the tag's words included
    assert _count(zk, pl, cv, table, rows, enc=lift) == want
    assert _count(zk, pl, cv, table, [(0,) + row[1:] for row in rows]) == ([0] * n, 0, None)   # nothing selected, nothing looked up


def test_count_a_crowded_wave_and_a_whole_wave_on_one_counter(zk, pl):
    cv, n = "BN128", 256
    r = ref.R[cv]
    table = [(1, v, 0, 0) for v in range(8)] + [(2, v, 0, 0) for v in range(8)] + [(3, 11, 0, 0), (3, 12, 0, 0)]
    table += [table[-1]] * (n - len(table))
    rows = [(1 + i % 2, i % 7, 0, 0) for i in range(64)]                                   # 14 counters in one wave: more than PL_ROUNDS = 4
    rows += [(3, 11, 0, 0)] * 64                                                           # 64 lanes on one counter of tag 3
    rows += [(1 + i % 3, 11 if i % 3 == 2 else i % 10, 0, 0) for i in range(64)]           # 8 and 9 are in neither table: misses among the crowd
    rows += [(0, i % 7, 0, 0) for i in range(64)]
    want = _want_count(r, table, rows)
    assert want[0][16] == ((3 * (64 + len([i for i in range(64) if i % 3 == 2]))) << 256) % r and want[1] > 0 and want[2] >= 128
    assert _count(zk, pl, cv, table, rows) == want
    alone = [(0, 0, 0, 0)] * 64 + rows[64:128] + [(0, 0, 0, 0)] * 128                      # that wave alone: m is 3 x 64
    got = _count(zk, pl, cv, table, alone)
    assert got == ([((3 * 64) << 256) % r if j == 16 else 0 for j in range(n)], 0, None)


def test_count_a_table_as_long_as_the_rows(zk, pl):
    cv, n = "BN128", 4096
    r, rng = ref.R[cv], random.Random(0x6a0)
    assert n == 2 * zk.lib().zk_frpoly_tile_elems()
    sizes = [1, 700, 2048, 1346, 1]                                                        # K = 5, T = n exactly: no padding row
    table = [(k + 1, rng.randrange(r), rng.randrange(1 << 16), j) for k, size in enumerate(sizes) for j in range(size)]
    assert len(table) == n
    rows = []
    for i in range(n):
        tag, a, b, c = table[rng.randrange(n)]
        kind = rng.randrange(8)
        rows.append((0, a, b, c) if kind == 0 else ((tag % 5) + 1, a, b, c) if kind == 1 else (tag, a, b, c))       # kind 1: the tuple under another table's tag
    rows[0], rows[n - 1] = table[n - 1], table[0]
    want = _want_count(r, table, rows)
    assert want[1] > 100
    assert _count(zk, pl, cv, table, rows) == want


def test_count_the_largest_tag_under_a_large_count(zk, pl):
    """K = 65535 tables of one row; 2^17 rows on the last: 65535 x 131072 is past 2^32, and fills limb 1 of the two the product has"""
    cv, K, n = "BN128", 65535, 1 << 17
    r = ref.R[cv]
    mont = lambda v: (v << 256) % r
    tags = np.frombuffer(b"".join(mont(k).to_bytes(32, "little") for k in range(1, K + 1)), dtype="<u8").astype(np.uint64)
    t1 = np.frombuffer(b"".join(mont(k * k).to_bytes(32, "little") for k in range(1, K + 1)), dtype="<u8").astype(np.uint64)
    zero = zk.DevArray.from_host(np.zeros(4 * n, np.uint64))
    d_tag, d_t1 = zk.DevArray.from_host(tags), zk.DevArray.from_host(t1)
    tab = pl.LookupTable(d_t1, zero, zero, K, cv, tag=d_tag)
    col = lambda v: zk.DevArray.from_host(np.tile(np.frombuffer(mont(v).to_bytes(32, "little"), dtype="<u8").astype(np.uint64), n))
    qk, a = col(K), col(K * K)
    try:
        m, bad, first = pl.count(tab, a, zero, zero, qk, n)
        got = _host(m, n)
        assert (bad, first) == (0, None) and K * n > 1 << 32
        assert got[K - 1] == mont(K * n) and not any(got[:K - 1]) and not any(got[K:])
        m.free()
    finally:
        tab.free()
        for d in (zero, d_tag, d_t1, qk, a):
            d.free()


def test_table_refusals(zk, pl):
    cv = "BN128"
    r = ref.R[cv]
    mont = lambda v: (v << 256) % r
    d = _dev(zk, [mont(1), mont(2), mont(3), mont(4)])
    try:
        for bad_tag, row in ((0, 2), (65536, 1), (r - 1, 3), (1 << 40, 0)):
            tags = [mont(1)] * 4
            tags[row] = mont(bad_tag)
            t = _dev(zk, tags)
            with pytest.raises(pl.ZkError, match=r"plonk lookup: the tag of table row %d is not in 1 \.\. 65535 \(1 such rows\)" % row):
                pl.LookupTable(d, d, d, 4, cv, tag=t)
            t.free()
        with pytest.raises(pl.ZkError, match="holds 5 elements"):
            pl.LookupTable(d, d, d, 5, cv, tag=d)
        tagged, plain = pl.LookupTable(d, d, d, 4, cv, tag=d), pl.LookupTable(d, d, d, 4, cv)
        lib = zk.lib()
        n_bad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
        with pytest.raises(pl.ZkError, match="the table has no tags"):
            zk._check(lib.zk_plonk_bn254_lookup_tagged_count_dev(plain._h, d.ptr, d.ptr, d.ptr, d.ptr, 4, d.ptr, ctypes.byref(n_bad), ctypes.byref(first), 0))
        with pytest.raises(pl.ZkError, match="the table is a tagged one"):
            zk._check(lib.zk_plonk_bn254_lookup_count_dev(tagged._h, d.ptr, d.ptr, d.ptr, d.ptr, 4, d.ptr, ctypes.byref(n_bad), ctypes.byref(first), 0))
        with pytest.raises(pl.ZkError, match="over another field"):
            zk._check(lib.zk_plonk_bls12_381_lookup_tagged_count_dev(tagged._h, d.ptr, d.ptr, d.ptr, d.ptr, 4, d.ptr, ctypes.byref(n_bad), ctypes.byref(first), 0))
        tagged.free(); plain.free()
    finally:
        d.free()


# ---- the denominators and the quotient's term -----------------------------------------------------------------------------------------------
def _columns(r, rng, names, m, kind):
    if kind == "top":
        return {k: [TOP] * m for k in names}
    if kind == "ends":                                                                     # the values 0 and r - 1, zero also written as r
        pool = [0, r, ((r - 1) << 256) % r]
        return {k: [pool[(i + j) % 3] for i in range(m)] for j, k in enumerate(names)}
    if kind == "wide":                                                                     # words >= r but < 2^256, the ends at the extremes
        cols = {k: [rng.randrange(r, 1 << 256) for _ in range(m)] for k in names}
        for k in names:
            cols[k][0], cols[k][1], cols[k][m - 1] = TOP, r, TOP
        return cols
    return {k: [(rng.randrange(r) << 256) % r for _ in range(m)] for k in names}


def _kinds(r, rng, log_n):
    if log_n > 4:
        return [("random", tuple(rng.randrange(r) for _ in range(3)))]
    return [("top", (r - 1, r - 1, r - 1)), ("ends", (r - 1, r - 1, r - 1)), ("ends", (0, 0, 0)), ("wide", (r - 1, rng.randrange(r), r - 1)),
            ("random", tuple(rng.randrange(r) for _ in range(3))), ("random", (0, rng.randrange(r), rng.randrange(r)))]


SHAPES = (("BN128", 3), ("BN128", 4), ("BN128", 8), ("BN128", 12), ("BLS12381", 4))


@pytest.mark.parametrize("cv,log_n", SHAPES)
def test_terms_word_for_word(zk, pl, cv, log_n):
    r, n, rng = ref.R[cv], 1 << log_n, random.Random(0x6c0 + log_n + len(cv))
    rinv = pow(1 << 256, -1, r)
    names = ("a", "b", "c", "qK", "t1", "t2", "t3", "T0")
    for kind, (_, eta, delta) in _kinds(r, rng, log_n):
        cols = _columns(r, rng, names, n, kind)
        ds = [_dev(zk, cols[k]) for k in names]
        out = pl.terms(ds, n, eta, delta, cv, tagged=True)
        val = {k: [w * rinv % r for w in cols[k]] for k in names}
        want = [((delta + val[x][i] + eta * val[y][i] + eta * eta * val[z][i] + eta ** 3 * val[w][i]) << 256) % r for x, y, z, w in (names[:4], names[4:]) for i in range(n)]
        assert _host(out, 2 * n) == want, kind
        out.free()
        for d in ds:
            d.free()


@pytest.mark.parametrize("cv,log_n", SHAPES)
def test_quotient_word_for_word(zk, pl, cv, log_n):
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x6d0 + log_n + len(cv))
    rinv = pow(1 << 256, -1, r)
    names = ("a", "b", "c", "qK", "t1", "t2", "t3", "T0", "M", "Phi")
    cases = [(kind, _columns(r, rng, names + ("acc",), m, kind), sc) for kind, sc in _kinds(r, rng, log_n)]
    wrap = {k: [(1 << 256) % r] * m for k in names}
    wrap["Phi"] = [((i + 2) << 256) % r for i in range(m)]                                  # Phi alone distinct at the wrap: 4n - 4 .. 4n - 1 read Phi at 0 .. 3
    cases.append(("wrap", dict(wrap, acc=[0] * m), tuple(rng.randrange(r) for _ in range(3))))
    for kind, cols, (alpha, eta, delta) in cases:
        ds = [_dev(zk, cols[k]) for k in names]
        acc = _dev(zk, cols["acc"])
        assert pl.lookup_quotient(ds, log_n, alpha, eta, delta, acc, cv, tagged=True) is acc
        val = {k: [w * rinv % r for w in cols[k]] for k in names + ("acc",)}
        a3, want = pow(alpha, 3, r), []
        for i in range(m):
            v = {"a": val["a"][i], "b": val["b"][i], "c": val["c"][i], "qK": val["qK"][i], "T1": val["t1"][i], "T2": val["t2"][i], "T3": val["t3"][i], "T0": val["T0"][i],
                 "M": val["M"][i], "Phi": val["Phi"][i], "Phiw": val["Phi"][(i + 4) % m]}
            f = delta + v["a"] + eta * v["b"] + eta * eta * v["c"] + eta ** 3 * v["qK"]
            t = delta + v["T1"] + eta * v["T2"] + eta * eta * v["T3"] + eta ** 3 * v["T0"]
            L = (v["Phiw"] - v["Phi"]) * f * t - v["qK"] * t + v["M"] * f
            assert L % r == pl.lookup_term(cv, v, eta, delta, tagged=True)                 # the package's host formula is the same one
            want.append(((val["acc"][i] + a3 * L) << 256) % r)
        got = _host(acc, m)
        assert got[m - 4:] == want[m - 4:], kind
        assert got == want, kind
        for d in ds + [acc]:
            d.free()


def test_kernel_refusals(zk, pl):
    r = ref.R["BN128"]
    cols = [_dev(zk, [0] * 32) for _ in range(11)]
    try:
        with pytest.raises(pl.ZkError, match="tagged quotient: the accumulator overlaps column 9"):
            pl.lookup_quotient(cols[:10], 3, 1, 2, 3, cols[9], "BN128", tagged=True)
        with pytest.raises(pl.ZkError, match="eta is not below"):
            pl.lookup_quotient(cols[:10], 3, 1, r, 3, cols[10], "BN128", tagged=True)
        with pytest.raises(pl.ZkError, match="every column of the quotient holds 4n = 64"):
            pl.lookup_quotient(cols[:10], 4, 1, 2, 3, cols[10], "BN128", tagged=True)
        with pytest.raises(pl.ZkError, match="takes 10 columns, not 9"):
            pl.lookup_quotient(cols[:9], 3, 1, 2, 3, cols[10], "BN128", tagged=True)
        with pytest.raises(pl.ZkError, match="take 8 columns, not 6"):
            pl.terms(cols[:6], 8, 1, 2, "BN128", tagged=True)
        with pytest.raises(pl.ZkError, match="delta is not below"):
            pl.terms(cols[:8], 8, 1, r, "BN128", tagged=True)
    finally:
        for d in cols:
            d.free()
