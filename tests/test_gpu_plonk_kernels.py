"""The three kernels of the PLONK prover (csrc/plonk_impl.hip.h) word for word against Python integers: the fused numerator
of the quotient at log_n = 3 and 5 (32 and 128 coset points), the row-by-row gate check with its exact count, the gather.  An input element is
the 256-bit integer its words are (any value below 2^256, not only below r) and stands for words / 2^256 mod r; every output word vector must
be the canonical Montgomery representative.  Exact: no tolerance anywhere."""
import importlib, random

import numpy as np
import pytest

import plonk_ref as ref

pytestmark = pytest.mark.gpu
CURVES = ("BN128", "BLS12381")
NAMES = ("a", "b", "c", "Z", "qL", "qR", "qO", "qM", "qC", "S1", "S2", "S3", "PI", "L1", "X")      # the order of zk_plonk_<curve>_quotient_dev


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def _dev(zk, words):
    """integers below 2^256, taken as the words themselves"""
    a = np.frombuffer(b"".join(w.to_bytes(32, "little") for w in words), dtype="<u8").astype(np.uint64)
    return zk.DevArray.from_host(a)


def _host(d, n):
    b = d.to_host()[:4 * n].astype("<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def _want_quotient(r, cols, m, alpha, beta, gamma, k1, k2):
    """the bracket at every index from the columns' words, as Montgomery words"""
    rinv = pow(1 << 256, -1, r)
    val = {k: [w * rinv % r for w in cols[k]] for k in NAMES}
    out = []
    for i in range(m):
        v = {k: val[k][i] for k in NAMES}
        v["Zw"] = val["Z"][(i + 4) % m]
        out.append((ref.bracket(r, v, v["X"], v["PI"], v["L1"], beta, gamma, alpha, k1, k2) << 256) % r)
    return out


def _run_quotient(zk, plonk, cv, log_n, cols, alpha, beta, gamma, k1, k2):
    m = 4 << log_n
    ds = [_dev(zk, cols[k]) for k in NAMES]
    try:
        out = plonk.quotient(ds, log_n, alpha, beta, gamma, k1, k2, cv)
        try:
            return _host(out, m)
        finally:
            out.free()
    finally:
        for d in ds:
            d.free()


@pytest.mark.parametrize("log_n", (3, 5))
@pytest.mark.parametrize("cv", CURVES)
def test_quotient_word_for_word(zk, plonk, cv, log_n):
    r, m, rng = ref.R[cv], 4 << log_n, random.Random(0x710 + log_n + len(cv))
    mont = lambda v: (v << 256) % r
    rand = lambda: {k: [mont(rng.randrange(r)) for _ in range(m)] for k in NAMES}
    const = lambda w: {k: [w] * m for k in NAMES}
    wide = {k: [rng.randrange(r, 1 << 256) for _ in range(m)] for k in NAMES}             # words >= r but < 2^256
    for k in NAMES:
        wide[k][0], wide[k][1], wide[k][m - 1] = (1 << 256) - 1, r, (1 << 256) - 1
    # Z alone distinct at the wrap: indices 4n - 4 .. 4n - 1 read Z at 0 .. 3
    wrap = const(mont(1))
    wrap["Z"] = [mont(i + 2) for i in range(m)]
    sc = lambda: [rng.randrange(r) for _ in range(3)]
    big = (rng.randrange(4, r), rng.randrange(4, r))
    cases = [("random, k = 2, 3", rand(), sc(), (2, 3)),
             ("random, large k", rand(), sc(), big),
             ("random, k = 1, 4 (the last by additions, the first by a product)", rand(), sc(), (1, 4)),
             ("random, k = 3, 0", rand(), sc(), (3, 0)),
             ("all zero", const(0), sc(), (2, 3)),
             ("all r - 1", const(mont(r - 1)), sc(), (2, 3)),
             ("all r - 1, every scalar r - 1", const(mont(r - 1)), [r - 1] * 3, (r - 1, r - 1)),
             ("words >= r", wide, sc(), (2, 3)),
             ("words >= r, large k, scalars r - 1", wide, [r - 1] * 3, big),
             ("the wrap of Z(wX)", wrap, sc(), (2, 3))]
    base = rand()
    for name, at in (("alpha = 0", 0), ("beta = 0", 1), ("gamma = 0", 2)):
        s = sc()
        s[at] = 0
        cases.append((name, base, s, (2, 3)))
    cases.append(("alpha = beta = gamma = 0", base, [0, 0, 0], (2, 3)))
    for name, cols, (alpha, beta, gamma), (k1, k2) in cases:
        got = _run_quotient(zk, plonk, cv, log_n, cols, alpha, beta, gamma, k1, k2)
        want = _want_quotient(r, cols, m, alpha, beta, gamma, k1, k2)
        assert all(w < r for w in got), name                                               # canonical
        assert got[m - 4:] == want[m - 4:], name                                           # the wrap
        assert got == want, name


@pytest.mark.parametrize("cv", CURVES)
def test_quotient_refusals(zk, plonk, cv):
    r = ref.R[cv]
    cols = [_dev(zk, [0] * 32) for _ in range(15)]
    try:
        with pytest.raises(plonk.ZkError, match="the output overlaps column 7"):
            plonk.quotient(cols, 3, 1, 2, 3, 2, 3, cv, out=cols[7])
        with pytest.raises(plonk.ZkError, match="beta is not below"):
            plonk.quotient(cols, 3, 1, r, 3, 2, 3, cv)
        with pytest.raises(plonk.ZkError, match="every column of the quotient holds 4n = 64"):
            plonk.quotient(cols, 4, 1, 2, 3, 2, 3, cv)
        with pytest.raises(plonk.ZkError, match="takes 15 columns"):
            plonk.quotient(cols[:14], 3, 1, 2, 3, 2, 3, cv)
    finally:
        for d in cols:
            d.free()


def _gate_rows(r, n, rng):
    """n rows that satisfy the gate equation, as values per column in the order a, b, c, qL, qR, qO, qM, qC, PI"""
    rows = []
    for _ in range(n):
        a, b, ql, qr, qm, qc, pi = (rng.randrange(r) for _ in range(7))
        c = rng.randrange(1, r)
        qo = -(ql * a + qr * b + qm * a * b + qc + pi) * pow(c, -1, r) % r
        rows.append((a, b, c, ql, qr, qo, qm, qc, pi))
    return rows


@pytest.mark.parametrize("cv", CURVES)
def test_gate_check_counts_exactly(zk, plonk, cv):
    r, n, rng = ref.R[cv], 600, random.Random(0x720 + len(cv))                             # three workgroups of 256 lanes, the last partly filled
    rows = _gate_rows(r, n, rng)
    mont = lambda v: (v << 256) % r

    def run(rows):
        ds = [_dev(zk, [mont(row[j]) for row in rows]) for j in range(9)]
        try:
            return plonk.gate_check(ds, len(rows), cv)
        finally:
            for d in ds:
                d.free()

    def broken(at):
        out = list(rows)
        for i in at:
            out[i] = out[i][:7] + ((out[i][7] + 1) % r,) + out[i][8:]
        return out
    assert run(rows) == (0, None)
    for at in ([0], [n - 1], [255], [256], [255, 256], [511, 512, 513], [n - 1, 0, 300]):
        assert run(broken(at)) == (len(at), min(at)), at
    assert run(broken(range(n))) == (n, 0)
    assert run(rows[:1]) == (0, None) and run(broken([0])[:1]) == (1, 0)
    # the largest representative below 2^256 of every word of satisfied rows: still satisfied
    lift = lambda w: w + r * (((1 << 256) - 1 - w) // r)
    ds = [_dev(zk, [lift(mont(row[j])) for row in rows[:300]]) for j in range(9)]
    try:
        assert plonk.gate_check(ds, 300, cv) == (0, None)
    finally:
        for d in ds:
            d.free()


@pytest.mark.parametrize("cv", CURVES)
def test_gather(zk, plonk, cv):
    r, rng = ref.R[cv], random.Random(0x730 + len(cv))
    m = 700
    src_words = [rng.randrange(1 << 256) for _ in range(m)]                                # a gather copies words, whatever they are
    src = _dev(zk, src_words)
    try:
        idx = [0, m - 1, 5, 5, 5, m - 1, 0] + [rng.randrange(m) for _ in range(520)]       # repeats, index 0 and the last; three workgroups
        out = plonk.gather(src, idx, cv)
        try:
            assert _host(out, len(idx)) == [src_words[i] for i in idx]
        finally:
            out.free()
        one = plonk.gather(src, [m - 1], cv)
        assert _host(one, 1) == [src_words[m - 1]]
        one.free()
        with pytest.raises(plonk.ZkError, match="index %d at position 3 is not below the source's %d elements" % (m, m)):
            plonk.gather(src, [0, 1, 2, m], cv)                                            # the host has the indices: refused there
        bad = list(idx)
        bad[2], bad[300], bad[519] = m, 0xFFFFFFFF, m + 7
        d_idx = plonk.upload_indices(np.asarray(bad, dtype=np.int64))
        d_out = zk.DevArray(4 * len(bad))
        try:
            with pytest.raises(plonk.ZkError, match="gather: 3 indices are not below the source's %d elements, the first at position 2" % m):
                plonk.gather_dev(src, d_idx, len(bad), cv, out=d_out)                      # only the device has them: counted there
            got = _host(d_out, len(bad))
            assert got == [0 if i in (2, 300, 519) else src_words[j] for i, j in enumerate(bad)]
        finally:
            d_idx.free(); d_out.free()
    finally:
        src.free()
