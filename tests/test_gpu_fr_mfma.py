"""The matrix-pipe form of the scalar-field Poseidon (csrc/fr_mfma.hip.h: mf_dense, mf_sparse, and poseidon_fr_reg around them) on chosen
states, for BN128 and BLS12-381 and every t = 3..17, through the probes of csrc/frhash_probe_impl.hip.h.  States go in and come back as
raw internal limbs, so the test chooses the exact representative: every word any value below 2^256 -- byte patterns 0x00 / 0x7F / 0x80 /
0xFF, values around r and 2r, 2^k +- 1 at the limb and word seams, one hot word, the drivers of single digit columns, a word that makes
the carry chain of mf_reduce_words wrap (tests/fr_mfma_model.py: directed) -- in the first half of a batch, seeded random words in the
second.  Lanes l and l + 32, which trade halves through permlane32_swap, never hold the same state.  Every batch runs with 256 states
(one block) and with 293 (a second, ragged block whose idle lanes shadow the last state).

The reference is the integer model of tests/fr_mfma_model.py, validated without a GPU by tests/test_fr_mfma_model.py.  Dense layers and
sparse rounds: every raw limb equal to the model's; on top of that, stated on their own, the documented bounds (below 2r; below
2^242 + r with limbs normalised) and congruence to plain modular arithmetic.  The whole permutation: congruent mod r to the model's
plain permutation, which the oracle pins.  No tolerance anywhere."""
import ctypes as C
import numpy as np
import pytest

import fr_mfma_model as mm

pytestmark = pytest.mark.gpu
FIELDS = ["bn128", "bls12381"]
TS = list(range(3, 18))
N_FULL, N_BLOCK = 256 + 37, 256
MFP_DENSE, MFP_SPARSE, MFP_PERM = range(3)
N_EXACT_RANDOM = 64        # random states whose full sparse rounds the model replays, beside every directed one: the ragged block and part of the first


@pytest.fixture(scope="module")
def dev(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible: the HIP path cannot run (no CPU fallback)"
    zk.init(0)
    for field in FIELDS:
        zk.bn128_init(field=field)
    return zk


def _probe(dev, field):
    fn = getattr(dev.lib(), "zk_%s_mf_probe" % field)
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    return fn


def _run(dev, field, kind, t, arg, L):
    """L: (n, t, NR) uint32 limbs -> the same shape"""
    L = np.ascontiguousarray(L)
    out = np.full(L.shape, 0xA5A5A5A5, np.uint32)
    rc = _probe(dev, field)(kind, t, arg, L.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), L.shape[0])
    assert rc == 0, dev.lib().zk_last_error()
    return out


def _both_sizes(dev, field, kind, t, arg, L):
    """the batch of N_FULL states and its first N_BLOCK alone: the same results for the states they share"""
    full = _run(dev, field, kind, t, arg, L)
    block = _run(dev, field, kind, t, arg, L[:N_BLOCK])
    assert np.array_equal(block, full[:N_BLOCK]), f"{field} t = {t}: a state's result depends on the size of the batch"
    return full


def _same_limbs(got, want, what, rows=None):
    """got, want: (n, t, NR) limbs; rows: the state indices `want` holds (all of them if None)"""
    rows = np.arange(got.shape[0]) if rows is None else np.asarray(rows)
    bad = np.argwhere(got[rows] != want)
    if len(bad):
        k, j, _ = bad[0]
        i = int(rows[k])
        raise AssertionError(f"{what}: {len(set(map(tuple, bad[:, :2])))} words differ from the model; first: state {i} (lane {i % 64} of wave {i // 64}), "
                             f"output word {j}: got {[hex(int(x)) for x in got[i, j]]}, want {[hex(int(x)) for x in want[k, j]]}")


def _congruent(vals, want, r, what):
    bad = np.argwhere((vals - want) % r != 0)
    if len(bad):
        i, j = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words not congruent mod r; first: state {i} (lane {i % 64}), output word {j}: got {int(vals[i, j]):#x}, "
                             f"want {int(want[i, j]):#x} mod r")


def _normalised(L):
    return bool((L[..., :-1] < (1 << mm.LB)).all())


@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("field", FIELDS)
def test_dense_layers_match_the_model(dev, field, t):
    """mf_dense once, with the matrix and addends of layer 0 (M, the round constants' image), 3 (P) and 7 (M, no image)"""
    m = mm.model(field, t)
    X = mm.states(field, t, N_FULL)
    L = m.limbs(X)
    for layer in (0, 3, 7):
        what = f"{field} t = {t} dense layer {layer}"
        got = _both_sizes(dev, field, MFP_DENSE, t, layer, L)
        want = m.dense(layer, X)
        _same_limbs(got, m.limbs(want), what)
        vals = m.values(got)
        assert np.all(vals < 2 * m.r) and _normalised(got), f"{what}: a result reaches 2r or is not normalised"
        _congruent(vals, m.plain_dense(layer, X), m.r, what)


@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("field", FIELDS)
def test_sparse_rounds_one_and_two_match_the_model(dev, field, t):
    """mf_sparse with one round and with two (the two parities of the LDS double buffer): every state, every limb"""
    m = mm.model(field, t)
    X = mm.states(field, t, N_FULL)
    L = m.limbs(X)
    for n_rounds in (1, 2):
        what = f"{field} t = {t} sparse rounds 0..{n_rounds - 1}"
        got = _both_sizes(dev, field, MFP_SPARSE, t, n_rounds, L)
        want, wrapped = m.sparse(n_rounds, X)
        assert wrapped.any(), f"{what}: no state makes lo[q] + c of mf_reduce_words wrap"
        _same_limbs(got, m.limbs(want), what)
        vals = m.values(got)
        assert np.all(vals < (1 << 242) + m.r) and _normalised(got), f"{what}: a result reaches 2^242 + r or is not normalised"
        _congruent(vals, m.plain_sparse(n_rounds, X), m.r, what)


@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("field", FIELDS)
def test_all_sparse_rounds_match_the_model(dev, field, t):
    """mf_sparse with all fh_nrp(t) rounds: every state congruent to the plain rounds and within the documented bound; raw limbs equal to
    the model on every directed state and a few random ones"""
    m = mm.model(field, t)
    X = mm.states(field, t, N_FULL)
    what = f"{field} t = {t} sparse rounds 0..{m.n_rp - 1}"
    got = _both_sizes(dev, field, MFP_SPARSE, t, m.n_rp, m.limbs(X))
    vals = m.values(got)
    assert np.all(vals < (1 << 242) + m.r) and _normalised(got), f"{what}: a result reaches 2^242 + r or is not normalised"
    _congruent(vals, m.plain_sparse(m.n_rp, X), m.r, what)
    n_dir = len(mm.directed(field, t))
    rows = list(range(n_dir)) + list(range(N_FULL - N_EXACT_RANDOM, N_FULL))
    assert n_dir >= 8 and n_dir <= N_FULL // 2
    want, wrapped = m.sparse(m.n_rp, X[rows])
    assert wrapped.any(), f"{what}: no replayed state makes lo[q] + c of mf_reduce_words wrap"
    _same_limbs(got, m.limbs(want), what, rows)


@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("field", FIELDS)
def test_permutation_matches_the_plain_permutation(dev, field, t):
    """poseidon_fr_reg under the production register budget, on internal-form words up to its entry bound (below 2r)"""
    m = mm.model(field, t)
    X = mm.permutation_inputs(field, t, N_FULL)
    assert np.all(X < 2 * m.r)
    got = _both_sizes(dev, field, MFP_PERM, t, 0, m.limbs(X))
    rinv = pow(m.Rp, -1, m.r)
    want = m.permutation(X * rinv % m.r) * m.Rp % m.r
    _congruent(m.values(got), want, m.r, f"{field} t = {t} permutation")


@pytest.mark.parametrize("field", FIELDS)
def test_probe_names_bad_arguments(dev, field):
    fn = _probe(dev, field)
    buf = np.zeros((1, 17, mm.NR), np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    for args, word in (((MFP_DENSE, 2, 0, p, p, 1), b"t must be"), ((MFP_DENSE, 18, 0, p, p, 1), b"t must be"), ((MFP_DENSE, 5, 8, p, p, 1), b"layer must be"),
                       ((MFP_SPARSE, 5, 0, p, p, 1), b"rounds must be"), ((MFP_SPARSE, 5, mm.n_rp(field, 5) + 1, p, p, 1), b"rounds must be"),
                       ((3, 5, 0, p, p, 1), b"no such probe"), ((MFP_PERM, 5, 0, p, p, 0), b"n must be"), ((MFP_PERM, 5, 0, None, p, 1), b"null")):
        assert fn(*args) != 0 and word in dev.lib().zk_last_error(), args[:3]
