"""No GPU.  The integer model of the scalar-field Poseidon's matrix-pipe form (tests/fr_mfma_model.py) before a device is involved:
  * against the host emulation of csrc/fr_mfma.hip.h (mf_emulate / mf_emulate_gen on the tables mf_build builds from the constants file,
    through zk_<field>_mf_emulate_probe): the same 320-bit integer for every output of M with the constants' image (layer 0), P (layer
    3), M without an image (layer 7) and the first, second, middle and last sparse round, on every directed state, both fields, every
    t = 3..17, with the emulation's `ok` true throughout (every digit column below 2^23, every biased word inside (0, 2^49));
  * the model's plain permutation mod r against the oracle's digests for every t, and the known answers tests/test_gpu_bn128.py carries.
The model takes no table from the library: it reads the constants file itself."""
import ctypes as C
import numpy as np
import pytest

import fr_mfma_model as mm

FIELDS = ["bn128", "bls12381"]
TS = list(range(3, 18))


def _emulate(zk, field, t, which, X):
    fn = getattr(zk.lib(), "zk_%s_mf_emulate_probe" % field)
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    n = X.shape[0]
    raw = b"".join(int(v).to_bytes(32, "little") for v in X.reshape(-1))
    x = np.frombuffer(raw, np.uint32).copy()
    out = np.zeros((n, t, 11), np.uint32)
    path = str(mm.DATA / ("poseidon_%s_constants.bin" % field)).encode()
    assert fn(path, t, which, x.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)) == 0, zk.lib().zk_last_error()
    val = np.array([[int.from_bytes(out[i, o, :10].tobytes(), "little") for o in range(t)] for i in range(n)], dtype=object)
    return val, out[..., 10].astype(bool)


@pytest.mark.parametrize("t", TS)
@pytest.mark.parametrize("field", FIELDS)
def test_model_equals_the_host_emulation(zk, field, t):
    m = mm.model(field, t)
    pats = mm.directed(field, t)
    X = np.array(pats, dtype=object)
    assert X.shape == (len(pats), t)
    for layer in (0, 3, 7):
        got, ok = _emulate(zk, field, t, layer, X)
        want = m.dense(layer, X)
        assert ok.all(), f"{field} t = {t} layer {layer}: the host emulation reports an intermediate out of range"
        bad = np.argwhere(got != want)
        assert not len(bad), (f"{field} t = {t} layer {layer}: state {bad[0][0]} output {bad[0][1]}: emulation {int(got[tuple(bad[0])]):#x}, "
                              f"model {int(want[tuple(bad[0])]):#x}")
        assert np.all(want < 2 * m.r) and np.all((want - m.plain_dense(layer, X)) % m.r == 0)
    for rnd in (0, 1, m.n_rp // 2, m.n_rp - 1):
        got, ok = _emulate(zk, field, t, 8 + rnd, X)
        want, _ = m.sparse_linear(rnd, X)
        assert ok.all(), f"{field} t = {t} sparse round {rnd}: the host emulation reports an intermediate out of range"
        bad = np.argwhere(got != want)
        assert not len(bad), (f"{field} t = {t} sparse round {rnd}: state {bad[0][0]} output {bad[0][1]}: emulation {int(got[tuple(bad[0])]):#x}, "
                              f"model {int(want[tuple(bad[0])]):#x}")
        assert np.all(want < (1 << 242) + m.r)


@pytest.mark.parametrize("field", FIELDS)
def test_emulation_probe_names_bad_arguments(zk, field):
    fn = getattr(zk.lib(), "zk_%s_mf_emulate_probe" % field)
    fn.restype, fn.argtypes = C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    x = np.zeros(17 * 8, np.uint32); out = np.zeros(17 * 11, np.uint32)
    path = str(mm.DATA / ("poseidon_%s_constants.bin" % field)).encode()
    px, po = x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args, word in (((path, 2, 0, px, 1, po), b"t must be"), ((path, 18, 0, px, 1, po), b"t must be"), ((path, 5, 8 + mm.n_rp(field, 5), px, 1, po), b"no such layer"),
                       ((path, 5, -1, px, 1, po), b"no such layer"), ((path, 5, 0, px, 0, po), b"n must be"), ((None, 5, 0, px, 1, po), b"null"),
                       ((b"/nonexistent/constants.bin", 5, 0, px, 1, po), b"cannot open")):
        assert fn(*args) != 0 and word in zk.lib().zk_last_error(), args[1:3]


@pytest.mark.parametrize("field", FIELDS)
def test_model_permutation_matches_the_oracle(orc, field):
    """every t = 2..17: the whole state after the permutation, on an edge input and two random ones"""
    h = orc.bn128() if field == "bn128" else orc.bls12381()
    rng = np.random.default_rng(41 if field == "bn128" else 43)
    for t in range(2, 18):
        m = mm.model(field, t)
        assert h.R == m.r
        rows = [[0] * t, [m.r - 1] * t] + [[int.from_bytes(rng.bytes(40), "little") % m.r for _ in range(t)] for _ in range(2)]
        got = m.permutation(np.array(rows, dtype=object))
        for i, row in enumerate(rows):
            assert [int(v) for v in got[i]] == h.hash_ints(row[1:], row[0], t), (field, t, i)


def test_model_permutation_known_answers():
    """the reference's known answers (poseidon_bn128_opt.rs, poseidon_bls12381_opt.rs), as tests/test_gpu_bn128.py carries them"""
    kat = {"bn128": [([1], 0x29176100eaa962bdc1fe6c654d6a3c130e96a4d1168b33848b897dc502820133),
                     ([1, 2], 0x115cc0f5e7d690413df64c6b9662e9cf2a3617f2743245519e19607a4417189a),
                     ([1, 2, 0, 0, 0], 0x024058dd1e168f34bac462b6fffe58fd69982807e9884c1c6148182319cee427),
                     ([3, 4, 0, 0, 0, 0], 0x1b1caddfc5ea47e09bb445a7447eb9694b8d1b75a97fff58e884398c6b22825a),
                     ([1, 2, 3, 4, 5, 6], 0x2d1a03850084442813c8ebf094dea47538490a68b05f2239134a4cca2f6302e1),
                     (list(range(16)), 0x1b733f2ff41971b23819a16bc8c16bbe13d98173358429fcc12f6f0826407a56)],
           "bls12381": [([1], 0x164efff6c8a32ef98836c868f8c8dedcbe3068d16ba6098f282a6d185edb551f),
                        ([1, 2, 0, 0, 0], 0x385acd94e53a8c6f981809c2201582beceaec12250200f1e75ba93e6cf5ec736),
                        ([1, 2, 3, 4], 0x6f5f297b0ab0d1e7400501b9bdd4c3be2fe676b6a05deb845143b87355167a8d),
                        (list(range(16)), 0x12d374bbdb8d3c1c0230b20b8fe1572f1e652a616d16e834718a982574106405)]}
    for field, rows in kat.items():
        for inp, exp in rows:
            got = mm.model(field, len(inp) + 1).permutation(np.array([[0] + inp], dtype=object))
            assert int(got[0, mm.OUT_IDX[field]]) == exp, (field, inp)


@pytest.mark.parametrize("field", FIELDS)
def test_directed_states_reach_what_they_are_for(field):
    """the state built for the carry of mf_reduce_words does make it wrap, in the first sparse round already; a driver of a digit
    column does push it further than any other directed state; the model objects to what the device code excludes"""
    for t in (3, 17):
        m = mm.model(field, t)
        pats = mm.directed(field, t)
        X = np.array(pats, dtype=object)
        _, wrapped = m.sparse(1, X)
        assert wrapped.any(), f"{field} t = {t}: no directed state makes lo[q] + c wrap"
        D, _ = m.dense_tables(0)
        col0 = mm.byte_matrix(X) @ D[:, 0]                                  # digit column 0 of output 0 of M
        drivers = m.column_drivers(D[:, :32], (0,))
        hi, lo = (int((mm.byte_matrix(np.array([d], dtype=object)) @ D[:, 0])[0]) for d in drivers)
        assert hi == col0.max() and lo == col0.min() and hi > 0 > lo
    m = mm.model(field, 3)
    with pytest.raises(mm.MfModelError, match="biased word"):
        m._finish(np.zeros((1, 1, 32)), np.zeros((1, 8), np.int64), 29, "no addends")
    with pytest.raises(mm.MfModelError, match="digit column"):
        m._finish(np.full((1, 1, 32), float(1 << 23)), np.full((1, 8), 1 << 48, np.int64), 29, "a column at 2^23")
