"""zk_plonk_<curve>_r1cs_extend_dev against the plain-integer model of tests/plonk_r1cs_ref.py: the auxiliary variables of an
R1csCircuit, word for word the Montgomery words of the model's values, for both fields.  products(f, 600) is more than one workgroup of
two-term segments (the lane kernel); shapes(f) has segments on both sides of every small length and one of 999 terms whose operands are all
p - 1 (the wave kernel's bound); `edges` has a segment of T - 1, T, T + 1 terms for T = zk_plonk_r1cs_wave_min_terms() and of 63, 64, 65, 127,
128, 129 and 64 * 5 + 1 terms, every coefficient and every wire p - 1, more long segments than a workgroup has waves.  A second call on the
handle gives the same words, and nothing below n_wires is written.  Exact."""
import importlib

import numpy as np
import pytest

import plonk_r1cs_ref as model
import r1cs_check_cases as cases

pytestmark = pytest.mark.gpu
ABI = {"BN128": "bn254", "BLS12381": "bls12_381"}
FIELDS = ("BN128", "BLS12381")


@pytest.fixture(scope="module", autouse=True)
def _gpu(zk):
    assert zk.lib().zk_device_count() >= 1, "no GPU visible (the product has no CPU fallback)"
    zk.init(0)


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def edge_lengths(T):
    return sorted({T - 1, T, T + 1, 63, 64, 65, 127, 128, 129, 64 * 5 + 1} - {0, 1})


def edges(field, T):
    """one product constraint per length t: (sum of t wires, each times p - 1) * b = out, every wire p - 1 -> (r1cs bytes, witness)"""
    p = model.R[field]
    lengths = edge_lengths(T)
    top = max(lengths)
    w = [1] + [p - 1] * top
    b = len(w); w.append(p - 1)
    cons = []
    for t in lengths:
        w.append(t * (p - 1) * (p - 1) * (p - 1) % p)
        cons.append(([(j, p - 1) for j in range(1, t + 1)], [(b, 1)], [(len(w) - 1, 1)]))
    return cases.write(field, len(w), cons), w


@pytest.fixture(scope="module")
def world(zk, plonk):
    """per (circuit, field): the library's circuit, the witness and the model's extended values as Montgomery words, made once"""
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    T = int(zk.lib().zk_plonk_r1cs_wave_min_terms())
    made = {}

    def get(name, field):
        if (name, field) not in made:
            if name == "products":
                data, w, _ = cases.products(field, 600)
            elif name == "shapes":
                data, w, _, _ = cases.shapes(field)
            else:
                data, w = edges(field, T)
            m = model.Compiled(data, field)
            made[(name, field)] = (plonk.R1csCircuit(data, field), w, m, kzg.to_mont(m.extend(w), field))
        return made[(name, field)]
    get.T = T
    yield get
    for c, _, _, _ in made.values():
        c.free()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", ("products", "shapes", "edges"))
def test_the_extension_is_the_models_word_for_word(zk, plonk, world, name, field):
    c, w, m, want = world(name, field)
    T = world.T
    lens = [len(t) for _, t in m.segments]
    assert (c.n_vars, c.n_wires, c.n_aux) == (m.n_vars, m.n_wires, m.n_aux) and not m.failing_gates(m.extend(w))
    if name == "products":
        assert max(lens) < T and len(lens) > 256                                      # the lane kernel alone, more than one workgroup
    elif name == "shapes":
        assert max(lens) == 999 and {4, 5} <= set(lens) and len(lens) == 10            # short segments beside the long row
    else:
        assert lens == edge_lengths(T) and sum(n >= T for n in lens) > 4              # more long segments than a workgroup has waves
    d = plonk.extend_witness(c, w)
    try:
        got = d.to_host().reshape(-1, 4)
    finally:
        d.free()
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "variable %d of %d differs (n_wires = %d)" % (int(bad[0]), m.n_vars, m.n_wires)


@pytest.mark.parametrize("field", FIELDS)
def test_a_second_call_repeats_and_the_witness_is_not_written(zk, plonk, world, field):
    c, w, m, want = world("shapes", field)
    buf = want.copy()
    buf[m.n_wires:] = np.uint64(0xFFFFFFFFFFFFFFFF)                                   # what the call must overwrite; the front it must leave
    for _ in range(2):
        d = zk.DevArray.from_host(buf.reshape(-1))
        try:
            zk._check(getattr(zk.lib(), "zk_plonk_%s_r1cs_extend_dev" % ABI[field])(c._h, d.ptr, None))
            got = d.to_host().reshape(-1, 4)
        finally:
            d.free()
        assert np.array_equal(got[:m.n_wires], buf[:m.n_wires])
        assert np.array_equal(got, want)
    # the witness as .wtns bytes is the same extension
    d = plonk.extend_witness(c, cases.wtns_bytes(field, w))
    try:
        assert np.array_equal(d.to_host().reshape(-1, 4), want)
    finally:
        d.free()
