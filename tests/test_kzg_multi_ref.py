"""tests/kzg_multi_ref.py against itself, without a GPU: the quotient by a vanishing polynomial through partial fractions (the device's route)
equals the one through successive division (the reference's), an honest proof satisfies the verifier's equation in the exponent, and a proof
with one changed value does not."""
import random

import pytest

import kzg_ref as ref
import kzg_multi_ref as mref

TAU = 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e


def _case(rng, r, lens, sizes, shared=0):
    """polynomials of the given lengths, sets of the given sizes whose first `shared` points are common to all"""
    common = [rng.randrange(r) for _ in range(shared)]
    sets = []
    for ns in sizes:
        s = common[:ns]
        while len(s) < ns:
            p = rng.randrange(r)
            if p not in s:
                s.append(p)
        sets.append(s)
    return [[rng.randrange(r) for _ in range(n)] for n in lens], sets


@pytest.mark.parametrize("curve", sorted(ref.R))
def test_partial_fractions_equal_successive_division(curve):
    r, rng = ref.R[curve], random.Random(31)
    for n in (1, 2, 3, 4, 9, 40):
        for ns in (1, 2, 3, 8, 16):
            f = [rng.randrange(r) for _ in range(n)]
            pts = ([0, 1] + [rng.randrange(r) for _ in range(ns)])[:ns] if n % 2 else [rng.randrange(r) for _ in range(ns)]
            q, ys = mref.quotient_by_successive_division(f, pts, r)
            assert len(q) == max(n - ns, 0)
            pf = mref.quotient_by_partial_fractions(f, pts, r)
            assert pf[:len(q)] == q and not any(pf[len(q):]), (n, ns)
            x = rng.randrange(r)                        # f(x) = q(x) Z_S(x) + r_S(x) at a random x
            assert (ref.horner(q, x, r) * mref.vanishing_at(pts, x, r) + mref.lagrange_eval(pts, ys, x, r)) % r == ref.horner(f, x, r)
            assert ref.horner(mref.interpolant(pts, ys, r), x, r) == mref.lagrange_eval(pts, ys, x, r)


@pytest.mark.parametrize("curve", sorted(ref.R))
def test_an_honest_proof_holds_and_a_changed_value_does_not(curve):
    r, rng = ref.R[curve], random.Random(32)
    tau = TAU % r
    for lens, sizes, shared in (((7,), (1,), 0), ((9, 4, 12), (2, 3, 2), 0), ((9, 4, 12), (2, 3, 2), 2), ((5, 5), (4, 4), 4), ((2, 1, 3), (3, 2, 3), 1)):
        polys, sets = _case(rng, r, lens, sizes, shared)
        gamma, z = rng.randrange(r), rng.randrange(r)
        values, w1, w2 = mref.open_scalars(polys, sets, gamma, z, tau, r)
        assert values == [[ref.horner(f, s, r) for s in ss] for f, ss in zip(polys, sets)]
        cs = [ref.horner(f, tau, r) for f in polys]
        assert mref.proof_holds(cs, sets, values, gamma, z, w1, w2, tau, r)
        bad = [list(v) for v in values]
        bad[-1][0] = (bad[-1][0] + 1) % r
        assert not mref.proof_holds(cs, sets, bad, gamma, z, w1, w2, tau, r)
        if len(polys) > 1:                              # gamma^0 = 1: one polynomial does not meet gamma
            assert not mref.proof_holds(cs, sets, values, (gamma + 1) % r, z, w1, w2, tau, r)
        assert not mref.proof_holds(cs, sets, values, gamma, z, (w1 + 1) % r, w2, tau, r)
        assert not mref.proof_holds(cs, sets, values, gamma, z, w1, (w2 + 1) % r, tau, r)
        good = (cs, sets, values, gamma, z, w1, w2)
        assert mref.batch_holds([good, good], [3, 5], tau, r)
        assert not mref.batch_holds([good, (cs, sets, bad, gamma, z, w1, w2)], [3, 5], tau, r)


def test_every_polynomial_its_own_interpolant():
    """n_i <= |S_i|: q = 0, W1 is infinity (scalar zero), and the proof still holds"""
    r, rng = ref.R["BN128"], random.Random(33)
    polys, sets = _case(rng, r, (2, 3, 1), (2, 4, 1))
    gamma, z = rng.randrange(r), rng.randrange(r)
    values, w1, w2 = mref.open_scalars(polys, sets, gamma, z, TAU % r, r)
    assert w1 == 0
    assert mref.proof_holds([ref.horner(f, TAU % r, r) for f in polys], sets, values, gamma, z, w1, w2, TAU % r, r)


def test_interleave():
    assert mref.interleave([[1, 2, 3], [4], [], [5, 6]]) == [1, 4, 0, 5, 2, 0, 0, 6, 3, 0, 0, 0]
    assert mref.interleave([[7, 8]]) == [7, 8] and mref.interleave([]) == []
