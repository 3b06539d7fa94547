"""The fflonk reference (tests/fflonk_ref.py) against itself and against the HOST part of eigen_zkvm_amd.fflonk, without a GPU: the field
facts round 3 relies on; the reference's proof passes the package's verifier arithmetic (host_check, which rebuilds the 18 opened values) and
the opening equation in scalars under the known tau; every mutation of it does not.  The package's transcript gives the reference's
challenges.  A point is stood in for by its scalar's bytes here: the transcript hashes it and the equation in the exponent reads it back."""
import importlib

import pytest

import fflonk_ref as ref
import kzg_multi_ref as mref

TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
PB = {"BN128": 64, "BLS12381": 96}
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(9)]
CASES = [("BN128", 1, BLIND), ("BN128", 1, [0] * 9), ("BN128", 3, BLIND), ("BLS12381", 3, BLIND)]
IDS = lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain")


@pytest.fixture(scope="module")
def fflonk(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk")


@pytest.fixture(scope="module")
def made():
    out = {}
    for cv, steps, blind in CASES:
        n_vars, public, gates, wit = ref.chain(steps, ref.R[cv])
        R = ref.Reference(cv, n_vars, public, gates, TAU[cv], lambda s, cv=cv: s.to_bytes(PB[cv], "little"))
        out[(cv, steps, tuple(blind))] = (R, R.prove(wit, blind))
    return out


def _scalar(b):
    return int.from_bytes(b, "little")


def _accepts(fflonk, R, vk, publics, proof, swap=None):
    """the package's host part, then the opening equation in scalars under the known tau: the whole verifier but for the group"""
    verdict, tup = fflonk.host_check(vk, publics, proof)
    if verdict != fflonk.ACCEPTED:
        return verdict
    cs, sets, ys, g, z, W1, W2 = tup
    if swap:
        i, j = swap
        sets, ys = list(sets), list(ys)
        sets[i], sets[j], ys[i], ys[j] = sets[j], sets[i], ys[j], ys[i]
    return int(mref.proof_holds([_scalar(c) for c in cs], sets, ys, g, z, _scalar(W1), _scalar(W2), R.tau, R.r))


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_the_field_facts_of_round_3(fflonk, cv):
    r = ref.R[cv]
    for log_n in (3, 4, 9, 20):
        facts = ref.field_facts(cv, log_n)
        assert all(facts.values()), [k for k, v in facts.items() if not v]
        n, w = 1 << log_n, fflonk.omega(cv, log_n)
        rt = fflonk.roots(cv, log_n, 0x1234567)
        xi = rt["xi"]
        assert pow(rt["h0"], 8, r) == pow(rt["h1"], 4, r) == pow(rt["h2"], 3, r) == xi and pow(rt["h3"], 3, r) == xi * w % r == rt["xiw"]
        assert all(pow(x, 8, r) == xi for x in rt["S0"]) and all(pow(x, 4, r) == xi for x in rt["S1"])
        assert all(pow(x, 3, r) == xi for x in rt["S2"][:3]) and all(pow(x, 3, r) == rt["xiw"] for x in rt["S2"][3:])
        assert len(set(rt["S0"] + rt["S1"] + rt["S2"])) == fflonk.N_OPENED == 18
        assert (xi, [rt["S0"], rt["S1"], rt["S2"]]) == ref.roots_of(cv, log_n, 0x1234567)
        assert max(len(rt[k]) for k in ("S0", "S1", "S2")) <= importlib.import_module("eigen_zkvm_amd.kzg").MULTI_MAX_POINTS
    assert fflonk.omega3(cv) == ref.omega3(cv) != 1 and (r - 1) % 24 == 0


def test_the_powers_a_file_must_hold(fflonk):
    for log_n in (3, 20):
        n = 1 << log_n
        assert fflonk.required_powers(n) == 9 * n + 18
        assert fflonk.file_power(log_n) == log_n + 3
        assert (2 << (log_n + 3)) - 1 >= 9 * n + 18 > (2 << (log_n + 2)) - 1
        assert sum(fflonk.quotient_coeffs(n)) == (2 * n + 2) + (n + 2) + (3 * n + 6) and 3 * fflonk.quotient_coeffs(n)[2] == 9 * n + 18

        class File:
            curve, max_coeffs = "BN128", 9 * n + 17

        class Table:
            curve = "BN128"
        Table.n, Table.log_n = n, log_n
        with pytest.raises(fflonk.ZkError, match=r"the file holds %d G1 powers, n = %d rows need 9n \+ 18 = %d \(a file of power %d has them\)" % (9 * n + 17, n, 9 * n + 18, log_n + 3)):
            fflonk.FflonkKey(File, Table)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_reference_proof_holds_and_every_mutation_does_not(fflonk, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    r, t = R.r, R.t
    vk = fflonk.VerifyingKey(cv, t.log_n, t.l, t.k[1], t.k[2], R.C0)
    assert vk.digest == R.vkd
    proof, publics = res["proof"], res["publics"]
    assert R.opening_holds(res)
    verdict, tup = fflonk.host_check(vk, publics, proof)
    assert verdict == fflonk.ACCEPTED
    cs, sets, ys, g, z, W1, W2 = tup
    assert (sets, ys, g, z) == (res["sets"], res["ys"], res["challenges"]["gamma_open"], res["challenges"]["z_open"])
    assert cs == [R.C0, proof["C1"], proof["C2"]] and (W1, W2) == (proof["W1"], proof["W2"])
    assert _accepts(fflonk, R, vk, publics, proof) == 1
    # T0, T1, T2 at xi as the package derives them from the 15 values are the reference's pointwise quotients
    ch = res["challenges"]
    got = fflonk.quotients_at(cv, t.log_n, t.k[1], t.k[2], publics, ch["beta"], ch["gamma"], ch["xi"], dict(zip(fflonk.VALUE_NAMES, res["values"])))
    assert got == tuple(res["at_xi"][k] for k in ("T0", "T1", "T2"))
    # and the 18 opened values give the 15 back
    assert fflonk.values_of(cv, res["ys"], fflonk.roots(cv, t.log_n, ch["s"])) == (res["values"], got)
    for i in range(15):                                                                # every one of the 15 values
        moved = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert _accepts(fflonk, R, vk, publics, moved) == 0, i
        ys2 = fflonk.host_check(vk, publics, moved)[1][2]                              # and with the honest challenges kept: the opened values alone
        assert ys2 != res["ys"] and not R.opening_holds(res, ys=ys2), i
    for name in fflonk.POINT_NAMES:                                                    # each of the 4 points' scalars
        other = ((_scalar(proof[name]) + 1) % r).to_bytes(PB[cv], "little")
        assert _accepts(fflonk, R, vk, publics, dict(proof, **{name: other})) == 0, name
    for i in range(3):
        f = list(res["f_tau"])
        f[i] = (f[i] + 1) % r
        assert not R.opening_holds(res, f_tau=f), i
    assert not R.opening_holds(res, w1=(res["w1"] + 1) % r) and not R.opening_holds(res, w2=(res["w2"] + 1) % r)
    assert not R.opening_holds(res, gamma=(ch["gamma_open"] + 1) % r) and not R.opening_holds(res, z=(ch["z_open"] + 1) % r)
    vk0 = fflonk.VerifyingKey(cv, t.log_n, t.l, t.k[1], t.k[2], ((R.c0 + 1) % r).to_bytes(PB[cv], "little"))
    assert _accepts(fflonk, R, vk0, publics, proof) == 0                               # another [C0]
    for i in range(len(publics)):                                                      # each public input
        assert _accepts(fflonk, R, vk, publics[:i] + [(publics[i] + 1) % r] + publics[i + 1:], proof) == 0, i
    for swap in ((0, 1), (1, 2), (0, 2)):                                              # swapped set order
        assert _accepts(fflonk, R, vk, publics, proof, swap=swap) == 0, swap
    halves = [res["sets"][0], res["sets"][1], res["sets"][2][3:] + res["sets"][2][:3]]  # the h2 and h3 halves of S2 exchanged under the same values
    assert not R.opening_holds(res, sets=halves)
    for i in (0, 8, 11, 14):                                                           # a value >= r
        assert _accepts(fflonk, R, vk, publics, dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])) == fflonk.INPUT_NOT_CANONICAL, i
    assert _accepts(fflonk, R, vk, [r], proof) == fflonk.INPUT_NOT_CANONICAL
    assert not fflonk.VerifyingKey(cv, t.log_n, t.l, t.k[1], t.k[1], R.C0).digest == vk.digest


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_package_transcript_gives_the_reference_challenges(fflonk, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    t, r = R.t, R.r
    vk = fflonk.VerifyingKey(cv, t.log_n, t.l, t.k[1], t.k[2], R.C0)
    assert fflonk.challenges(vk, res["publics"], res["proof"]) == res["challenges"]
    # PI left out of c0 would give the same challenges for other public inputs: they must differ
    assert fflonk.challenges(vk, [(res["publics"][0] + 1) % r], res["proof"])["beta"] != res["challenges"]["beta"]
    data = fflonk.proof_to_bytes(res["proof"])
    assert len(data) == 4 * PB[cv] + 15 * 32 and fflonk.proof_from_bytes(data, PB[cv]) == res["proof"]
    back = fflonk.vk_from_bytes(fflonk.vk_to_bytes(vk))
    assert (back.curve, back.log_n, back.n_public, back.k1, back.k2, back.c0, back.digest) == (cv, t.log_n, t.l, t.k[1], t.k[2], R.C0, R.vkd)


def test_a_witness_that_breaks_a_gate_or_a_copy_is_seen_by_the_reference():
    cv = "BN128"
    r = ref.R[cv]
    n_vars, public, gates, wit = ref.chain(3, r)
    R = ref.Reference(cv, n_vars, public, gates, TAU[cv], lambda s: s.to_bytes(64, "little"))
    bad = list(wit)
    bad[5] = (bad[5] + 1) % r
    assert R.gates_hold(R.wires_of(bad), [bad[public[0]]])
    wires = R.wires_of(wit)
    assert R.product(wires, 5, 7)[1] == 1
    for k in "abc":
        wires[k][2] = (wires[k][2] + 9) % r
    assert not R.gates_hold(wires, [wit[public[0]]]) and R.product(wires, 5, 7)[1] != 1
