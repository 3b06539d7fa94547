"""The reference of fflonk with lookups (tests/fflonk_lookup_ref.py) against itself and against the HOST part of eigen_zkvm_amd.fflonk_lookup,
without a GPU: the field facts round 3 relies on; the reference's proof passes the package's verifier arithmetic (host_check, which rebuilds
the 26 opened values) and the opening equation in scalars under the known tau; every mutation of it does not.  The package's transcript
gives the reference's challenges, every point of the proof moves one, and the lookup sum closes exactly when the multiplicities are right.
A point is stood in for by its scalar's bytes here: the transcript hashes it and the equation in the exponent reads it back."""
import importlib

import pytest

import fflonk_lookup_ref as ref
import kzg_multi_ref as mref

TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
PB = {"BN128": 64, "BLS12381": 96}
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]
CASES = [("BN128", 0, BLIND), ("BN128", 0, [0] * 14), ("BN128", 1, BLIND), ("BLS12381", 1, BLIND)]
IDS = lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain")


@pytest.fixture(scope="module")
def fl(zk):
    return importlib.import_module("eigen_zkvm_amd.fflonk_lookup")


@pytest.fixture(scope="module")
def made():
    out = {}
    for cv, steps, blind in CASES:
        n_vars, public, gates, table, wit = ref.lookup_chain(steps, ref.R[cv])
        R = ref.Reference(cv, n_vars, public, gates, table, TAU[cv], lambda s, cv=cv: s.to_bytes(PB[cv], "little"))
        assert R.t.n == (8, 16)[steps]
        out[(cv, steps, tuple(blind))] = (R, wit, R.prove(wit, blind))
    return out


def _scalar(b):
    return int.from_bytes(b, "little")


def _vk(fl, R, c0=None, c0l=None):
    t = R.t
    return fl.VerifyingKey(R.curve, t.log_n, t.l, t.k[1], t.k[2], R.C0 if c0 is None else c0, R.C0L if c0l is None else c0l)


def _accepts(fl, R, vk, publics, proof, swap=None):
    """the package's host part, then the opening equation in scalars under the known tau: the whole verifier but for the group"""
    verdict, tup = fl.host_check(vk, publics, proof)
    if verdict != fl.ACCEPTED:
        return verdict
    cs, sets, ys, g, z, W1, W2 = tup
    if swap:
        i, j = swap
        sets, ys = list(sets), list(ys)
        sets[i], sets[j], ys[i], ys[j] = sets[j], sets[i], ys[j], ys[i]
    return int(mref.proof_holds([_scalar(c) for c in cs], sets, ys, g, z, _scalar(W1), _scalar(W2), R.tau, R.r))


@pytest.mark.parametrize("cv", ("BN128", "BLS12381"))
def test_the_field_facts_of_round_3(fl, cv):
    r = ref.R[cv]
    kzg = importlib.import_module("eigen_zkvm_amd.kzg")
    for log_n in (3, 4, 9, 20):
        facts = ref.field_facts(cv, log_n)
        assert all(facts.values()), [k for k, v in facts.items() if not v]
        n, w = 1 << log_n, fl.omega(cv, log_n)
        w4n = pow(7, (r - 1) // (4 * n), r)
        assert pow(w4n, 4, r) == w == pow(fl.omega(cv, log_n + 2), 4, r)
        rt = fl.roots(cv, log_n, 0x1234567)
        xi = rt["xi"]
        assert pow(rt["h0"], 8, r) == pow(rt["h1"], 4, r) == pow(rt["h3"], 2, r) == xi and pow(rt["h1"] * w4n, 4, r) == xi * w % r == rt["xiw"]
        assert all(pow(x, 8, r) == xi for x in rt["S0"]) and all(pow(x, 4, r) == xi for x in rt["S1"]) and all(pow(x, 2, r) == xi for x in rt["S3"])
        assert rt["S2"][:4] == rt["S1"] and all(pow(x, 4, r) == rt["xiw"] for x in rt["S2"][4:])
        assert len(set(rt["S2"])) == 8 and len(set(rt["S0"])) == 8 and len(set(rt["S3"])) == 2      # S2's eight points distinct
        assert len(rt["S0"]) + 2 * len(rt["S1"]) + len(rt["S2"]) + len(rt["S3"]) == fl.N_OPENED == 26
        assert len(set(fl.all_points(rt))) == 18 and set(fl.all_points(rt)) == set(rt["S0"] + rt["S1"] + rt["S2"] + rt["S3"])
        assert (xi, [rt["S0"], rt["S1"], rt["S2"], rt["S3"]]) == ref.roots_of(cv, log_n, 0x1234567)
        assert max(len(rt[k]) for k in ("S0", "S1", "S2", "S3")) <= kzg.MULTI_MAX_POINTS
    with pytest.raises(fl.ZkError):                                                          # k + 2 beyond the 2-adicity
        fl.roots(cv, ref.pref.TWO_ADICITY[cv] - 1, 5)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_reference_proof_holds_and_every_mutation_does_not(fl, made, case):
    cv, steps, blind = case
    R, wit, res = made[(cv, steps, tuple(blind))]
    r, t = R.r, R.t
    vk = _vk(fl, R)
    assert vk.digest == R.vkd
    proof, publics = res["proof"], res["publics"]
    assert R.opening_holds(res)
    verdict, tup = fl.host_check(vk, publics, proof)
    assert verdict == fl.ACCEPTED
    cs, sets, ys, g, z, W1, W2 = tup
    assert (sets, ys, g, z) == (res["sets"], res["ys"], res["challenges"]["gamma_open"], res["challenges"]["z_open"])
    assert cs == [R.C0, R.C0L, proof["C1"], proof["C2"], proof["C3"]] and (W1, W2) == (proof["W1"], proof["W2"])
    assert sets[1] == sets[2] and sets[3][:4] == sets[1]                                   # one set twice, and contained in another
    assert _accepts(fl, R, vk, publics, proof) == 1
    # T0 .. T3 at xi as the package derives them from the 22 values are the reference's pointwise quotients
    ch = res["challenges"]
    got = fl.quotients_at(cv, t.log_n, t.k[1], t.k[2], publics, ch, ch["xi"], dict(zip(fl.VALUE_NAMES, res["values"])))
    assert got == tuple(res["at_xi"][k] for k in ("t0", "t1", "t2", "t3"))
    # and the 26 opened values give the 22 back
    assert fl.values_of(cv, res["ys"], fl.roots(cv, t.log_n, ch["s"])) == (res["values"], got)
    assert fl.VALUE_NAMES == ref.VALUE_NAMES and len(res["values"]) == fl.N_VALUES == 22
    for i in range(22):                                                                # every one of the 22 values
        moved = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert _accepts(fl, R, vk, publics, moved) == 0, i
        ys2 = fl.host_check(vk, publics, moved)[1][2]                                  # and with the honest challenges kept: the opened values alone
        assert ys2 != res["ys"] and not R.opening_holds(res, ys=ys2), i
    for name in fl.POINT_NAMES:                                                        # each of the 5 points' scalars
        other = ((_scalar(proof[name]) + 1) % r).to_bytes(PB[cv], "little")
        assert _accepts(fl, R, vk, publics, dict(proof, **{name: other})) == 0, name
    for i in range(5):
        f = list(res["f_tau"])
        f[i] = (f[i] + 1) % r
        assert not R.opening_holds(res, f_tau=f), i
    assert not R.opening_holds(res, w1=(res["w1"] + 1) % r) and not R.opening_holds(res, w2=(res["w2"] + 1) % r)
    assert not R.opening_holds(res, gamma=(ch["gamma_open"] + 1) % r) and not R.opening_holds(res, z=(ch["z_open"] + 1) % r)
    assert _accepts(fl, R, _vk(fl, R, c0=((R.c0 + 1) % r).to_bytes(PB[cv], "little")), publics, proof) == 0          # another [C0]
    assert _accepts(fl, R, _vk(fl, R, c0l=((R.c0l + 1) % r).to_bytes(PB[cv], "little")), publics, proof) == 0        # another [C0L]
    assert _accepts(fl, R, _vk(fl, R, c0=R.C0L, c0l=R.C0), publics, proof) == 0                                      # the two exchanged
    for i in range(len(publics)):                                                      # each public input
        assert _accepts(fl, R, vk, publics[:i] + [(publics[i] + 1) % r] + publics[i + 1:], proof) == 0, i
    for swap in ((0, 3), (2, 3), (3, 4), (0, 4)):                                      # swapped set order
        assert _accepts(fl, R, vk, publics, proof, swap=swap) == 0, swap
    halves = list(res["sets"])
    halves[3] = halves[3][4:] + halves[3][:4]                                          # the two halves of S2 exchanged under the same values
    assert not R.opening_holds(res, sets=halves)
    # eta and delta exchanged: the opened values of C2 and C3 (T0 .. T3) the verifier would rebuild are others
    ex = dict(ch, eta=ch["delta"], delta=ch["eta"])
    ys_ex = fl.opened_values(cv, t.log_n, t.k[1], t.k[2], publics, res["values"], ex, fl.roots(cv, t.log_n, ch["s"]))
    assert ys_ex[:4] == res["ys"][:4] and ys_ex[4] != res["ys"][4] and not R.opening_holds(res, ys=ys_ex)
    for i in (0, 8, 11, 15, 21):                                                       # a value >= r
        assert _accepts(fl, R, vk, publics, dict(proof, values=proof["values"][:i] + [r] + proof["values"][i + 1:])) == fl.INPUT_NOT_CANONICAL, i
    assert _accepts(fl, R, vk, [r], proof) == fl.INPUT_NOT_CANONICAL
    assert not fl.VerifyingKey(cv, t.log_n, t.l, t.k[1], t.k[1], R.C0, R.C0L).digest == vk.digest


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_package_transcript_gives_the_reference_challenges(fl, made, case):
    cv, steps, blind = case
    R, wit, res = made[(cv, steps, tuple(blind))]
    t, r = R.t, R.r
    vk = _vk(fl, R)
    proof, ch = res["proof"], res["challenges"]
    assert fl.challenges(vk, res["publics"], proof) == ch
    # PI left out of c0 would give the same challenges for other public inputs: they must differ
    assert fl.challenges(vk, [(res["publics"][0] + 1) % r], proof)["beta"] != ch["beta"]
    # every point of the proof moves a challenge: C1 the four of round 1, C2 and C3 the seed, W1 the opening's z'; W2 is the last message
    for name, moves in (("C1", ("beta", "gamma", "eta", "delta", "s")), ("C2", ("s", "xi", "gamma_open")), ("C3", ("s", "xi", "gamma_open")), ("W1", ("z_open",))):
        other = fl.challenges(vk, res["publics"], dict(proof, **{name: bytes(PB[cv] - 1) + b"\x01"}))
        assert all(other[k] != ch[k] for k in moves), name
        if name != "C1":
            assert all(other[k] == ch[k] for k in ("beta", "gamma", "eta", "delta")), name
    assert fl.challenges(vk, res["publics"], dict(proof, W2=bytes(PB[cv]))) == ch
    assert len({ch[k] for k in ("beta", "gamma", "eta", "delta")}) == 4
    data = fl.proof_to_bytes(proof)
    assert len(data) == 5 * PB[cv] + 22 * 32 and fl.proof_from_bytes(data, PB[cv]) == proof
    assert vk.digest == R.vkd


def test_the_sum_closes_exactly_when_the_multiplicities_are_right():
    cv = "BN128"
    r = ref.R[cv]
    n_vars, public, gates, table, wit = ref.lookup_chain(1, r)
    R = ref.Reference(cv, n_vars, public, gates, table, TAU[cv], lambda s: s.to_bytes(64, "little"))
    wires = R.wires_of(wit)
    m, bad = R.multiplicities(wires)
    assert not bad and sum(m) == sum(R.qk) and m[1] == 0 and R.rows[0] == R.rows[1]        # the first index of the repeated row takes the count
    assert R.running_sum(wires, m, 5, 7)[1] == 0
    j = next(i for i, c in enumerate(m) if c)
    moved = list(m)
    moved[j] -= 1
    moved[next(k for k in range(R.t.n) if R.rows[k] != R.rows[j])] += 1
    assert R.running_sum(wires, moved, 5, 7)[1] != 0
    with pytest.raises(AssertionError, match="the lookup sum does not close"):
        R.prove(wit, BLIND, multiplicities=moved)
    onto_copy = [m[0] - 1, 1] + m[2:]                                                       # onto the other copy of the same row: closes, another proof
    assert R.running_sum(wires, onto_copy, 5, 7)[1] == 0
    assert R.prove(wit, BLIND, multiplicities=onto_copy)["proof"]["C1"] != R.prove(wit, BLIND)["proof"]["C1"]
    # a witness whose looked-up tuple is no row of the table, and one that breaks a gate
    looked = [i for i in range(R.t.n) if R.qk[i]]
    out = list(wit)
    out[R.t.wire["c"][looked[0]]] = (out[R.t.wire["c"][looked[0]]] + 2) % r
    assert R.multiplicities(R.wires_of(out))[1]
    broken = list(wit)
    broken[5] = (broken[5] + 1) % r
    assert R.gates_hold(R.wires_of(broken), [broken[public[0]]])
