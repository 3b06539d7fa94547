"""The reference of the PLONK prover with lookups (tests/plonk_lookup_ref.py) against itself and against the HOST part of
eigen_zkvm_amd.plonk_lookup, without a GPU: the reference's proof satisfies the verifier's field identity (the reference's own and the
package's, written separately) and the opening equation in scalars under the known tau; every single mutation does not.  The package's
transcript gives the reference's challenges byte for byte.  A point is stood in for by its scalar's bytes: only the transcript reads it."""
import importlib

import pytest

import plonk_lookup_ref as lref
import plonk_ref as ref

TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
PB = {"BN128": 64, "BLS12381": 96}
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]
CASES = [("BN128", 0, BLIND), ("BN128", 0, [0] * 14), ("BN128", 1, BLIND), ("BLS12381", 1, BLIND)]
IDS = lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain")
POINTS = ("A", "B", "C", "M", "Z", "Phi", "T")


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


def _made(cv, steps, blind):
    n_vars, public, gates, table, wit = lref.lookup_chain(steps, ref.R[cv])
    R = lref.Reference(cv, n_vars, public, gates, table, TAU[cv], lambda s: s.to_bytes(PB[cv], "little"))
    return R, R.prove(wit, blind)


@pytest.fixture(scope="module")
def made():
    return {(cv, steps, tuple(b)): _made(cv, steps, b) for cv, steps, b in CASES}


def test_the_circuits_have_the_sizes_and_the_table_the_tests_rely_on():
    r = ref.R["BN128"]
    for steps, n in ((0, 8), (1, 16)):
        n_vars, public, gates, table, wit = lref.lookup_chain(steps, r)
        R = lref.Reference("BN128", n_vars, public, gates, table, TAU["BN128"], lambda s: s.to_bytes(64, "little"))
        assert R.t.n == n and len(wit) == n_vars and sum(gates["qK"]) >= 2
        m, bad = R.multiplicities(R.wires_of(wit))
        assert not bad and sum(m) == sum(gates["qK"]) and table[0] == table[1] and m[1] == 0     # the duplicated row's second copy counts nothing
        assert R.rows[len(table):] == [R.rows[len(table) - 1]] * (n - len(table))
    # a table longer than the gates forces n
    n_vars, public, gates, table, wit = lref.lookup_chain(0, r, bits=3)
    assert lref.Reference("BN128", n_vars, public, gates, table, 5, lambda s: s.to_bytes(64, "little")).t.n == 128


def test_the_sum_closes_exactly_when_the_multiplicities_are_right():
    cv = "BN128"
    r = ref.R[cv]
    n_vars, public, gates, table, wit = lref.lookup_chain(1, r)
    R = lref.Reference(cv, n_vars, public, gates, table, TAU[cv], lambda s: s.to_bytes(64, "little"))
    wires = R.wires_of(wit)
    m, bad = R.multiplicities(wires)
    assert R.running_sum(wires, m, 11, 13)[1] == 0
    moved = list(m)
    j = next(i for i, c in enumerate(m) if c)
    moved[j] -= 1
    moved[next(k for k in range(len(m)) if R.rows[k] != R.rows[j])] += 1                    # onto another row: onto a copy of the same row it would still close
    assert R.running_sum(wires, moved, 11, 13)[1] != 0
    i = R.qk.index(1)                                                                       # a selected row outside the table
    wires["c"][i] = (wires["c"][i] + 1) % r
    assert R.multiplicities(wires)[1] == [i]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_reference_proof_holds_and_every_mutation_does_not(pl, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    r = R.r
    ch, values, publics = res["challenges"], res["values"], res["publics"]
    held = lambda p, v, c: pl.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], p, v, c)
    assert len(values) == 21 and R.identity_holds(publics, values, ch) and held(publics, values, ch) and R.opening_holds(res)
    for i in range(21):
        moved = list(values)
        moved[i] = (moved[i] + 1) % r
        assert not R.identity_holds(publics, moved, ch), i
        assert not held(publics, moved, ch), i
        assert not R.opening_holds(res, values=moved), i
    other = [(publics[0] + 1) % r]
    assert not R.identity_holds(other, values, ch) and not held(other, values, ch)
    for name in ("beta", "gamma", "alpha", "eta", "delta"):
        assert not held(publics, values, dict(ch, **{name: (ch[name] + 1) % r})), name
    swapped = dict(ch, eta=ch["delta"], delta=ch["eta"])
    assert not held(publics, values, swapped) and not R.identity_holds(publics, values, swapped)
    for i in range(19):                                                                     # the 12 fixed commitments and the proof's seven
        f = list(res["f_tau"])
        f[i] = (f[i] + 1) % r
        assert not R.opening_holds(res, f_tau=f), i
    assert not R.opening_holds(res, w1=(res["w1"] + 1) % r) and not R.opening_holds(res, w2=(res["w2"] + 1) % r)
    assert not R.opening_holds(res, gamma=(ch["gamma_open"] + 1) % r) and not R.opening_holds(res, z=(ch["z_open"] + 1) % r)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_package_transcript_and_host_check_agree_with_the_reference(pl, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    r, proof = R.r, res["proof"]
    vk = pl.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)
    assert vk.digest == R.vkd
    assert pl.challenges(vk, res["publics"], proof) == res["challenges"]
    verdict, tup = pl.host_check(vk, res["publics"], proof)
    assert verdict == pl.ACCEPTED
    cs, sets, ys, g, z, W1, W2 = tup
    assert (sets, ys, g, z) == (res["sets"], res["ys"], res["challenges"]["gamma_open"], res["challenges"]["z_open"])
    assert cs == R.vk_points + [proof[k] for k in ("A", "B", "C", "T", "M", "Z", "Phi")] and (W1, W2) == (proof["W1"], proof["W2"])
    for name in POINTS:                                                                     # every point of the proof moves a challenge of the identity
        other = (int.from_bytes(proof[name], "little") + 1).to_bytes(PB[cv], "little")
        assert pl.host_check(vk, res["publics"], dict(proof, **{name: other})) == (pl.REJECTED, None), name
    w1 = (res["w1"] + 1).to_bytes(PB[cv], "little")
    assert pl.host_check(vk, res["publics"], dict(proof, W1=w1))[1][4] != z                  # W1 moves z'; W2 is the pairing's to refuse
    moved = dict(proof, values=[(proof["values"][0] + 1) % r] + proof["values"][1:])
    assert pl.host_check(vk, res["publics"], moved) == (pl.REJECTED, None)
    assert pl.host_check(vk, [(res["publics"][0] + 1) % r], proof) == (pl.REJECTED, None)
    assert pl.host_check(vk, res["publics"], dict(proof, values=proof["values"][:20] + [r])) == (pl.INPUT_NOT_CANONICAL, None)
    assert pl.host_check(vk, [r], proof) == (pl.INPUT_NOT_CANONICAL, None)
    with pytest.raises(pl.ZkError, match="a proof holds 21 values"):
        pl.host_check(vk, res["publics"], dict(proof, values=proof["values"][:20]))
    with pytest.raises(pl.ZkError, match="the proof holds no M, Phi"):
        pl.host_check(vk, res["publics"], {k: v for k, v in proof.items() if k not in ("M", "Phi")})
    data = pl.proof_to_bytes(proof)
    assert len(data) == 9 * PB[cv] + 21 * 32 and pl.proof_from_bytes(data, PB[cv]) == proof
    with pytest.raises(pl.ZkError, match="a proof is %d bytes" % len(data)):
        pl.proof_from_bytes(data[:-1], PB[cv])
    assert pl.challenges(vk, [(res["publics"][0] + 1) % r], proof)["eta"] != res["challenges"]["eta"]


def test_keys_and_transcripts_of_the_two_provers_are_apart(pl, made):
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    R, res = made[("BN128", 0, tuple(BLIND))]
    assert pl.vk_digest("BN128", 3, 1, 2, 3, R.vk_points[:8]) != plonk.vk_digest("BN128", 3, 1, 2, 3, R.vk_points[:8])
    assert pl.transcript_start("BN128", R.vkd, [5]) != plonk.transcript_start("BN128", R.vkd, [5])
    with pytest.raises(pl.ZkError, match="holds 12 commitments"):
        pl.VerifyingKey("BN128", 3, 1, 2, 3, R.vk_points[:8])
