"""The PLONK reference (tests/plonk_ref.py) against itself and against the HOST part of eigen_zkvm_amd.plonk, without a GPU: the reference's
proof satisfies the verifier's field identity (the reference's own and the package's, written separately) and the opening equation in
scalars under the known tau; every mutation of it does not.  The package's transcript gives the reference's challenges byte for byte.  A point
is stood in for by its scalar's bytes here: only the transcript reads it."""
import importlib

import pytest

import plonk_ref as ref

TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
PB = {"BN128": 64, "BLS12381": 96}
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(9)]
CASES = [("BN128", 1, BLIND), ("BN128", 1, [0] * 9), ("BN128", 3, BLIND), ("BLS12381", 3, BLIND)]


@pytest.fixture(scope="module")
def plonk(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk")


def _made(cv, steps, blind):
    r = ref.R[cv]
    n_vars, public, gates, wit = ref.chain(steps, r)
    R = ref.Reference(cv, n_vars, public, gates, TAU[cv], lambda s: s.to_bytes(PB[cv], "little"))
    return R, R.prove(wit, blind)


@pytest.fixture(scope="module")
def made():
    return {(cv, steps, tuple(b)): _made(cv, steps, b) for cv, steps, b in CASES}


def test_the_chain_has_the_sizes_the_tests_rely_on():
    for steps, n in ((1, 8), (3, 16), (1023, 4096)):
        n_vars, public, gates, wit = ref.chain(steps, ref.R["BN128"])
        assert 1 + len(gates["a"]) == n - 1 and len(wit) == n_vars and public == [n_vars - 1]
    n_vars, public, gates, wit = ref.chain(1, ref.R["BN128"], 3)
    assert wit[public[0]] == 3 ** 3 + 3 + 5
    t = ref.Table("BN128", n_vars, public, gates)
    assert {t.wire[k][2] for k in "abc"} == {2}                       # one variable in all three columns
    assert t.sel["qC"][1] == ref.R["BN128"] - 5                       # a constant gate


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain"))
def test_the_reference_proof_holds_and_every_mutation_does_not(plonk, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    r = R.r
    ch, values, publics = res["challenges"], res["values"], res["publics"]
    assert R.identity_holds(publics, values, ch)
    assert plonk.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], publics, values, ch)
    assert R.opening_holds(res)
    for i in range(14):
        moved = list(values)
        moved[i] = (moved[i] + 1) % r
        assert not R.identity_holds(publics, moved, ch), i
        assert not plonk.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], publics, moved, ch), i
        assert not R.opening_holds(res, values=moved), i
    other = [(publics[0] + 1) % r]
    assert not R.identity_holds(other, values, ch) and not plonk.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], other, values, ch)
    for name in ("beta", "gamma", "alpha"):
        assert not plonk.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], publics, values, dict(ch, **{name: (ch[name] + 1) % r})), name
    assert not plonk.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[1], publics, values, ch)            # k_2 = k_1
    for i in range(13):
        f = list(res["f_tau"])
        f[i] = (f[i] + 1) % r
        assert not R.opening_holds(res, f_tau=f), i
    assert not R.opening_holds(res, w1=(res["w1"] + 1) % r) and not R.opening_holds(res, w2=(res["w2"] + 1) % r)
    assert not R.opening_holds(res, gamma=(ch["gamma_open"] + 1) % r) and not R.opening_holds(res, z=(ch["z_open"] + 1) % r)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain"))
def test_the_package_transcript_and_host_check_agree_with_the_reference(plonk, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    vk = plonk.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)
    assert vk.digest == R.vkd
    assert plonk.challenges(vk, res["publics"], res["proof"]) == res["challenges"]
    verdict, tup = plonk.host_check(vk, res["publics"], res["proof"])
    assert verdict == plonk.ACCEPTED
    cs, sets, ys, g, z, W1, W2 = tup
    assert (sets, ys, g, z) == (res["sets"], res["ys"], res["challenges"]["gamma_open"], res["challenges"]["z_open"])
    assert cs == R.vk_points + [res["proof"][k] for k in ("A", "B", "C", "T", "Z")] and (W1, W2) == (res["proof"]["W1"], res["proof"]["W2"])
    r = R.r
    moved = dict(res["proof"], values=[(res["proof"]["values"][0] + 1) % r] + res["proof"]["values"][1:])
    assert plonk.host_check(vk, res["publics"], moved) == (plonk.REJECTED, None)
    assert plonk.host_check(vk, [(res["publics"][0] + 1) % r], res["proof"]) == (plonk.REJECTED, None)
    assert plonk.host_check(vk, res["publics"], dict(res["proof"], values=res["proof"]["values"][:13] + [r])) == (plonk.INPUT_NOT_CANONICAL, None)
    assert plonk.host_check(vk, [r], res["proof"]) == (plonk.INPUT_NOT_CANONICAL, None)
    with pytest.raises(plonk.ZkError, match="a proof holds 14 values"):
        plonk.host_check(vk, res["publics"], dict(res["proof"], values=res["proof"]["values"][:13]))
    with pytest.raises(plonk.ZkError, match="point W2 of the proof is"):
        plonk.host_check(vk, res["publics"], dict(res["proof"], W2=res["proof"]["W2"][:-1]))
    data = plonk.proof_to_bytes(res["proof"])
    assert plonk.proof_from_bytes(data, PB[cv]) == res["proof"]
    with pytest.raises(plonk.ZkError, match="a proof is %d bytes" % len(data)):
        plonk.proof_from_bytes(data[:-1], PB[cv])
    # PI left out of c0 would give the same challenges for other public inputs: they must differ
    assert plonk.challenges(vk, [(res["publics"][0] + 1) % r], res["proof"])["beta"] != res["challenges"]["beta"]


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
    # row 2 is x + x - 2x = 0 for ANY x: another value there satisfies every gate and breaks the copy of x
    for k in "abc":
        wires[k][2] = (wires[k][2] + 9) % r
    assert not R.gates_hold(wires, [wit[public[0]]]) and R.product(wires, 5, 7)[1] != 1
