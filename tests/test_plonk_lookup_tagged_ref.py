"""The reference of the tagged lookups (tests/plonk_lookup_tagged_ref.py) against itself and against the HOST part of
eigen_zkvm_amd.plonk_lookup, without a GPU.  The model proves and verifies a circuit with a range table and an XOR table at n = 8 and 16;
the package's transcript, identity and host check agree with it; a row tagged "range" whose tuple is a row of the XOR table only is refused
by the model's prover, and a proof forced for it fails the model's verifier -- while the SAME cheat is accepted by the single-table model
over the concatenated table: the unsoundness the tags remove, pinned here.  A point is stood in for by its scalar's bytes."""
import importlib

import pytest

import plonk_lookup_ref as lref
import plonk_lookup_tagged_ref as tref
import plonk_ref as ref

TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
PB = {"BN128": 64, "BLS12381": 96}
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]
CASES = [("BN128", 0, BLIND), ("BN128", 0, [0] * 14), ("BN128", 1, BLIND), ("BLS12381", 1, BLIND)]
IDS = lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain")


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


def _point(cv):
    return lambda s: s.to_bytes(PB[cv], "little")


@pytest.fixture(scope="module")
def made():
    out = {}
    for cv, steps, blind in CASES:
        n_vars, public, gates, tables, wit = tref.tagged_chain(steps, ref.R[cv])
        R = tref.Reference(cv, n_vars, public, gates, tables, TAU[cv], _point(cv))
        out[(cv, steps, tuple(blind))] = (R, R.prove(wit, blind))
    return out


def test_the_circuits_have_the_sizes_and_the_tables_the_tests_rely_on():
    r = ref.R["BN128"]
    for steps, n in ((0, 8), (1, 16)):
        n_vars, public, gates, tables, wit = tref.tagged_chain(steps, r)
        R = tref.Reference("BN128", n_vars, public, gates, tables, TAU["BN128"], _point("BN128"))
        assert R.t.n == n and len(wit) == n_vars and {1, 2} <= set(gates["qK"]) <= {0, 1, 2}
        assert [row[0] for row in R.rows[:7]] == [1, 1, 2, 2, 2, 2, 2] and R.rows[7:] == [R.rows[6]] * (n - 7)          # padding repeats the last row, tag included
        assert R.rows[0][1:] == R.rows[2][1:] == R.rows[3][1:] == (0, 0, 0)                # one tuple in both tables, twice in the second
        m, bad = R.multiplicities(R.wires_of(wit))
        counts, _ = R.multiplicities(R.wires_of(wit), weighted=False)
        assert not bad and sum(counts) == sum(1 for q in gates["qK"] if q) and sum(m) == sum(gates["qK"])
        assert counts[0] == 1 and counts[2] == 2 and counts[3] == 0                        # (0, 0, 0) counted per table; the duplicate's second copy counts nothing
        assert all(m[j] == R.rows[j][0] * counts[j] for j in range(n))


def test_the_sum_closes_exactly_when_the_multiplicities_are_weighted():
    cv = "BN128"
    n_vars, public, gates, tables, wit = tref.tagged_chain(1, ref.R[cv])
    R = tref.Reference(cv, n_vars, public, gates, tables, TAU[cv], _point(cv))
    wires = R.wires_of(wit)
    m, _ = R.multiplicities(wires)
    assert R.running_sum(wires, m, 11, 13)[1] == 0
    assert R.running_sum(wires, R.multiplicities(wires, weighted=False)[0], 11, 13)[1] != 0       # the count alone is not m
    onto_other_table = list(m)                                                              # the count of (0, 0, 0) moved from table 2 to table 1
    onto_other_table[2] -= 2; onto_other_table[0] += 2
    assert R.running_sum(wires, onto_other_table, 11, 13)[1] != 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_model_proves_and_verifies_and_every_mutation_fails(pl, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    r = R.r
    ch, values, publics = res["challenges"], res["values"], res["publics"]
    held = lambda p, v, c: pl.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], p, v, c)
    assert len(values) == 22 and R.verify(res) and held(publics, values, ch)
    for i in range(22):
        moved = list(values)
        moved[i] = (moved[i] + 1) % r
        assert not R.identity_holds(publics, moved, ch), i
        assert not held(publics, moved, ch), i
        assert not R.opening_holds(res, values=moved), i
    for name in ("beta", "gamma", "alpha", "eta", "delta"):
        assert not held(publics, values, dict(ch, **{name: (ch[name] + 1) % r})), name
    for i in range(20):                                                                     # the 13 fixed commitments and the proof's seven
        f = list(res["f_tau"])
        f[i] = (f[i] + 1) % r
        assert not R.opening_holds(res, f_tau=f), i


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_package_transcript_and_host_check_agree_with_the_model(pl, made, case):
    cv, steps, blind = case
    R, res = made[(cv, steps, tuple(blind))]
    r, proof = R.r, res["proof"]
    vk = pl.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)
    assert vk.tagged and vk.digest == R.vkd
    assert vk.digest != pl.vk_digest(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)          # the single-table domain string
    assert pl.transcript_start(cv, R.vkd, res["publics"], True) != pl.transcript_start(cv, R.vkd, res["publics"])
    assert pl.challenges(vk, res["publics"], proof) == res["challenges"]
    verdict, tup = pl.host_check(vk, res["publics"], proof)
    assert verdict == pl.ACCEPTED
    cs, sets, ys, g, z, W1, W2 = tup
    assert (sets, ys, g, z) == (res["sets"], res["ys"], res["challenges"]["gamma_open"], res["challenges"]["z_open"])
    assert cs == R.vk_points + [proof[k] for k in ("A", "B", "C", "T", "M", "Z", "Phi")] and (W1, W2) == (proof["W1"], proof["W2"])
    for i in (0, 8, 12, 21):                                                               # q_L, q_K, T0, Phi(zeta w)
        moved = dict(proof, values=proof["values"][:i] + [(proof["values"][i] + 1) % r] + proof["values"][i + 1:])
        assert pl.host_check(vk, res["publics"], moved) == (pl.REJECTED, None), i
    assert pl.host_check(vk, res["publics"], dict(proof, values=proof["values"][:21] + [r])) == (pl.INPUT_NOT_CANONICAL, None)
    with pytest.raises(pl.ZkError, match="a proof holds 22 values, not 21"):
        pl.host_check(vk, res["publics"], dict(proof, values=proof["values"][:21]))
    data = pl.proof_to_bytes(proof)
    assert len(data) == 9 * PB[cv] + 22 * 32 and pl.proof_from_bytes(data, PB[cv], tagged=True) == proof
    with pytest.raises(pl.ZkError, match="a proof is %d bytes, not %d" % (len(data) - 32, len(data))):
        pl.proof_from_bytes(data, PB[cv])


def _cheat(cv):
    """tagged_chain(1) with the range lookup of row s = 2 moved onto (1, 1, 0): a row of the XOR table, no row of the range table"""
    r = ref.R[cv]
    n_vars, public, gates, tables, wit = tref.tagged_chain(1, r)
    g = max(i for i, q in enumerate(gates["qK"]) if q == 1)
    wit = list(wit) + [1, 1, 0]
    for k, v in zip("abc", range(n_vars, n_vars + 3)):
        gates[k][g] = v
    return n_vars + 3, public, gates, tables, wit, len(public) + g


def test_a_range_row_holding_an_xor_tuple_is_refused_and_a_forced_proof_fails(pl):
    cv = "BN128"
    n_vars, public, gates, tables, wit, row = _cheat(cv)
    R = tref.Reference(cv, n_vars, public, gates, tables, TAU[cv], _point(cv))
    wires = R.wires_of(wit)
    assert (wires["a"][row], wires["b"][row], wires["c"][row]) == (1, 1, 0) and R.qk[row] == 1
    assert (2, 1, 1, 0) in R.rows and (1, 1, 1, 0) not in R.rows
    assert R.multiplicities(wires)[1] == [row]
    with pytest.raises(AssertionError, match=r"rows \[%d\] are no rows of the tables they name" % row):
        R.prove(wit, BLIND)
    # forced: the prover books the row on the XOR table's (1, 1, 0) with the row's own weight, and checks nothing
    m, _ = R.multiplicities(wires)
    m[R.rows.index((2, 1, 1, 0))] += 1
    res = R.prove(wit, BLIND, multiplicities=m, force=True)
    assert res["closes"] != 0
    assert R.opening_holds(res)                                                             # everything committed is a polynomial and is opened honestly
    assert not R.identity_holds(res["publics"], res["values"], res["challenges"]) and not R.verify(res)
    assert not pl.identity_holds(cv, R.t.log_n, R.t.k[1], R.t.k[2], res["publics"], res["values"], res["challenges"])
    vk = pl.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)
    assert pl.host_check(vk, res["publics"], res["proof"]) == (pl.REJECTED, None)
    # t(zeta) bent until the identity holds is no value of the committed t: the opening refuses it
    ch, values = res["challenges"], list(res["values"])
    v = dict(zip(tref.ORDER + ("Z", "Zw", "Phi", "Phiw"), values))
    lw = ref.lagrange_weights(R.t, ch["zeta"])
    pi = -sum(x * lw[i] for i, x in enumerate(res["publics"])) % R.r
    values[tref.ORDER.index("t")] = R.bracket(v, ch["zeta"], pi, lw[0], ch) * pow(pow(ch["zeta"], R.t.n, R.r) - 1, -1, R.r) % R.r
    assert R.identity_holds(res["publics"], values, ch) and not R.opening_holds(res, values=values) and not R.verify(res, values=values)
    # every other booking of the row fails as well: unweighted on the XOR row, on the range table's first row, nowhere
    for j, w in ((R.rows.index((2, 1, 1, 0)), 2), (0, 1), (0, 0)):
        m, _ = R.multiplicities(wires)
        m[j] += w
        assert not R.verify(R.prove(wit, BLIND, multiplicities=m, force=True)), (j, w)


def test_the_same_cheat_is_accepted_over_the_concatenated_single_table(pl):
    """what this feature removes: one table holding the range rows and the XOR rows, q_K = 1 on every lookup"""
    cv = "BN128"
    n_vars, public, gates, tables, wit, row = _cheat(cv)
    gates = dict(gates, qK=[1 if q else 0 for q in gates["qK"]])
    table = [tref.pad(t) for tab in tables for t in tab]
    R = lref.Reference(cv, n_vars, public, gates, table, TAU[cv], _point(cv))
    wires = R.wires_of(wit)
    assert (wires["a"][row], wires["b"][row], wires["c"][row]) == (1, 1, 0) and R.qk[row] == 1
    assert R.multiplicities(wires)[1] == []                                                # the range check of 1, 1, 0 finds the XOR row
    res = R.prove(wit, BLIND)
    assert R.identity_holds(res["publics"], res["values"], res["challenges"]) and R.opening_holds(res)
    vk = pl.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)
    assert not vk.tagged and pl.host_check(vk, res["publics"], res["proof"])[0] == pl.ACCEPTED
