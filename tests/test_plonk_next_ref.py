"""The model of the PLONK prover with a next-row term (tests/plonk_next_ref.py) against itself and against the HOST part of
eigen_zkvm_amd.plonk_next, without a GPU: the model's proof satisfies the verifier's field identity (the model's own and the package's,
written separately) and the opening equation in scalars under the known tau; each of the 16 values, each commitment's scalar, W1, W2, a
public input and every challenge moved does not.  The package's transcript gives the model's challenges byte for byte.  A point is stood in
for by its scalar's bytes here: only the transcript reads it.  Then the chain rule: the tables zk_plonk_<curve>_next_r1cs_new compiles (on the
host) equal the model's array for array."""
import importlib

import numpy as np
import pytest

import plonk_next_ref as nref
import plonk_r1cs_ref as rr
import r1cs_check_cases as cases

TAU = {"BN128": 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, "BLS12381": 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe}
PB = {"BN128": 64, "BLS12381": 96}
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(10)]
TERMS = {3: (False, 8), 5: (True, 16)}                        # number of terms -> (the sum twice, n)
CASES = [("BN128", 3, BLIND), ("BN128", 3, [0] * 10), ("BN128", 5, BLIND), ("BLS12381", 5, BLIND)]
IDS = lambda c: "%s-%d-%s" % (c[0], c[1], "blind" if any(c[2]) else "plain")


def circuit_of(cv, m):
    r = nref.R[cv]
    return nref.running_sums([(r - 1 - 3 * i, 1000 + 7 * i) for i in range(m)], r, twice=TERMS[m][0])


@pytest.fixture(scope="module")
def pn(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_next")


@pytest.fixture(scope="module")
def made():
    out = {}
    for cv, m, blind in CASES:
        n_vars, public, gates, wit = circuit_of(cv, m)
        R = nref.Reference(cv, n_vars, public, gates, TAU[cv], lambda s, cv=cv: s.to_bytes(PB[cv], "little"))
        out[(cv, m, tuple(blind))] = (R, R.prove(wit, blind))
    return out


def test_the_circuits_use_the_next_row_in_earnest():
    for m, (twice, n) in TERMS.items():
        n_vars, public, gates, wit = circuit_of("BN128", m)
        t = nref.Table("BN128", n_vars, public, gates)
        r = t.r
        assert t.n == n and len(wit) == n_vars
        rows = [i for i in range(t.n) if t.sel["qN"][i]]
        assert len(rows) == (2 if twice else 1) * ((m + 1) // 2) and all(t.sel["qN"][i] == r - 1 for i in rows)
        assert any(i + 1 in rows for i in rows)                                        # a chain that crosses rows
        closing = [i + 1 for i in rows if i + 1 not in rows]                           # where a chain lands
        assert t.sel["qM"][closing[0]] == 1 and t.sel["qO"][closing[0]] == r - 1       # in a closing gate
        if twice:
            assert all(t.sel[k][closing[1]] == 0 for k in nref.SELECTORS)              # in a row of its own
        assert t.sel["qN"][t.n - 1] == 0 and not any(t.sel["qN"][:t.l])
        R = nref.Reference("BN128", n_vars, public, gates, TAU["BN128"], lambda s: s.to_bytes(64, "little"))
        wires = R.wires_of(wit)
        assert not R.gates_hold(wires, [wit[public[0]]])
        # a chain's auxiliary moved in c of row i + 1 alone, where that row does not read c: row i fails, and only through its next-row term
        i = rows[0]
        assert t.sel["qO"][i + 1] in (0, 1)
        wires["c"][i + 1] = (wires["c"][i + 1] + 1) % r
        bad = R.gates_hold(wires, [wit[public[0]]])
        assert i in bad and set(bad) <= {i, i + 1}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_model_proof_holds_and_every_mutation_does_not(pn, made, case):
    cv, m, blind = case
    R, res = made[(cv, m, tuple(blind))]
    r = R.r
    ch, values, publics = res["challenges"], res["values"], res["publics"]
    ident = lambda x, v, c, k2=R.t.k[2]: pn.identity_holds(cv, R.t.log_n, R.t.k[1], k2, x, v, c)
    assert len(values) == 16 and R.identity_holds(publics, values, ch) and ident(publics, values, ch) and R.opening_holds(res)
    for i in range(16):
        moved = list(values)
        moved[i] = (moved[i] + 1) % r
        assert not R.identity_holds(publics, moved, ch), i
        assert not ident(publics, moved, ch), i
        assert not R.opening_holds(res, values=moved), i
    other = [(publics[0] + 1) % r]
    assert not R.identity_holds(other, values, ch) and not ident(other, values, ch)
    for name in ("beta", "gamma", "alpha", "zeta"):
        assert not ident(publics, values, dict(ch, **{name: (ch[name] + 1) % r})), name
    assert not ident(publics, values, ch, k2=R.t.k[1])
    for i in range(14):                                                                # each commitment's scalar
        f = list(res["f_tau"])
        f[i] = (f[i] + 1) % r
        assert not R.opening_holds(res, f_tau=f), i
    assert not R.opening_holds(res, w1=(res["w1"] + 1) % r) and not R.opening_holds(res, w2=(res["w2"] + 1) % r)
    assert not R.opening_holds(res, gamma=(ch["gamma_open"] + 1) % r) and not R.opening_holds(res, z=(ch["z_open"] + 1) % r)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_package_transcript_and_host_check_agree_with_the_model(pn, made, case):
    cv, m, blind = case
    R, res = made[(cv, m, tuple(blind))]
    r = R.r
    vk = pn.VerifyingKey(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points)
    assert vk.digest == R.vkd and len(R.vk_points) == 9
    assert pn.challenges(vk, res["publics"], res["proof"]) == res["challenges"]
    verdict, tup = pn.host_check(vk, res["publics"], res["proof"])
    assert verdict == pn.ACCEPTED
    cs, sets, ys, g, z, W1, W2 = tup
    assert (sets, ys, g, z) == (res["sets"], res["ys"], res["challenges"]["gamma_open"], res["challenges"]["z_open"])
    assert cs == R.vk_points + [res["proof"][k] for k in ("A", "B", "C", "T", "Z")] and (W1, W2) == (res["proof"]["W1"], res["proof"]["W2"])
    assert z not in sets[11] and len(sets[11]) == len(sets[13]) == 2 and sets[11] == sets[13]          # c and Z on {zeta, zeta w}
    values = res["proof"]["values"]
    for i in range(16):
        moved = dict(res["proof"], values=values[:i] + [(values[i] + 1) % r] + values[i + 1:])
        assert pn.host_check(vk, res["publics"], moved) == (pn.REJECTED, None), i
    assert pn.host_check(vk, [(res["publics"][0] + 1) % r], res["proof"]) == (pn.REJECTED, None)
    assert pn.host_check(vk, res["publics"], dict(res["proof"], values=values[:15] + [r])) == (pn.INPUT_NOT_CANONICAL, None)
    assert pn.host_check(vk, [r], res["proof"]) == (pn.INPUT_NOT_CANONICAL, None)
    with pytest.raises(pn.ZkError, match="plonk next: a proof holds 16 values"):
        pn.host_check(vk, res["publics"], dict(res["proof"], values=values[:15]))
    with pytest.raises(pn.ZkError, match="point W2 of the proof is"):
        pn.host_check(vk, res["publics"], dict(res["proof"], W2=res["proof"]["W2"][:-1]))
    data = pn.proof_to_bytes(res["proof"])
    assert len(data) == 7 * PB[cv] + 16 * 32 and pn.proof_from_bytes(data, PB[cv]) == res["proof"]
    with pytest.raises(pn.ZkError, match="a proof is %d bytes" % len(data)):
        pn.proof_from_bytes(data[:-1], PB[cv])
    assert pn.challenges(vk, [(res["publics"][0] + 1) % r], res["proof"])["beta"] != res["challenges"]["beta"]
    # the domain strings are this protocol's own: plonk.py's transcript over the same bytes draws other challenges
    plonk = importlib.import_module("eigen_zkvm_amd.plonk")
    assert plonk.vk_digest(cv, R.t.log_n, R.t.l, R.t.k[1], R.t.k[2], R.vk_points) != R.vkd
    assert plonk.transcript_start(cv, R.vkd, res["publics"]) != pn.transcript_start(cv, R.vkd, res["publics"])


# ---- the chain rule -----------------------------------------------------------------------------------------------------------------------
def _long_row(field, m):
    """one linear constraint of m signals and one product constraint whose A side has m signals -> (r1cs bytes, witness)"""
    p = rr.R[field]
    w = [1] + [(5 + 11 * i) % p for i in range(m)]
    s = sum((i + 2) * w[i + 1] for i in range(m)) % p
    w += [s, 3, 3 * s % p]
    lc = [(i + 1, i + 2) for i in range(m)]
    cons = [(lc, [(0, 1)], [(m + 1, 1)]), (lc, [(m + 2, 1)], [(m + 3, 1)])]
    return cases.write(field, len(w), cons), w


def _tables_equal(c, t, m):
    ints = lambda a: [int.from_bytes(np.ascontiguousarray(row).tobytes(), "little") for row in a]
    for k in nref.SELECTORS:
        assert ints(c.gates[k]) == t[k], k
    for k in "abc":
        assert c.gates[k].tolist() == t[k], k
    assert c.origin.tolist() == t["origin"]
    s = c.segments
    assert (s["seg_first"].tolist(), s["seg_ptr"].tolist(), s["seg_wire"].tolist(), ints(s["seg_coef"])) == (t["seg_first"], t["seg_ptr"], t["seg_wire"], t["seg_coef"])
    assert c.info == {"n_wires": m.n_wires, "n_public": m.n_public, "n_constraints": m.n_constraints, "n_gates": m.n_gates, "n_aux": m.n_aux, "n_segments": len(m.segments),
                      "max_segment_terms": max([len(x) for _, x in m.segments] or [0]), "n_segment_terms": len(t["seg_wire"])}


@pytest.mark.parametrize("field", rr.FIELDS)
def test_the_chain_tables_are_the_models_array_for_array(pn, field):
    seen = []
    for name, data, w, _ in rr.circuits(field):
        m, old = nref.Compiled(data, field), rr.Compiled(data, field)
        c = pn.NextR1csCircuit(data, field)
        try:
            _tables_equal(c, m.tables(), m)
            assert isinstance(c, pn.R1csCircuit) and isinstance(c, pn.NextCircuit) and c.has_next
            assert m.n_gates <= old.n_gates and m.n_aux <= old.n_aux, name             # never more gates than the rule of fan-in 2
            assert not m.failing_gates(m.extend(w)), name
            assert m.n_gates == 0 or m.gates["qN"][-1] == 0, name                     # the last real row never reads the next
            assert not c.sel["qN"][c.n_public + c.n_gates - 1].any() and not c.sel["qN"][:c.n_public].any()
            seen.append(name)
        finally:
            c.free()
    assert seen[:3] == ["products", "shapes", "one_constraint"] and len(seen) == 4
    data, w, _, _ = cases.shapes(field)
    m, old = nref.Compiled(data, field), rr.Compiled(data, field)
    assert m.n_gates < old.n_gates // 2 + 20 and m.n_aux < old.n_aux // 2 + 20        # the 1000-term row in half the gates


@pytest.mark.parametrize("field", rr.FIELDS)
@pytest.mark.parametrize("m_terms", (3, 4, 5, 253, 254))
def test_long_rows_take_half_the_gates(pn, field, m_terms):
    data, w = _long_row(field, m_terms)
    m = nref.Compiled(data, field)
    c = pn.NextR1csCircuit(data, field)
    try:
        _tables_equal(c, m.tables(), m)
    finally:
        c.free()
    lin = [g for g, o in enumerate(m.origin) if o == 0]
    k = (m_terms + 2) // 2                                                             # the linear constraint has m + 1 signals: ceil((m + 1) / 2) rows
    assert len(lin) == k and m.gates["qN"][lin[-1]] == 0 and all(m.gates["qN"][g] == m.p - 1 for g in lin[:-1])
    prod = [g for g, o in enumerate(m.origin) if o == 1]
    assert len(prod) == (m_terms + 1) // 2 + 2                                         # the chain, its landing row (C is one signal), the closing gate
    land = prod[-2]
    assert all(m.gates[s][land] == 0 for s in nref.SELECTORS) and m.gates["c"][land] == m.gates["a"][prod[-1]]
    if m_terms == 254:
        assert (m_terms + 1) // 2 <= 128                                               # a constraint of 254 terms: at most 128 gates for the sum
        assert len(lin) <= 128
    ext = m.extend(w)
    assert not m.failing_gates(ext)
    ext[m.gates["c"][lin[1]]] = (ext[m.gates["c"][lin[1]]] + 1) % m.p                  # one auxiliary of the closed chain wrong
    assert m.failing_gates(ext)[0] == lin[0]                                           # seen by the row before it, through q_N


def test_a_product_with_chains_on_all_three_sides_needs_no_landing_row(pn):
    field = "BN128"
    p = rr.R[field]
    w = [1] + list(range(2, 14))
    A, B, C = [(1, 2), (2, 3), (3, 5)], [(4, 1), (5, p - 1), (6, 7), (7, 1)], [(8, 1), (9, 1), (10, 1), (11, 1), (12, 1)]
    ev = lambda lc: sum(c * w[j] for j, c in lc) % p
    w.append((ev(A) * ev(B) - ev(C)) % p)
    C = C + [(13, 1)]
    data = cases.write(field, len(w), [(A, B, C)])
    m = nref.Compiled(data, field)
    assert m.n_gates == 2 + 2 + 3 + 1 and m.n_aux == 7 and not m.failing_gates(m.extend(w))
    assert m.gates["qN"] == [p - 1] * 7 + [0]
    assert m.gates["c"][2] == m.gates["a"][7] and m.gates["c"][4] == m.gates["b"][7] and m.gates["c"][7] == m.n_vars - 1     # each lands in the next
    c = pn.NextR1csCircuit(data, field)
    try:
        _tables_equal(c, m.tables(), m)
    finally:
        c.free()
    with pytest.raises(pn.ZkError, match="constraint 0 is 0 = k with k not zero"):
        pn.NextR1csCircuit(cases.write(field, 2, [([], [], [(0, 1)])]), field)
