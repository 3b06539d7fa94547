"""The plain-integer model of the R1CS import (tests/plonk_r1cs_ref.py) checked against the rule's own promises, without a
GPU: on products(f, 37), shapes(f), one_constraint(f) and the reference's multiplier.r1cs the extended witness satisfies every gate, a
corrupted output wire breaks only gates of that constraint, a constraint 0 = 5 is refused, duplicate wires and zero coefficients normalise
away, and wire 0 never stands under a non-zero selector."""
import pytest

import plonk_r1cs_ref as model
import r1cs_check_cases as cases

FIELDS, circuits = model.FIELDS, model.circuits


@pytest.mark.parametrize("field", FIELDS)
def test_the_extended_witness_satisfies_every_gate_and_a_wrong_output_breaks_its_constraint_alone(field):
    for name, data, w, outs in circuits(field):
        m = model.Compiled(data, field)
        full = m.extend(w)
        assert len(full) == m.n_vars == m.n_wires + m.n_aux and full[:m.n_wires] == w, name
        assert m.failing_gates(full) == [], name
        assert len(m.origin) == m.n_gates and m.origin == sorted(m.origin) and all(0 <= o < m.n_constraints for o in m.origin), name
        for wire, con in outs:
            bad = m.failing_gates(m.extend(cases.corrupt(w, wire, p=m.p)))
            assert bad and {m.origin[g] for g in bad} == {con}, (name, wire)
        # wire 0 never stands under a non-zero selector; every operand is a variable
        g = m.gates
        for i in range(m.n_gates):
            assert all(0 <= g[k][i] < m.n_vars for k in "abc")
            assert not (g["a"][i] == 0 and (g["qL"][i] or g["qM"][i])) and not (g["b"][i] == 0 and (g["qR"][i] or g["qM"][i])) and not (g["c"][i] == 0 and g["qO"][i]), (name, i)
        # every auxiliary is defined once, by a segment over original wires
        ids = [first + j for first, terms in m.segments for j in range(len(terms) - 1)]
        assert ids == list(range(m.n_wires, m.n_vars)), name
        assert all(0 < s < m.n_wires and 0 < c < m.p for _, terms in m.segments for s, c in terms), name


@pytest.mark.parametrize("field", FIELDS)
def test_the_figures_of_shapes(field):
    data, w, long_row, cw = cases.shapes(field)
    m = model.Compiled(data, field)
    assert (m.n_gates, m.n_aux, len(m.segments), max(len(t) for _, t in m.segments)) == (1046, 1039, 10, 999)
    assert set(range(m.n_constraints)) - set(m.origin) == {0}                         # A = B = C = empty emits nothing
    bad = m.failing_gates(m.extend(cases.corrupt(w, cw, p=m.p)))
    assert bad == [m.n_gates - 1]                                                     # the last wire breaks exactly the last gate


@pytest.mark.parametrize("field", FIELDS)
def test_normalisation_and_refusals(field):
    p = model.R[field]
    # 0 = 5: (0) * (0) = 5 on wire 0; and a linear constraint whose signals cancel, leaving 3 = 0
    with pytest.raises(model.Refused, match="constraint 1 is 0 = "):
        model.Compiled(cases.write(field, 4, [([(1, 1)], [(2, 1)], [(3, 1)]), ([], [], [(0, 5)])]), field)
    with pytest.raises(model.Refused, match="constraint 0 is 0 = 3"):
        model.Compiled(cases.write(field, 4, [([(0, 1)], [(1, 2), (0, 3)], [(1, 2)])]), field)
    model.Compiled(cases.write(field, 4, [([(0, 1)], [(1, 2), (0, 3)], [(1, 2), (0, 3)])]), field)          # 0 = 0: nothing emitted, nothing refused
    with pytest.raises(model.Refused, match="wire 4 of 4"):
        model.Compiled(cases.write(field, 4, [([(4, 1)], [(2, 1)], [(3, 1)])]), field)
    other = "BLS12381" if field == "BN128" else "BN128"
    with pytest.raises(model.Refused, match="another field"):
        model.Compiled(cases.one_constraint(other), field)
    # duplicates add up, zeros drop out, wire 0 becomes the constant: (3 w1 + 0 w2 + 4 w1 + 2) * (w2 - w2 + w3 + 1) = w1 + 5
    data = cases.write(field, 4, [([(1, 3), (2, 0), (1, 4), (0, 2)], [(2, 1), (2, p - 1), (3, 1), (0, 1)], [(1, 1), (0, 5)])])
    m = model.Compiled(data, field)
    assert (m.n_gates, m.n_aux, m.segments) == (1, 0, [])
    assert [m.gates[k][0] for k in ("a", "b", "c")] == [1, 3, 1]
    assert [m.gates[k][0] for k in model.SELECTORS] == [7, 2, p - 1, 7, (2 - 5) % p]
    # a linear constraint of five signals: reduce(L, 3) folds the first three
    data = cases.write(field, 7, [([(0, 2)], [(1, 1), (2, 1), (3, 1), (4, 1), (0, 9)], [(5, 1), (0, 1)])])
    m = model.Compiled(data, field)
    assert m.segments == [(7, [(1, 2), (2, 2), (3, 2)])] and m.n_aux == 2 and m.n_gates == 3
    assert [(m.gates["a"][i], m.gates["b"][i], m.gates["c"][i]) for i in range(3)] == [(1, 2, 7), (7, 3, 8), (8, 4, 5)]
    assert [m.gates[k][2] for k in model.SELECTORS] == [1, 2, p - 1, 0, 17]
    w = [1, 10, 20, 30, 40, 0, 0]
    w[5] = (2 * (10 + 20 + 30 + 40 + 9) - 1) % p
    assert m.failing_gates(m.extend(w)) == []
