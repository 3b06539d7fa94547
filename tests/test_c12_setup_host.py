"""The restatement of the reference's compressor12 setup (tests/c12_setup_ref.py) on hand-sized circuits whose answers are
worked out here, its .exec writer against oracle/compressor12.py's reader, and the R1CS helper against itself.  No GPU."""
import pathlib, sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import compressor12 as C12  # noqa: E402
import c12_setup_ref as REF  # noqa: E402

P = REF.P


def circuit(constraints, n_wires=10):
    return {"num_inputs": 3, "num_outputs": 0, "num_variables": n_wires, "constraints": constraints, "custom_gates": [], "custom_gates_uses": []}


def test_one_multiplication():
    """(2 w1 + 3) * (5 w2) = 7 w3 + 1: qm = 10, ql = 2*0 = 0, qr = 3*5, qo = -7, qc = 3*0 - 1"""
    pg, pa = REF.r1cs2plonk(circuit([([(0, 3), (1, 2)], [(2, 5)], [(0, 1), (3, 7)])]))
    assert pa == [] and pg == [(1, 2, 3, 10, 0, 15, P - 7, P - 1)]


def test_sum_of_five_terms_gives_two_additions_in_order():
    """A = 0, C = 2 w1 + 3 w2 + 4 w3 + 5 w4 + 6 w5 + 9: terms leave the front in wire order, the sums join at the back:
    (w1, w2) -> w10, then (w3, w4) -> w11, leaving [w5, w10, w11]"""
    pg, pa = REF.r1cs2plonk(circuit([([], [], [(5, 6), (1, 2), (0, 9), (3, 4), (2, 3), (4, 5)])]))
    assert pa == [(1, 2, 2, 3), (3, 4, 4, 5)]
    assert pg == [(1, 2, 10, 0, P - 2, P - 3, 1, 0), (3, 4, 11, 0, P - 4, P - 5, 1, 0), (5, 10, 11, 0, 6, 1, 1, 9)]


def test_constant_times_b():
    """A = 4 (a constant), B = w1 + 2 w2, C = 3 w2 + w3: the sum 4 B + C (r1cs2plonk.rs:209-211 joins with +)"""
    pg, pa = REF.r1cs2plonk(circuit([([(0, 4)], [(1, 1), (2, 2)], [(2, 3), (3, 1)])]))
    assert pa == [] and pg == [(1, 2, 3, 0, 4, 11, 1, 0)]


def test_a_is_zero():
    """A has only a zero coefficient: the constraint is C = 0 whatever B is; unused slots are wire 0 with coefficient 0"""
    pg, pa = REF.r1cs2plonk(circuit([([(1, 0)], [(2, 5)], [(0, 8), (4, 3)])]))
    assert pa == [] and pg == [(4, 0, 0, 0, 3, 0, 0, 8)]


def test_rows_of_a_hand_sized_circuit():
    """three equal multiplications: one row holds two of them in its first half and the third, repeated, in its second"""
    mul = lambda a, b, c: ([(a, 1)], [(b, 1)], [(c, 1)])
    r = circuit([mul(1, 2, 3), mul(3, 4, 5), mul(5, 6, 7)])
    s = REF.plonk_setup(r, [0] * 372)
    assert (s["n_publics"], s["n_used"], s["n_bits"], s["n_const"]) == (2, 2, 1, 31)
    assert [s["s_map"][c][0] for c in range(12)] == [1, 2] + [0] * 10
    assert [s["s_map"][c][1] for c in range(12)] == [1, 2, 3, 3, 4, 5, 5, 6, 7, 5, 6, 7]
    row = s["const"][1]
    assert row[13:25] == [0, 0, P - 1, 1, 0, 0, 0, 0, P - 1, 1, 0, 0] and row[25:31] == [0, 0, 1, 0, 0, 0]
    assert s["const"][0][0] == 1 and s["const"][1][0] == 0                     # L1
    # wire 1: cells (0,0) and (1,0) swap their identities; wire 5 sits in three cells of row 1
    w = REF.root_of_unity(1); k = REF.K
    assert s["const"][0][1] == w and s["const"][1][1] == 1
    ident = lambda i, j: pow(w, i, P) * pow(k, j, P) % P
    assert [row[1 + 6], row[1 + 9], row[1 + 5]] == [ident(1, 5), ident(1, 6), ident(1, 9)]


def test_exec_writer_round_trip():
    adds = [(1, 2, 5, P - 1), (3, 11, 1, 7)]
    s_map = [[c * 3 + i for i in range(3)] for c in range(12)]
    text = REF.write_exec(adds, s_map)
    assert text == C12.write_exec(adds, s_map) and " " not in text
    n_adds, n_rows, a, m = C12.read_exec(text)
    assert (n_adds, n_rows) == (2, 3)
    assert [a[2] * C12.RINV % P, a[3] * C12.RINV % P, a[7] * C12.RINV % P] == [5, P - 1, 7]
    assert [m[12 * i + c] for c in range(12) for i in range(3)] == [v for col in s_map for v in col]


def test_r1cs_helper_round_trip():
    cons = [([(2, 5), (1, 3)], [(0, 1)], [(3, P - 1)]), ([], [], [(4, 2)])]
    gates = [("CMulAdd", []), ("FFT4", [3, 5, 7, 4])]
    uses = [(0, list(range(1, 13))), (1, [(1 << 32) + 5] + list(range(1, 24)))]
    for order in (None, [5, 2, 4, 1, 3]):
        r = REF.read_r1cs(REF.write_r1cs(30, 1, 2, 26, cons, gates, uses, section_order=order))
        assert (r["num_inputs"], r["num_outputs"], r["num_variables"]) == (4, 1, 30)
        assert r["constraints"][0] == ([(1, 3), (2, 5)], [(0, 1)], [(3, P - 1)]) and r["constraints"][1] == ([], [], [(4, 2)])
        assert r["custom_gates"] == gates and r["custom_gates_uses"] == uses


def test_poseidon_rows_end_in_the_hash(orc):
    """the row states the Poseidon12 proof test uses (tests/c12_setup_circuits.py, the project's constants and matrix): the
    31st row is the Poseidon-Goldilocks permutation of the first, so its first four lanes are the oracle's hash"""
    import numpy as np
    import c12_setup_circuits as CC
    state = [(i * 0x9E3779B97F4A7C15 + 1) % P for i in range(12)]
    rows = CC.poseidon_rows(state)
    assert len(rows) == 31
    assert [int(v) for v in orc.poseidon(np.array(state[:8], np.uint64), np.array(state[8:], np.uint64), 12)] == rows[30]
