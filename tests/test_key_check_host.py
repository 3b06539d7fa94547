"""The plain-Python key checker (tests/key_check_ref.py) on hand-made inputs, and the finding lines of the command-line tool: no GPU.
The keys come from the oracle's generate_parameters restatement (oracle/groth16.py) with a fixed trapdoor."""
import importlib.util, json, pathlib, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import groth16 as G  # noqa: E402
import key_check_cases as KC  # noqa: E402
import key_check_ref as K  # noqa: E402
TD = [3, 5, 7, 11, 13]


@pytest.fixture(scope="module")
def key(orc):
    g = G.Groth16Oracle(orc, "bn254")
    r1cs, _ = KC.circuit(g.r, 8)
    return g, g.r1cs_bytes(r1cs), g.params_bytes(g.setup(r1cs, *TD))


def test_curve_model():
    for C in K.CURVES.values():
        for g in (0, 1):
            assert C.on_curve(C.gen[g], g) and C.mul(C.gen[g], C.r) is None
            p, x = None, 1
            while p is None: p = C.lift_x((x, 1 if g else 0), g); x += 1
            assert C.on_curve(p, g) and C.mul(p, C.order(g)) is None
            assert C.classify(C.coords(C.gen[g], g), g) is None and C.classify((0,) * (4 if g else 2), g) == "infinity"
            c = list(C.coords(C.gen[g], g)); c[0] += C.q
            assert C.classify(c, g) == "coordinate_range"
            c[0] -= C.q; c[-1] ^= 1
            assert C.classify(c, g) == "not_on_curve"
    C = K.BLS12381
    p = C.lift_x((4, 0), 0)
    assert C.classify(C.coords(p, 0), 0) == "not_in_subgroup" and C.classify(C.coords(C.mul(p, C.cofactor[0]), 0), 0) is None


def test_clean_key_and_each_kind_of_finding(key):
    g, rb, pb = key
    n = KC.layout("BN128", pb)["b_g1"][0]
    clean = K.report("BN128", rb, pb, b_indices=[0, n - 1])
    assert clean["findings"] == [] and clean["skipped"] == [] and clean["checked"]["pairs"] == 2 + n
    assert clean["sections"]["h"] == (1 << clean["domain_log"]) - 1 and clean["sections"]["ic"] == clean["n_public"] + 1
    rep = K.report("BN128", rb, KC.truncate("BN128", pb, "l", 1), b_indices=[])
    assert rep["findings"] == [dict(kind="size", section="l", have=clean["sections"]["l"] - 1, want=clean["sections"]["l"])]
    rep = K.report("BN128", rb, KC.off_curve("BN128", pb, "a", 2), b_indices=[])
    assert rep["findings"] == [dict(kind="not_on_curve", section="a", n_points=1, first_index=2)]
    rep = K.report("BN128", rb, KC.set_point("BN128", pb, "b_g2", 1, KC.twist_point_outside_subgroup("BN128")), b_indices=[])
    assert rep["findings"] == [dict(kind="not_in_subgroup", section="b_g2", n_points=1, first_index=1)]
    assert rep["skipped"] == [dict(check="g1_g2_mismatch", section="b", reason="an invalid point")]
    rep = K.report("BN128", rb, KC.doubled("BN128", pb, "b_g1", n - 1), b_indices=[0, n - 1])
    assert rep["findings"] == [dict(kind="g1_g2_mismatch", section="b", first_index=n - 1)]
    with pytest.raises(ValueError, match="proving key: (truncated file|trailing bytes)"):
        K.report("BN128", rb, pb[:-5])
    with pytest.raises(ValueError, match="proving key"):
        K.parse_key(K.BLS12381, pb)
    rep = K.report("BN128", rb, pb, b_indices=[], max_findings=1, vk_json=json.dumps(
        {"vk_alpha_1": {"x": "1", "y": "2"}, "vk_beta_2": {"x": ["1", "0"], "y": ["2", "0"]}, "vk_gamma_2": {"x": ["1", "0"], "y": ["2", "0"]},
         "vk_delta_2": {"x": ["1", "0"], "y": ["2", "0"]}, "IC": []}))
    assert rep["counts"]["vk_mismatch"] == 5 and [f["field"] for f in rep["findings"]] == ["vk_alpha_1"]


def test_finding_lines_are_the_tools():
    spec = importlib.util.spec_from_file_location("key_check_lines", ROOT / "eigen-zkvm_amd" / "key_check_lines.py")   # it imports nothing of the
    L = importlib.util.module_from_spec(spec); spec.loader.exec_module(L)                                           # package, which needs the library
    assert L.POINT_CLASSES == K.CLASSES
    fs = [dict(kind="size", section="h", have=3, want=7), dict(kind="infinity", section="l", n_points=1, first_index=4),
          dict(kind="not_on_curve", section="a", n_points=2, first_index=63), dict(kind="g1_g2_mismatch", section="b", first_index=9),
          dict(kind="vk_mismatch", field="vk_delta_2")]
    assert [L.key_check_line(f) for f in fs] == [K.finding_line(f) for f in fs]
    assert K.finding_line(fs[0]) == "size: section h has 3 points, the circuit needs 7 (the key of another circuit?)"
    assert K.finding_line(fs[2]) == "not_on_curve: section a: 2 points, first at index 63"
    s = dict(check="g1_g2_mismatch", section="b", reason="an invalid point")
    assert L.key_check_skipped_line(s) == K.skipped_line(s) == "skipped: g1_g2_mismatch of b: an invalid point"


def test_findings_are_listed_kind_by_kind(key):
    """not_on_curve in h, infinity in l: the sections come in the other order than the kinds, and the kinds decide"""
    g, rb, pb = key
    rep = K.report("BN128", rb, KC.set_point("BN128", KC.off_curve("BN128", pb, "h", 1), "l", 0, None), b_indices=[])
    assert [(f["kind"], f["section"]) for f in rep["findings"]] == [("infinity", "l"), ("not_on_curve", "h")]
