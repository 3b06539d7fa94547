"""groth16_key_check --ptau without a GPU: the identities of the randomised check in the exponent, over Fr alone -- they pin
the root of unity, the 1/m of the inverse transform, bellman's dummy input rows, the density order of a and b and the public / other
split before any kernel is believed --, the plain-Python yardstick of the GPU tests on keys whose answer is known by construction, and
the surface: the command line's parser, the finding lines, the header."""
import importlib.util, pathlib, random, sys
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle")); sys.path.insert(0, str(ROOT / "tools"))
import groth16 as G  # noqa: E402
import key_check_srs_ref as KS  # noqa: E402
CURVES = ("bn254", "bls12_381")


@pytest.fixture(scope="module")
def g16(orc):
    return {cv: G.Groth16Oracle(orc, cv) for cv in CURVES}


def _columns_at_tau(g, cir, tau):
    """a_j(tau), b_j(tau), c_j(tau) = sum_i M[i, j] L_i(tau) with L_i(tau) = (tau^m - 1) w^i / (m (tau - w^i))"""
    r = g.r; m = 1 << cir["log_m"]; w = g.omega(cir["log_m"])
    zt = (pow(tau, m, r) - 1) % r
    L = [zt * pow(w, i, r) % r * pow(m * (tau - pow(w, i, r)) % r, -1, r) % r for i in range(m)]
    out = [[0] * cir["n_wires"] for _ in range(3)]
    for i, row in enumerate(cir["rows"]):
        for which in range(3):
            for j, cf in row[which]:
                out[which][j] = (out[which][j] + cf * L[i]) % r
    return out


def _coefficients(g, cir, which, rho, lo, hi):
    """u = the oracle's inverse transform of M (rho restricted to wires lo .. hi), as integers"""
    r = g.r; m = 1 << cir["log_m"]
    ptr, cols, cf = g.csr(cir["rows"], which)
    cf = g.fr_ints(g.from_mont(cf)) if len(cols) else []
    s = [0] * m
    for i in range(len(ptr) - 1):
        s[i] = sum(cf[k] * rho[cols[k]] for k in range(int(ptr[i]), int(ptr[i + 1])) if lo <= cols[k] < hi) % r
    return g.fr_ints(g.from_mont(g.ntt(g.to_mont(g.fr_array(s)), inverse=True)))


@pytest.mark.parametrize("cv", CURVES)
@pytest.mark.parametrize("n_mul", [6, 40])
def test_the_identities_of_the_check_hold_in_the_exponent(g16, cv, n_mul):
    g = g16[cv]; r = g.r; rng = random.Random(100 + n_mul)
    r1cs, _ = G.synthetic_r1cs(r, n_mul, seed=5)
    cir = g.circuit(r1cs)
    ni, nw, m = cir["num_inputs"], cir["n_wires"], 1 << cir["log_m"]
    tau, alpha, beta, gamma, delta = (rng.randrange(2, r) for _ in range(5))
    rho = [rng.getrandbits(128) for _ in range(nw)]
    at, bt, ct = _columns_at_tau(g, cir, tau)
    pw = [pow(tau, t, r) for t in range(2 * m - 1)]
    at_tau = lambda u: sum(x * p for x, p in zip(u, pw)) % r
    u = {(which, part): _coefficients(g, cir, which, rho, lo, hi) for which in range(3) for part, lo, hi in (("pub", 0, ni), ("aux", ni, nw))}
    # a and b: the whole query against tauG1, and the section's entries are the wires of the density order, none left out that counts
    wires = KS.wires(g, r1cs)
    for which, col, name in ((0, at, "a"), (1, bt, "b_g1")):
        whole = [(x + y) % r for x, y in zip(u[(which, "pub")], u[(which, "aux")])]
        assert sum(rho[j] * col[j] for j in range(nw)) % r == at_tau(whole)
        assert [j for j in range(nw) if col[j]] == wires[name]
        assert sum(rho[j] * col[j] for j in wires[name]) % r == at_tau(whole)
    if n_mul == 40:
        assert wires["a"] != list(range(len(wires["a"])))                      # an aux wire without A-density: the map is not the identity
    # ic and l: gamma sum rho_j ic_j = X_pub, delta sum rho_j l_j = X_aux, with X_S = sum_t (u^B alpha + u^A beta + u^C) tau^t
    ext = [(beta * at[j] + alpha * bt[j] + ct[j]) % r for j in range(nw)]
    for part, lo, hi, k in (("pub", 0, ni, gamma), ("aux", ni, nw, delta)):
        q = [ext[j] * pow(k, -1, r) % r for j in range(nw)]                    # ic_j or l_(j - ni)
        x = (alpha * at_tau(u[(1, part)]) + beta * at_tau(u[(0, part)]) + at_tau(u[(2, part)])) % r
        assert k * sum(rho[j] * q[j] for j in range(lo, hi)) % r == x
    assert ext[nw - 1] == 0                                                    # the wire no row mentions: infinity in l, nothing on either side
    # h: delta sum rho'_i h_i = sum rho'_i (tau^(i + m) - tau^i), as one sum over 2m - 1 powers with the scalars (-rho' | 0 | rho')
    rho2 = [rng.getrandbits(128) for _ in range(m - 1)]
    h = [pw[i] * (pow(tau, m, r) - 1) % r * pow(delta, -1, r) % r for i in range(m - 1)]
    sc = [(-x) % r for x in rho2] + [0] + rho2
    assert len(sc) == 2 * m - 1
    assert delta * sum(x * y for x, y in zip(rho2, h)) % r == sum(x * p for x, p in zip(sc, pw)) % r
    # the oracle's own key generation sees the same columns
    T = g.setup(r1cs, tau, alpha, beta, gamma, delta)["trapdoor"]
    assert (T["at"], T["bt"], T["ct"]) == (at, bt, ct)


@pytest.mark.parametrize("cv", CURVES)
def test_the_yardstick_answers_by_construction(g16, cv):
    g = g16[cv]; r = g.r; rng = random.Random(7)
    r1cs, _ = G.synthetic_r1cs(r, 40, seed=5)
    td = tuple(rng.randrange(2, r) for _ in range(5))
    pb = g.params_bytes(g.setup(r1cs, *td))
    assert KS.report(g, r1cs, pb, td) == dict(counts=dict(query_mismatch=0, vk_mismatch=0), findings=[])
    w = KS.wires(g, r1cs)
    n_a = len(KS.split_key(g, pb)["a"])
    k = n_a - 2                                                                # among the aux wires, where the density order has skipped one
    assert w["a"][k] != k
    rep = KS.report(g, r1cs, KS.swap(g, pb, "a", k, k + 1), td)
    assert rep == dict(counts=dict(query_mismatch=1, vk_mismatch=0), findings=[dict(kind="query_mismatch", section="a", first_index=k, wire=w["a"][k])])
    # another alpha: alpha_g1, and with it ic and l from their first entries on; h has no wire
    other = g.params_bytes(g.setup(r1cs, td[0], td[1] + 1, *td[2:]))
    rep = KS.report(g, r1cs, KS.swap(g, other, "h", 3, 4), td)
    ni = g.circuit(r1cs)["num_inputs"]
    assert rep["findings"] == [dict(kind="query_mismatch", section="ic", first_index=0, wire=0), dict(kind="query_mismatch", section="l", first_index=0, wire=ni),
                               dict(kind="query_mismatch", section="h", first_index=3), dict(kind="vk_mismatch", field="alpha_g1")]
    assert rep["counts"] == dict(query_mismatch=3, vk_mismatch=1)


def _cli():
    spec = importlib.util.spec_from_file_location("zkgpu_prove_for_key_check_srs", ROOT / "tools" / "zkgpu_prove.py")
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def test_the_command_line_takes_ptau_and_no_other_command_changed(monkeypatch):
    import argparse
    monkeypatch.setenv("COLUMNS", "100")                                       # the help is wrapped to the terminal
    p = _cli().build_parser()
    a = p.parse_args(["groth16_key_check", "--r1cs", "c.r1cs", "-p", "k.key", "--ptau", "pot.ptau", "--no-check-srs"])
    assert a.ptau == "pot.ptau" and a.no_check_srs is True
    a = p.parse_args(["groth16_key_check", "--r1cs", "c.r1cs", "-p", "k.key"])
    assert a.ptau is None and a.no_check_srs is False
    sub = next(x for x in p._actions if isinstance(x, argparse._SubParsersAction))
    helps = {name: sp.format_help() for name, sp in sub.choices.items()}
    assert "--ptau FILE" in helps["groth16_key_check"] and "--no-check-srs" in helps["groth16_key_check"]
    # every other sub-command's help as it was before --ptau (recorded from the commit before this feature)
    golden = (ROOT / "tests" / "golden" / "key_check_srs" / "cli_help_other_commands.txt").read_text()
    assert "".join("== %s\n%s" % (c, helps[c]) for c in sorted(helps) if c != "groth16_key_check") == golden


def test_the_finding_lines_and_the_header():
    spec = importlib.util.spec_from_file_location("key_check_lines_for_srs", ROOT / "eigen-zkvm_amd" / "key_check_lines.py")
    L = importlib.util.module_from_spec(spec); spec.loader.exec_module(L)
    assert L.key_check_srs_line(dict(kind="query_mismatch", section="b_g1", first_index=7, wire=9)) == \
        "query_mismatch: section b_g1 is not the circuit's over this powers-of-tau file, first at index 7 (wire 9)"
    assert L.key_check_srs_line(dict(kind="query_mismatch", section="h", first_index=3)) == \
        "query_mismatch: section h is not the circuit's over this powers-of-tau file, first at index 3"
    assert L.key_check_srs_line(dict(kind="vk_mismatch", field="alpha_g1")) == "vk_mismatch: alpha_g1 differs from the powers-of-tau file's"
    h = " ".join((ROOT / "include" / "zkgpu.h").read_text().split())
    assert ("char* zk_groth16_key_check_srs(const char* curve, const void* r1cs, size_t r1cs_len, const void* params, size_t params_len, "
            "const zk_srs_t* srs, const uint8_t* seed, uint32_t max_findings);") in h
