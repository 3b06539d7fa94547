"""The surface of the tagged lookups without a GPU: the header declares the four entry points and the library exports them,
the package binds them, every refusal of LookupCircuit(tables=...) comes back with its text, a circuit file round-trips with and without
table_tag, and the codecs of the tagged and the single-table protocol refuse each other's keys and proofs, in both directions, as
plonk.py, fflonk.py and fflonk_lookup.py refuse both."""
import importlib, json, pathlib, re

import numpy as np
import pytest

import plonk_lookup_ref as lref
import plonk_lookup_tagged_ref as tref
import plonk_ref as ref

ROOT = pathlib.Path(__file__).resolve().parent.parent
ENTRY_POINTS = ["zk_plonk_%s_lookup_tagged_%s" % (c, f) for c in ("bn254", "bls12_381") for f in ("table_new", "count_dev", "terms_dev", "quotient_dev")]
TAU, PB = 0x1f3a9c5b7d2e4f60718293a4b5c6d7e8f90a1b2c3d4e5f60718293a4b5c6d7e, 64
BLIND = [0x1111 * (i + 1) + (i << 200) for i in range(14)]


@pytest.fixture(scope="module")
def pl(zk):
    return importlib.import_module("eigen_zkvm_amd.plonk_lookup")


def test_header_declares_and_the_package_binds_the_entry_points(zk, pl):
    text = (ROOT / "include" / "zkgpu.h").read_text()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
    for macro, value in (("ZK_PLONK_LOOKUP_TAGGED_TERMS_COLS", 8), ("ZK_PLONK_LOOKUP_TAGGED_QUOTIENT_COLS", 10), ("ZK_PLONK_LOOKUP_MAX_TABLES", 65535)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    assert set(ENTRY_POINTS) <= set(zk.EXPORTS)
    lib = zk.lib()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    assert (pl.TAGGED_PROTOCOL, pl.TAGGED_N_VALUES, pl.TAGGED_N_FIXED, pl.TAGGED_FIXED[-1], pl.MAX_TABLES) == ("plonk-shplonk-lookup-tagged", 22, 13, "T0", 65535)
    assert pl.TAGGED_VALUE_NAMES[12:14] == ("T0", "a") and len(pl.TAGGED_VALUE_NAMES) == 22
    doc = pl.__doc__.replace("\n", " ")
    assert '"plonklt-vk"' in doc and '"plonklt-v1"' in doc and "several tables in one circuit" not in doc.split("Not built:")[1].split(".")[0]
    fl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup").__doc__.replace("\n", " ")
    assert "setup refuses a tagged circuit" in fl.split("Not built:")[1]
    # the library's refusals that need no device
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    big = np.frombuffer(ref.R["BN128"].to_bytes(32, "little"), dtype="<u8").astype(np.uint64)
    ptrs = np.zeros(10, dtype=np.uint64)
    assert not lib.zk_plonk_bn254_lookup_tagged_table_new(None, None, None, None, 4, None) and "null argument" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_tagged_count_dev(None, None, None, None, None, 0, None, None, None, None) != 0 and "null table" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_tagged_terms_dev(zk._ptr(ptrs), 8, zk._ptr(big), zk._ptr(one), None, None) != 0 and "eta is not below" in lib.zk_last_error().decode()
    assert lib.zk_plonk_bn254_lookup_tagged_quotient_dev(zk._ptr(ptrs), 27, *[zk._ptr(one)] * 3, None, None) != 0 and "exceeds the field's 2-adicity" in lib.zk_last_error().decode()


def _parts(r, steps=0):
    n_vars, public, gates, tables, wit = tref.tagged_chain(steps, r)
    return n_vars, public, {k: list(v) for k, v in gates.items()}, tables, wit


def test_every_refusal_of_the_circuit_class(pl):
    r = ref.R["BN128"]
    n_vars, public, gates, tables, wit = _parts(r)
    c = pl.LookupCircuit(n_vars, public, gates, tables=tables)
    assert c.tagged and (c.n, c.n_table, c.table_sizes) == (8, 7, [2, 5]) and c.table_tag.tolist() == [1, 1, 2, 2, 2, 2, 2] and c.table_tag.dtype == np.uint32
    assert c.tag_col[:, 0].tolist() == [1, 1, 2, 2, 2, 2, 2, 2] and not c.tag_col[:, 1:].any()         # padded with the last row's tag
    rows = [tuple(pl.pa.int_of(c.table[j][i]) for j in range(3)) for i in range(c.n)]
    assert rows[:2] == [(0, 0, 0), (1, 0, 0)] and rows[7] == rows[6] == (1, 1, 0)                       # short rows padded with zeros on the right
    one = pl.LookupCircuit(n_vars, public, dict(gates, qK=[min(q, 1) for q in gates["qK"]]), [tref.pad(t) for tab in tables for t in tab])
    assert not one.tagged and not hasattr(one, "table_tag")
    with pytest.raises(pl.ZkError, match="exactly one of the two"):
        pl.LookupCircuit(n_vars, public, gates, tables[1], tables=tables)
    with pytest.raises(pl.ZkError, match="exactly one of the two"):
        pl.LookupCircuit(n_vars, public, gates)
    with pytest.raises(pl.ZkError, match="row 1 of table 2 holds 4 values: a table row holds one, two or three"):       # a row wider than three
        pl.LookupCircuit(n_vars, public, gates, tables=[tables[0], [(0, 0, 0), (1, 2, 3, 4)]])
    with pytest.raises(pl.ZkError, match="row 0 of table 1 holds 0 values"):
        pl.LookupCircuit(n_vars, public, gates, tables=[[()], tables[1]])
    with pytest.raises(pl.ZkError, match="table 2 is empty: a table has at least one row"):             # an empty table
        pl.LookupCircuit(n_vars, public, gates, tables=[tables[0], []])
    with pytest.raises(pl.ZkError, match=r"tables= takes 2 \.\. 65535 tables, not 1 \(one table is table=\)"):          # K out of range, below
        pl.LookupCircuit(n_vars, public, gates, tables=[tables[1]])
    with pytest.raises(pl.ZkError, match=r"tables= takes 2 \.\. 65535 tables, not 65536"):              # and above
        pl.LookupCircuit(n_vars, public, gates, tables=[[(0,)]] * 65536)
    with pytest.raises(pl.ZkError, match="tables= is a sequence of tables"):
        pl.LookupCircuit(n_vars, public, gates, tables=5)

    class Huge(list):
        def __len__(self):
            return 1 << 26
    with pytest.raises(pl.ZkError, match=r"a table of %d rows does not fit n <= 2\^26 rows on BN128" % ((1 << 26) + 2)):  # sum T_k beyond the size limit
        pl.LookupCircuit(n_vars, public, gates, tables=[tables[0], Huge()])
    g = gates["qK"].index(2)
    for v in (3, r - 1):                                                                   # qK above K
        with pytest.raises(pl.ZkError, match=r"selector qK of gate %d names no table: the circuit has tables 1 \.\. 2 \(0 is no lookup\)" % g):
            pl.LookupCircuit(n_vars, public, dict(gates, qK=gates["qK"][:g] + [v] + gates["qK"][g + 1:]), tables=tables)
    with pytest.raises(pl.ZkError, match="selector qK of gate %d is not below" % g):
        pl.LookupCircuit(n_vars, public, dict(gates, qK=gates["qK"][:g] + [r] + gates["qK"][g + 1:]), tables=tables)
    with pytest.raises(pl.ZkError, match="table value 1 is not below"):
        pl.LookupCircuit(n_vars, public, gates, tables=[tables[0], [(0, r, 0)]])
    with pytest.raises(pl.ZkError, match="selector qK of gate %d is not 0 or 1" % g):      # the single-table circuit keeps its own rule
        pl.LookupCircuit(n_vars, public, gates, [tref.pad(t) for tab in tables for t in tab])
    assert pl.LookupCircuit(n_vars, public, gates, tables=[[(0,)]] * 3 + [[(1, 2)]]).table_tag.tolist() == [1, 2, 3, 4]
    # the package's padded tables, tags and selectors are the reference's
    R = tref.Reference("BN128", n_vars, public, gates, tables, 5, lambda s: s.to_bytes(64, "little"))
    assert [(int(t),) + row for t, row in zip(c.tag_col[:, 0], rows)] == R.rows and [pl.pa.int_of(w) for w in c.sel["qK"]] == R.qk


def test_a_circuit_file_round_trips_with_and_without_table_tag(pl, tmp_path):
    r = ref.R["BLS12381"]
    n_vars, public, gates, tables, wit = _parts(r, 1)
    c = pl.LookupCircuit(n_vars, public, gates, curve="BLS12381", tables=tables)
    c.save(tmp_path / "c.npz")
    with np.load(tmp_path / "c.npz") as z:
        assert z["table_tag"].shape == (7,) and z["table_tag"].dtype == np.uint32 and z["table"].shape == (7, 3, 4) and z["qK"].shape == (c.n_gates, 4)
        parts = {k: z[k] for k in z.files}
    d = pl.LookupCircuit.load(tmp_path / "c.npz", "BLS12381")
    assert d.tagged and (d.n_vars, d.public, d.n, d.n_table, d.table_sizes) == (c.n_vars, c.public, c.n, c.n_table, c.table_sizes)
    assert np.array_equal(c.table, d.table) and np.array_equal(c.tag_col, d.tag_col) and np.array_equal(c.table_tag, d.table_tag)
    assert all(np.array_equal(c.sel[k], d.sel[k]) for k in ref.SELECTORS + ("qK",)) and all(np.array_equal(c.wire[k], d.wire[k]) for k in "abc")
    # a file without table_tag loads as a circuit of one table, as before
    n_vars1, public1, gates1, table1, _ = lref.lookup_chain(1, r)
    one = pl.LookupCircuit(n_vars1, public1, gates1, table1, "BLS12381")
    one.save(tmp_path / "one.npz")
    with np.load(tmp_path / "one.npz") as z:
        assert "table_tag" not in z.files
    back = pl.LookupCircuit.load(tmp_path / "one.npz", "BLS12381")
    assert not back.tagged and np.array_equal(back.table, one.table)
    # the tagged file without its tags is a single-table circuit whose qK = 2 is refused; tags out of order are refused by name
    np.savez(tmp_path / "stripped.npz", **{k: v for k, v in parts.items() if k != "table_tag"})
    with pytest.raises(pl.ZkError, match="is not 0 or 1"):
        pl.LookupCircuit.load(tmp_path / "stripped.npz", "BLS12381")
    for bad in ([1, 1, 2, 2, 1, 2, 2], [2, 2, 2, 2, 2, 2, 2], [1, 1, 3, 3, 3, 3, 3], [1, 1, 2, 2, 2, 2]):
        np.savez(tmp_path / "bad.npz", **dict(parts, table_tag=np.asarray(bad, dtype=np.uint32)))
        with pytest.raises(pl.ZkError, match="table_tag of .* is not the tags 1 .. K of the table's 7 rows in order"):
            pl.LookupCircuit.load(tmp_path / "bad.npz", "BLS12381")


@pytest.fixture(scope="module")
def both():
    """(reference, its proof) of the tagged and of the single-table protocol over n = 8"""
    r, point = ref.R["BN128"], lambda s: s.to_bytes(PB, "little")
    n_vars, public, gates, tables, wit = tref.tagged_chain(0, r)
    T = tref.Reference("BN128", n_vars, public, gates, tables, TAU, point)
    n_vars1, public1, gates1, table1, wit1 = lref.lookup_chain(0, r)
    P = lref.Reference("BN128", n_vars1, public1, gates1, table1, TAU, point)
    return (T, T.prove(wit, BLIND)), (P, P.prove(wit1, BLIND))


def test_the_codecs_refuse_each_other_in_both_directions(zk, pl, both):
    (T, tres), (P, pres) = both
    cv = "BN128"
    tvk = pl.VerifyingKey(cv, T.t.log_n, T.t.l, T.t.k[1], T.t.k[2], T.vk_points)
    pvk = pl.VerifyingKey(cv, P.t.log_n, P.t.l, P.t.k[1], P.t.k[2], P.vk_points)
    assert tvk.tagged and not pvk.tagged
    # keys: asked for one protocol, the other is refused by name, before a point is read (the round trips themselves need the device:
    # tests/test_gpu_plonk_lookup_tagged.py)
    tjs, pjs = json.dumps({"protocol": pl.TAGGED_PROTOCOL, "curve": cv}), json.dumps({"protocol": pl.PROTOCOL, "curve": cv})
    with pytest.raises(pl.ZkError, match=r'plonk lookup: a verification key of the single-table protocol \("plonk-shplonk-lookup"\), not of the tagged protocol'):
        pl.vk_from_json(pjs, tagged=True)
    with pytest.raises(pl.ZkError, match=r'plonk lookup: a verification key of the tagged protocol \("plonk-shplonk-lookup-tagged"\), not of the single-table protocol'):
        pl.vk_from_json(tjs, tagged=False)
    with pytest.raises(pl.ZkError, match=r"holds 12 commitments \(13 when its tables are tagged\), not 14"):
        pl.VerifyingKey(cv, 3, 1, 2, 3, T.vk_points + T.vk_points[:1])
    # proofs
    tp, pp = tjs, pjs
    with pytest.raises(pl.ZkError, match=r'plonk lookup: a proof of the single-table protocol \("plonk-shplonk-lookup"\), not of the tagged protocol'):
        pl.proof_from_json(pp, cv, tagged=True)
    with pytest.raises(pl.ZkError, match=r'plonk lookup: a proof of the tagged protocol \("plonk-shplonk-lookup-tagged"\), not of the single-table protocol'):
        pl.proof_from_json(tp, cv, tagged=False)
    with pytest.raises(pl.ZkError, match="a proof is"):
        pl.proof_from_bytes(pl.proof_to_bytes(pres["proof"]), PB, tagged=True)
    with pytest.raises(pl.ZkError, match="a proof is"):
        pl.proof_from_bytes(pl.proof_to_bytes(tres["proof"]), PB)
    # the verifier's host part: a proof of the one under a key of the other
    assert pl.host_check(tvk, tres["publics"], tres["proof"])[0] == pl.ACCEPTED and pl.host_check(pvk, pres["publics"], pres["proof"])[0] == pl.ACCEPTED
    with pytest.raises(pl.ZkError, match="a proof holds 22 values, not 21"):
        pl.host_check(tvk, pres["publics"], pres["proof"])
    with pytest.raises(pl.ZkError, match="a proof holds 21 values, not 22"):
        pl.host_check(pvk, tres["publics"], tres["proof"])
    cut = dict(tres["proof"], values=tres["proof"]["values"][:12] + tres["proof"]["values"][13:])      # T0(zeta) dropped: other challenges, another identity
    assert pl.host_check(pvk, pres["publics"], cut) == (pl.REJECTED, None)
    # plonk.py, fflonk.py and fflonk_lookup.py refuse the tagged protocol's files as they refuse the single-table one's
    for name in ("plonk", "fflonk", "fflonk_lookup"):
        mod = importlib.import_module("eigen_zkvm_amd." + name)
        with pytest.raises(pl.ZkError, match=r'not a verification key of this prover \(protocol "plonk-shplonk-lookup-tagged"\)'):
            mod.vk_from_json(tjs)
        with pytest.raises(pl.ZkError, match='not a proof of this prover on BN128 \\(protocol "plonk-shplonk-lookup-tagged"'):
            mod.proof_from_json(tp, cv)


def test_fflonk_with_lookups_refuses_a_tagged_circuit_before_any_device_work(pl):
    import types
    fl = importlib.import_module("eigen_zkvm_amd.fflonk_lookup")
    n_vars, public, gates, tables, wit = _parts(ref.R["BN128"])
    c = pl.LookupCircuit(n_vars, public, gates, tables=tables)
    with pytest.raises(pl.ZkError, match="fflonk lookup: the circuit has 2 tagged tables: fflonk with lookups proves one table"):
        fl.setup(types.SimpleNamespace(curve="BN128", max_coeffs=1 << 20), c)
