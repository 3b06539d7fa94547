"""Every forged proof of tests/stark_forge.py isolates its check, shown on the restated verifier (oracle/stark_prover.py) before a GPU is touched:
rejected as it stands, accepted when exactly its own check is not made, rejected again when any other single check is not made instead.
That is what lets tests/test_gpu_verify_forged.py read a rejection by the library as the work of one named check."""
import pytest

import stark_forge as F

GL = [("fib_gl", "three steps"), ("fib_gl", "one step"), ("plookup_gl", "three steps"), ("plookup_gl", "one step")]
FR = [("fibonacci", "BN128"), ("fibonacci", "BLS12381")]
STRUCTS = {"three steps": F.STRUCT, "one step": F.ONE_STEP, "BN128": dict(F.STRUCT, verificationHashType="BN128"),
           "BLS12381": dict(F.STRUCT, verificationHashType="BLS12381")}


def _isolated(S, name, z, check):
    assert S.verify(z) is False, name
    assert S.verify(z, skip=(check,)) is True, "%s: not accepted without its own check %s" % (name, check)
    for c in S.checks():
        if c != check:
            assert S.verify(z, skip=(c,)) is False, "%s: accepted without %s, so %s is not what stops it" % (name, c, check)


@pytest.mark.parametrize("fixture,struct", GL + FR)
def test_every_forgery_is_stopped_by_its_own_check_and_no_other(orc, fixture, struct):
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    n = len(S.steps)
    assert S.checks() == ("eq30", "merkle") + tuple("fold%d" % k for k in range(1, n)) + ("last_fold", "degree")
    named = {name: e for name, e in cat.items() if e[1] in S.checks()}
    # A in full, and of B / C every tamper the restated verifier has a named check for: all siblings, both depths
    assert {"degree", "last_fold"} | {"fold%d" % k for k in range(1, n)} <= set(named)
    n_trees = 5 + n - 1
    if S.gl:
        assert sum(1 for e in named.values() if e[1] == "merkle") == 4 * n_trees + (2 if n > 1 else 1)
    else:
        assert sum(1 for e in named.values() if e[1] == "merkle") == 2 * n_trees      # 16-ary: the top level (the depth-1 tree's only level)
    for name, (z, check, phrase) in named.items():
        _isolated(S, name, z, check)


@pytest.mark.parametrize("fixture,struct", GL + FR)
def test_honest_proof_is_accepted_with_every_skip_and_with_none(orc, fixture, struct):
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    assert S.verify(honest) is True
    for c in S.checks():
        assert S.verify(honest, skip=(c,)) is True, c
    assert S.verify(honest, skip=S.checks()) is True


@pytest.mark.parametrize("fixture,struct", GL)
def test_a_bumped_evaluation_is_rejected_whatever_single_check_is_skipped(orc, fixture, struct):
    """Eq. 30 is the first check to see it, but the evaluations also feed the challenges after them: not isolated, and the catalogue says so"""
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    evs = {name: e for name, e in cat.items() if name.startswith("evals[")}
    assert len(evs) == len(honest["evals"])
    for name, (z, check, phrase) in evs.items():
        assert check is None
        for skip in [()] + [(c,) for c in S.checks()]:
            assert S.verify(z, skip=skip) is False, (name, skip)


@pytest.mark.parametrize("fixture,struct", [c for c in GL + FR if c[1] != "one step"])
def test_a_step_value_outside_the_compared_triple_is_seen_by_the_merkle_check_and_the_next_fold(orc, fixture, struct):
    """fold 2 transforms the whole s1 row, so the word is not unread: rejected under every single skip, accepted only without both.  (16-ary
    trees: the reference's path check never reaches the row, merklehash_bn128.rs:108-128, so fold 2 alone stands there.)"""
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    z, check, phrase = cat[F.OFF_TRIPLE]
    assert check is None
    for skip in [()] + [(c,) for c in S.checks() if c != "fold2"]:
        assert S.verify(z, skip=skip) is False, skip
    assert S.verify(z, skip=("fold2",)) is not S.gl
    assert S.verify(z, skip=("merkle", "fold2")) is True


@pytest.mark.parametrize("fixture,struct", FR)
def test_the_reference_leniency_below_the_top_level_is_what_strict_entries_rest_on(orc, fixture, struct):
    """merklehash_bn128.rs:108-128 binds only the last level of a 16-ary path: the restated verifier accepts these, the library must not"""
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    strict = {name: e for name, e in cat.items() if e[1] == "strict"}
    assert len(strict) == 2 * 6                         # five trees of depth 3 and s1 of depth 2, at two queries; s2 has one level
    for name, (z, check, phrase) in strict.items():
        assert S.verify(z) is True, name


def test_degree_forgery_of_the_one_step_struct_fills_the_forbidden_coefficients(orc):
    """nBits 10, nBitsExt 11, one step of 11 bits: max_deg = 1024, coefficients 1025 .. 2047 of the last polynomial must be zero"""
    import numpy as np
    S, honest, cat = F.catalogue(orc, "fib_gl", F.ONE_STEP)
    for z, zero in ((honest, True), (cat["degree"][0], False), (cat["last_fold"][0], True)):
        last = np.array([int(v) for e in z["finalPol"] for v in e], np.uint64)
        assert last.size == 3 * 2048
        coef = orc.f3_ntt(last, 11, inverse=True).reshape(-1, 3)
        assert (not coef[1025:].any()) is zero


def test_forgeries_keep_what_they_must_not_touch(orc):
    """a fold<k> forgery differs from the honest proof from step k's tree on, never before; `degree` differs in two evaluations only there"""
    S, honest, cat = F.catalogue(orc, "fib_gl", F.STRUCT)
    early = ["root1", "root2", "root3", "root4", "evals", "publics"]
    for name in ("fold1", "fold2", "last_fold"):
        z = cat[name][0]
        assert all(z[k] == honest[k] for k in early), name
    assert cat["fold2"][0]["s1_root"] == honest["s1_root"] and cat["fold2"][0]["s2_root"] != honest["s2_root"]
    assert cat["fold1"][0]["s1_root"] != honest["s1_root"]
    assert cat["last_fold"][0]["s2_root"] == honest["s2_root"] and cat["last_fold"][0]["finalPol"] != honest["finalPol"]
    z = cat["degree"][0]
    assert all(z[k] == honest[k] for k in early if k != "evals")
    assert sum(1 for a, b in zip(z["evals"], honest["evals"]) if a != b) == 2
