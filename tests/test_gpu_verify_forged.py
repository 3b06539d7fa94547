"""zk_stark_verify / zk_stark_verify_with (csrc/stark_verify.hip) against the catalogue of tests/stark_forge.py: a forged proof for every check
the verifier makes, each rejected BY NAME -- the verdict is False and last_reject() names the one check that can see the forgery
(tests/test_stark_forge.py shows on the restated verifier that no other check does).  A check that is deleted, or made for the first step or
the first tree only, now fails a test instead of hiding behind the next check in line.  Plus one sweep: every word of two queries, of every root,
evaluation, public and last-polynomial value of a proof bumped, one at a time -- none accepted, none an error."""
import copy
import importlib
import json
import time

import numpy as np
import pytest

import stark_forge as F

pytestmark = pytest.mark.gpu
STRUCTS = {"three steps": F.STRUCT, "one step": F.ONE_STEP, "BN128": dict(F.STRUCT, verificationHashType="BN128"),
           "BLS12381": dict(F.STRUCT, verificationHashType="BLS12381")}
CASES = [("fib_gl", "three steps"), ("fib_gl", "one step"), ("plookup_gl", "three steps"), ("plookup_gl", "one step"),
         ("fibonacci", "BN128"), ("fibonacci", "BLS12381")]


def _device(zk, S):
    """the library's setup for the oracle's: the same program text, the constants from the same file"""
    zk.init(0)
    stark = importlib.import_module("eigen_zkvm_amd.stark")
    kw = {} if S.gl else {"prover_addr": F.PROVER_ADDR}
    ns = stark.NativeStarkSetup(np.fromfile(S.const_path, dtype="<u8"), S.program_json(), json.dumps(S.ss), **kw)
    assert ns.const_root() == S.const_root()
    return stark, ns


def _entry_points(stark, ns, S):
    program, ss, root = S.program_json(), json.dumps(S.ss), S.const_root()
    return {"ns.verify": ns.verify, "stark.stark_verify": lambda z: stark.stark_verify(z, root, program, ss)}   # the second needs no prover setup


def _oracle_accepts(S, z):
    try:
        return S.verify(z)
    except IndexError:                    # a missing opening: the reference indexes them blindly and panics (fri.rs:214-226)
        return False


@pytest.mark.parametrize("fixture,struct", CASES)
def test_the_device_and_the_oracle_write_the_same_honest_proof(zk, orc, fixture, struct):
    """the forgeries are the oracle prover's: they stand on the proof the device writes for the same setup, byte for byte"""
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    stark, ns = _device(zk, S)
    got = ns.gen(np.fromfile(S.cm_path, dtype="<u8"))
    assert list(got) == list(honest) and got == honest
    assert json.dumps(got) == json.dumps(honest)
    ns.free()


@pytest.mark.parametrize("fixture,struct", CASES)
def test_every_forged_proof_is_rejected_by_the_check_it_targets(zk, orc, fixture, struct):
    S, honest, cat = F.catalogue(orc, fixture, STRUCTS[struct])
    stark, ns = _device(zk, S)
    entries = _entry_points(stark, ns, S)
    for verify in entries.values():
        assert verify(honest) is True
    wrong = []
    for name, (z, check, phrase) in cat.items():
        for ep, verify in entries.items():
            verdict = verify(z)                                            # (a ZkError here fails the test: every entry is a well-formed proof)
            why = ns.last_reject()
            if verdict is not False or phrase not in why or not why.startswith("stark_verify: "):
                wrong.append((name, ep, verdict, why, "expected: " + phrase))
        # the restated verifier agrees -- except where the reference is lenient and the library strict by design (16-ary paths below the top level)
        want = check == "strict"
        if _oracle_accepts(S, z) is not want:
            wrong.append((name, "oracle", not want))
        if check == "strict":
            with stark.reference_compat_paths():
                if ns.verify(z) is not True:
                    wrong.append((name, "reference-compatible paths", False, ns.last_reject()))
    assert wrong == []
    for verify in entries.values():
        assert verify(honest) is True                                      # (nothing is left in a bad state)
    ns.free()


def test_words_are_reduced_and_words_past_64_bits_are_errors(zk, orc):
    """parse_word: FGL::from(u64) reduces, so v + p (below 2^64) reads as v wherever a word stands; 2^64 is no u64 and is malformed input.
    v + p < 2^64 needs v < 2^32 - 1: the fixtures' opened values are uniform field elements and none is that small, so the accepted case is
    shown on the publics (1 and 2 in the fibonacci fixture) and on a path's zero words (tree1's rows are two words wide, so a leaf is its row
    padded with zeros and stands in its neighbour's path as it is): the same parser, into the transcript, the verifier program and the hashes."""
    S, honest, cat = F.catalogue(orc, "fibonacci", F.STRUCT)
    stark, ns = _device(zk, S)
    assert honest["publics"][:2] == ["1", "2"] and honest["s0_siblings1"][0][0][2:] == ["0", "0"]
    for ep, verify in _entry_points(stark, ns, S).items():
        z = copy.deepcopy(honest)
        z["publics"][0] = str(1 + F.P); z["publics"][1] = str(2 + F.P)
        z["s0_siblings1"][0][0][2] = str(F.P)
        assert verify(z) is True, ep
        z["publics"][0] = str(2 + F.P)                                     # (and it is the VALUE that is read: 2 is not 1)
        assert verify(z) is False and "Q != C * P at xi" in ns.last_reject(), ep
        for where in (lambda b: b["s0_vals1"][0], lambda b: b["s0_siblings4"][7][10], lambda b: b["s1_vals"][3], lambda b: b["finalPol"][2],
                      lambda b: b["evals"][0], lambda b: b["publics"], lambda b: b["root2"]):
            z = copy.deepcopy(honest)
            where(z)[0] = str(1 << 64)
            with pytest.raises(zk.ZkError, match="out of range"):
                verify(z)
            z = copy.deepcopy(honest)
            where(z)[0] = str((1 << 64) - 1)                               # the largest u64 is a word (2^32 - 2 after reduction), and not the honest one
            assert verify(z) is False, ep
        assert verify(honest) is True
    ns.free()


def test_sweep_every_word_of_two_queries_and_of_what_the_transcript_absorbs(zk, orc):
    """fib_gl, 2^10 rows: 2 queries x (6 opened step-0 words + 5 paths of 11 x 4 + two step rows of 48 + paths of 7 x 4 and 3 x 4) = 724,
    + 6 roots x 4 + 6 evaluations x 3 + 1 public + 8 x 3 words of the last polynomial = 791 proofs, each with one word + 1"""
    S, honest, cat = F.catalogue(orc, "fib_gl", F.STRUCT)
    stark, ns = _device(zk, S)
    assert ns.verify(honest) is True
    accepted, n, t0 = [], 0, time.perf_counter()
    for where, text in F.sweep(honest, S.ss["nQueries"]):
        n += 1
        if ns.verify(text) is not False:                                   # (a ZkError fails the test as it stands: none may raise)
            accepted.append(where)
    dt = time.perf_counter() - t0
    print("sweep: %d tampered proofs in %.2f s" % (n, dt))
    assert n == 791
    assert accepted == []
    assert ns.verify(honest) is True
    ns.free()
