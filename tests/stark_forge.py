"""Forged STARK proofs, one for every check the verifier makes (csrc/stark_verify.hip, and its restatement in oracle/stark_prover.py),
each built so that exactly ONE check can reject it.  "Rejected" alone does not say which check did the work -- bump a word of an honest
proof and a Merkle path, a fold and half the transcript break together, so a check could be deleted while another masks it.  Here:

  A  transcript-consistent forgeries.  The oracle's prover with its `cheat` hooks: what it changes it also commits to and absorbs, so every
     root, challenge and query index is the one a verifier derives, every Merkle path opens, and only the named check sees the lie:
       degree      an evaluation of a committed polynomial is off by one, the evaluation of the quotient piece qs[0] is corrected so that
                   Q Z = C still holds at xi.  The FRI polynomial is then a quotient with a remainder, not of low degree; it is folded honestly.
       fold<k>     limb 0 of every value of the k-th folded polynomial + 1 before it is merkelized: step k's tree opens, later folds start from it
       last_fold   the same on the last folded polynomial (a constant shift keeps its degree low)
  B  tampers of an honest proof that leave every opened value and everything the transcript absorbs alone: siblings, path depth.  Plus
     those where the ORDER of the checks says which one answers: a step value outside the triple fold 1 compares (the step tree's Merkle
     check, then fold 2), an evaluation (Eq. 30, first of all), and structure cases.
  C  the same sibling tampers on 16-ary scalar-field trees, where the reference binds only the last level of a path
     (merklehash_bn128.rs:108-128) and the library is strict by default.

catalogue() -> {name: (zkin, check, phrase)}: `check` is the oracle's name for the one check that stops it (stark_prover.checks()), "strict" for
what only the library's strict level check stops (the restated verifier ACCEPTS those, as the reference would), None where no single
check of the restated verifier isolates it (an evaluation also moves the transcript; the step value; structure); `phrase` is what
last_reject() must contain.  No test."""
import copy
import json
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import interp              # noqa: E402
import stark_prover as SP  # noqa: E402
import starkinfo as SI     # noqa: E402

D = ROOT / "tests" / "golden" / "starky_data"
P = SP.P
STRUCT = {"nBits": 10, "nBitsExt": 11, "nQueries": 8, "verificationHashType": "GL", "steps": [{"nBits": 11}, {"nBits": 7}, {"nBits": 3}]}
ONE_STEP = dict(STRUCT, steps=[{"nBits": 11}])        # the query code's value is compared with finalPol directly; max_deg = 1024 of 2048
FIXTURES = {"fib_gl": ("fib.pil.json.gl", "fib.const.gl", "fib.cm.gl"), "plookup_gl": ("plookup.pil.json.gl", "plookup.const.gl", "plookup.cm.gl"),
            "fibonacci": ("fib.pil.json", "fib.const", "fib.cm")}
PROVER_ADDR = "273030697313060285579891744179749754319274977764"
S0 = ("1", "2", "3", "4", "C")
TREE_NAME = {"1": "tree1", "2": "tree2", "3": "tree3", "4": "tree4", "C": "the constants' tree"}   # stark_verify.hip, `what`
STEP_NAME = "a FRI step"
OFF_TRIPLE = "s1_vals word outside the triple fold 1 reads"


class Setup:
    """one fixture under one StarkStruct: the oracle's setup, and the backend its hash type needs"""

    def __init__(self, orc, fixture, ss):
        pil_f, const_f, cm_f = FIXTURES[fixture]
        self.fixture, self.ss, self.orc, self.cm_path, self.const_path = fixture, ss, orc, D / cm_f, D / const_f
        self.gl = ss["verificationHashType"] == "GL"
        self.b = orc if self.gl else SP.BN128Backend(orc, ss["verificationHashType"].lower())
        self.su = SP.setup(json.load(open(D / pil_f)), D / const_f, ss, self.b)
        self.info, self.prog = self.su["starkinfo"], self.su["program"]
        self.steps = [s["nBits"] for s in ss["steps"]]

    def program_json(self):
        return json.dumps(SI.to_json(self.info, self.prog))

    def const_root(self):
        return [int(v) for v in self.su["const_tree"][-4:]]

    def prove(self, cheat=None):
        proof = SP.stark_gen(self.cm_path, self.su, self.ss, self.b, cheat=cheat)
        return SP.to_zkin(proof) if self.gl else SP.to_zkin_bn128(proof, self.b, PROVER_ADDR)

    def verify(self, z, skip=()):
        """the restated verifier's verdict on zkin text (stark_verify.rs answers Ok(false) or bails with FRIVerifierFailed)"""
        proof = SP.from_zkin(z) if self.gl else SP.from_zkin_bn128(z, self.b)
        try:
            return bool(SP.stark_verify(proof, self.const_root(), self.info, self.prog, self.ss, self.b, skip=skip))
        except ValueError as e:
            assert "FRIVerifierFailed" in str(e)
            return False

    def checks(self):
        return SP.checks(self.ss)

    def query_indices(self, z):
        """the query indices a verifier derives for this proof (stark_verify.rs:28-61, fri.rs:196-212): the transcript replayed"""
        proof = SP.from_zkin(z) if self.gl else SP.from_zkin_bn128(z, self.b)
        tr = self.b.transcript()
        for p in proof["publics"]:
            tr.put([p])
        for k, n in (("root1", 2), ("root2", 2), ("root3", 1), ("root4", 1)):
            tr.put(proof[k])
            for _ in range(n):
                tr.get_field()
        for e in proof["evals"]:
            tr.put(e)
        tr.get_field(); tr.get_field()
        fp = proof["fri_proof"]
        for si in range(len(self.steps)):
            tr.get_field()
            if si < len(self.steps) - 1:
                tr.put(fp["queries"][si + 1]["root"])
            else:
                for e in fp["last"]:
                    tr.put(e)
        return [int(v) for v in tr.get_permutations(self.ss["nQueries"], self.steps[0])]


# ---- A: the dishonest prover's hooks -----------------------------------------------------------------------------------------------
def degree_cheat(S):
    info, prog, orc = S.info, S.prog, S.orc
    nbits = S.ss["nBits"]
    quotient = {info["ev_idx"]["cm"][(0, q)] for q in info["qs"]}
    k = next(i for i, ev in enumerate(info["ev_map"]) if ev["type_"] == "cm" and i not in quotient)
    kq = info["ev_idx"]["cm"][(0, info["qs"][0])]

    def evals_hook(evals, challenge, publics):
        evals[k][0] = (evals[k][0] + 1) % P
        xi = SP.f3(challenge[7])
        x_n = SP.f3_pow(xi, 1 << nbits)
        ctx = {"evals": evals, "publics": publics, "challenge": challenge, "Z": interp.v_sub(x_n, (1,)),
               "Zp": interp.v_sub(SP.f3_pow(interp.v_mul(xi, (orc.root(nbits),)), 1 << nbits), (1,))}
        res = SP.execute_code(prog["verifier_code"]["first"], ctx)                # C(xi) from the forged evaluations
        x_acc, q = (1,), (0,)
        for i in range(info["q_deg"]):
            q = interp.v_add(q, interp.v_mul(x_acc, SP.f3(evals[info["ev_idx"]["cm"][(0, info["qs"][i])]])))
            x_acc = interp.v_mul(x_acc, x_n)
        delta = interp.v_sub(interp.v_mul(res, SP.f3_inv(orc, ctx["Z"])), q)     # res' / Z(xi) - q: piece 0 enters q with weight 1
        evals[kq] = list(interp.v_add(SP.f3(evals[kq]), delta))
        return evals
    return {"evals": evals_hook}


def shift_cheat(si_target):
    def folded(si, pol):
        if si == si_target:
            v = pol.reshape(-1, 3)
            v[:, 0] = np.where(v[:, 0] == np.uint64(P - 1), np.uint64(0), v[:, 0] + np.uint64(1))
        return pol
    return {"folded": folded}


def forgeries(S):
    n = len(S.steps)
    out = {"degree": (S.prove(degree_cheat(S)), "degree", "degree is too high")}
    for k in range(1, n):
        out["fold%d" % k] = (S.prove(shift_cheat(k - 1)), "fold%d" % k, "a fold does not match the next step's opening (step %d)" % k)
    out["last_fold"] = (S.prove(shift_cheat(n - 1)), "last_fold", "the last fold does not match the last polynomial")
    return out


# ---- B / C: tampers of an honest proof ---------------------------------------------------------------------------------------------
def bump(s):
    """a decimal Goldilocks word + 1"""
    return str((int(s) + 1) % P)


def _bump_digit(s):
    """a decimal scalar-field element that stays canonical and differs (digests are ~2^254: the last digit moves, never carries out)"""
    return s[:-1] + str((int(s[-1]) + 1) % 10)


def _edit(z, f):
    bad = copy.deepcopy(z)
    f(bad)
    assert bad != z
    return bad


def _trees(S):
    """(siblings key, bits of the tree's height, name in last_reject()) of every tree a proof opens"""
    return [("s0_siblings" + nm, S.steps[0], TREE_NAME[nm]) for nm in S0] + \
           [("s%d_siblings" % k, S.steps[k], STEP_NAME) for k in range(1, len(S.steps))]


def sibling_tampers(S, z):
    """one word of one sibling, at the first and the last query, at the lowest and the top level of every tree's path.  GL: word 0 at level 0,
    word 3 at the top.  Scalar fields: node 5 of the level's 16.  At the top level the root moves (`does not open to its root`).  Below it the
    strict walk answers: at level 0 if node 5 is where the leaf's digest stands (idx & 15), else at level 1, whose node no longer is the
    hash of the level below."""
    out, nq = {}, S.ss["nQueries"]
    ys = None if S.gl else S.query_indices(z)
    for sk, bits, what in _trees(S):
        depth = len(z[sk][0])
        for q in (0, nq - 1):
            for lvl in sorted({0, depth - 1}):
                name = "%s[%d] level %d" % (sk, q, lvl)
                if S.gl:
                    w = 3 if lvl == depth - 1 else 0
                    bad = _edit(z, lambda b: b[sk][q][lvl].__setitem__(w, bump(b[sk][q][lvl][w])))
                    out[name] = (bad, "merkle", what + " does not open to its root")
                    continue
                bad = _edit(z, lambda b: b[sk][q][lvl].__setitem__(5, _bump_digit(b[sk][q][lvl][5])))
                if lvl == depth - 1:
                    out[name] = (bad, "merkle", what + " does not open to its root")
                else:
                    seen_at = 0 if (ys[q] % (1 << bits)) & 15 == 5 else 1
                    out[name] = (bad, "strict", "%s: level %d of the path does not hold the value carried up" % (what, seen_at))
    return out


def step_value_off_the_triple(S, z):
    """a word of s1_vals outside the triple 3 gi .. 3 gi + 2 that fold 1 compares.  The step tree's Merkle check is the first to see it, and
    the only one before fold 2, which transforms the whole row: so two checks see it and no single skip isolates it (check None).  Under
    scalar-field trees the reference never looks at a row's digest once the path has a level; there the strict walk is what answers first."""
    if len(S.steps) < 2:
        return {}
    q = S.ss["nQueries"] - 1
    gi = (S.query_indices(z)[q] % (1 << S.steps[0])) >> S.steps[1]
    w = 3 * ((gi + 1) % (len(z["s1_vals"][q]) // 3)) + 1
    assert not 3 * gi <= w < 3 * gi + 3
    bad = _edit(z, lambda b: b["s1_vals"][q].__setitem__(w, bump(b["s1_vals"][q][w])))
    return {OFF_TRIPLE: (bad, None, STEP_NAME + (" does not open to its root" if S.gl else ": level 0 of the path does not hold the value carried up"))}


def depth_tampers(S, z):
    """a copy of the top level appended to a path: the restated verifier has no depth check, its Merkle check sees a different root"""
    out = {"depth s0_siblings3[0]": (_edit(z, lambda b: b["s0_siblings3"][0].append(list(b["s0_siblings3"][0][-1]))), "merkle", "tree3: the Merkle path has")}
    if len(S.steps) > 1:
        q = S.ss["nQueries"] - 1
        out["depth s1_siblings[%d]" % q] = (_edit(z, lambda b: b["s1_siblings"][q].append(list(b["s1_siblings"][q][-1]))), "merkle",
                                            STEP_NAME + ": the Merkle path has")
    return out


def eval_tampers(S, z):
    """Eq. 30 comes before anything derived from the evaluations, so it is the check that answers -- but a bumped evaluation also moves the
    challenges after it, so no skip isolates it (check None)"""
    return {"evals[%d][0]" % k: (_edit(z, lambda b: b["evals"][k].__setitem__(0, bump(b["evals"][k][0]))), None, "Q != C * P at xi")
            for k in range(len(z["evals"]))}


def structure_tampers(S, z):
    n = len(S.steps)
    out = {"finalPol short by one": (_edit(z, lambda b: b["finalPol"].pop()), None, "the last polynomial does not hold 2^steps.last values"),
           "one query's opening missing": (_edit(z, lambda b: (b["s0_vals1"].pop(), b["s0_siblings1"].pop())), None, "s0_vals1: one opening per query expected"),
           "one step too many": (_edit(z, lambda b: b.update({"s%d_root" % n: b["root4"], "s%d_vals" % n: b["s0_vals4"], "s%d_siblings" % n: b["s0_siblings4"]})),
                                 None, "the proof has more FRI steps than the starkStruct")}
    if n > 1:
        last = n - 1
        out["one step too few"] = (_edit(z, lambda b: [b.pop("s%d_%s" % (last, k)) for k in ("root", "vals", "siblings")]), None,
                                   "the proof has fewer FRI steps than the starkStruct")
        # one row of a step tree shorter than the others: the rows of a tree are hashed together, so their widths are compared first;
        # `wrong group size` / `not a list of extension values` need every row of the tree forged AND its Merkle paths to open
        out["a step row short by one triple"] = (_edit(z, lambda b: b["s1_vals"][0].__delitem__(slice(-3, None))), None, STEP_NAME + ": rows of one tree differ in width")
        out["a step row not divisible by 3"] = (_edit(z, lambda b: b["s1_vals"][0].pop()), None, STEP_NAME + ": rows of one tree differ in width")
    return out


def tampers(S, z):
    out = {}
    out.update(sibling_tampers(S, z))
    out.update(step_value_off_the_triple(S, z))
    if S.gl:
        out.update(depth_tampers(S, z))
        out.update(eval_tampers(S, z))
        out.update(structure_tampers(S, z))
    return out


_CACHE = {}


def catalogue(orc, fixture, ss):
    """-> (Setup, honest zkin, {name: (zkin, check, phrase)}), built once per (fixture, struct) and shared: nobody changes an entry"""
    key = (fixture, json.dumps(ss, sort_keys=True))
    if key not in _CACHE:
        S = Setup(orc, fixture, ss)
        z = S.prove()
        cat = forgeries(S)
        cat.update(tampers(S, z))
        _CACHE[key] = (S, z, cat)
    return _CACHE[key]


def sweep(z, n_queries):
    """every numeric leaf of a GL zkin that belongs to query 0 or to the last query, and every word of the roots, evaluations, publics and the
    last polynomial, bumped one at a time: yields (where, zkin text).  One parsed copy is edited and restored, so a thousand cases cost a
    thousand json.dumps and nothing else.  rootC is not part of the proof a verifier reads (the constants' root comes from the setup)."""
    b = copy.deepcopy(z)

    def leaves(node, path):
        if isinstance(node, list):
            for i in range(len(node)):
                if isinstance(node[i], str):
                    yield node, i, path + (i,)
                else:
                    yield from leaves(node[i], path + (i,))
    for key in b:
        if key == "rootC" or not isinstance(b[key], list):
            continue
        per_query = key.endswith(("_vals", "_siblings")) or key.startswith(("s0_vals", "s0_siblings"))     # one member per query
        tops = [(b[key][q], (key, q)) for q in sorted({0, n_queries - 1})] if per_query else [(b[key], (key,))]
        for node, path in tops:
            for holder, i, where in leaves(node, path):
                old = holder[i]
                holder[i] = bump(old)
                yield where, json.dumps(b)
                holder[i] = old
    assert b == z
