"""A plain-Python trace checker: the reference the device's pil_verify report is compared with, field by field and exactly.

Written from the semantics of the check alone (include/zkgpu.h "pil_verify"): the PIL as written (`expressions`, `polIdentities`,
`plookupIdentities`, `permutationIdentities`, `connectionIdentities`, `publics`) on the rows of the trace; N = the common `polDeg`; `next`
reads row (i + 1) mod N; every value is a base-field word.  Columns are numpy object arrays of Python ints (exact arithmetic, and quick
enough for 2^19 rows); tuples are compared as tuples, multisets with collections.Counter.  Nothing here comes from the product."""
import collections

import numpy as np

P = 0xFFFFFFFF00000001
K = 12275445934081160404                                                      # helper.rs:16-23: k_0 = 1, k_j = K^j


def gl_root(nbits):                                                           # MG[nbits]
    w = pow(7, 0xFFFFFFFF, P)
    for _ in range(32 - nbits):
        w = w * w % P
    return w


class Rows:
    def __init__(self, pil, const, cm):
        refs = pil["references"]
        degs = {r["polDeg"] for r in refs.values()}
        assert len(degs) == 1
        (self.n,) = degs
        self.pil = pil
        n_const, n_cm = pil["nConstants"], pil["nCommitments"]
        const = np.asarray(const, dtype=np.uint64).reshape(-1)
        cm = np.asarray(cm, dtype=np.uint64).reshape(-1)
        assert const.size == self.n * n_const and cm.size == self.n * n_cm
        self.const = [const[j::n_const].astype(object) for j in range(n_const)]
        self.cm = [cm[j::n_cm].astype(object) for j in range(n_cm)]
        self._exp = {}
        self._publics = None

    def publics(self):
        if self._publics is None:
            self._publics = []
            for p in self.pil["publics"]:                                      # a cell of a committed column, or of an expression (imP)
                col = self.cm[p["polId"]] if p["polType"] == "cmP" else self.exp(p["polId"])
                self._publics.append(int(col[p["idx"]]))
        return self._publics

    def exp(self, k):
        if k not in self._exp:
            self._exp[k] = self.ev(self.pil["expressions"][k])
        return self._exp[k]

    def ev(self, e):
        op = e["op"]
        if op in ("cm", "const", "exp"):
            v = self.cm[e["id"]] if op == "cm" else self.const[e["id"]] if op == "const" else self.exp(e["id"])
            return np.roll(v, -1) if e.get("next") else v
        if op == "number":
            return np.full(self.n, int(e["value"]) % P, dtype=object)
        if op == "public":
            return np.full(self.n, self.publics()[e["id"]], dtype=object)
        if op == "neg":
            return (-self.ev(e["values"][0])) % P
        a, b = self.ev(e["values"][0]), self.ev(e["values"][1])
        if op == "add":
            return (a + b) % P
        if op == "sub":
            return (a - b) % P
        if op == "mul":
            return (a * b) % P
        raise ValueError("expression op " + op)


def _src(kind, index, d):
    return {"kind": kind, "index": index, "fileName": d.get("fileName", ""), "line": d.get("line", 0)}


def _set_sides(R, d, kind, index, findings):
    """-> (f tuples, t tuples, selected f rows, selected t rows); selector findings go to `findings`"""
    n = R.n
    f = list(zip(*[R.exp(k).tolist() for k in d["f"]]))
    t = list(zip(*[R.exp(k).tolist() for k in d["t"]]))
    sel = []
    for side, key in (("f", "selF"), ("t", "selT")):
        if d.get(key) is None:
            sel.append(range(n))
            continue
        s = R.exp(d[key]).tolist()
        bad = [i for i in range(n) if s[i] > 1]
        if bad:
            findings.append(dict(_src("selector", index, d), identity=kind, side=side, n_rows=str(len(bad)), first_row=str(bad[0]), value=str(s[bad[0]])))
        sel.append([i for i in range(n) if s[i] != 0])
    return f, t, sel[0], sel[1]


def check(pil, const, cm):
    """-> the report, in the shape of zk_pil_check_run's"""
    R = Rows(pil, const, cm)
    n = R.n
    findings = []
    for k, d in enumerate(pil["polIdentities"]):
        v = R.exp(d["e"]).tolist()
        bad = [i for i in range(n) if v[i] != 0]
        if bad:
            findings.append(dict(_src("identity", k, d), n_rows=str(len(bad)), first_row=str(bad[0]), value=str(v[bad[0]])))
    for k, d in enumerate(pil.get("plookupIdentities") or []):
        f, t, sf, st = _set_sides(R, d, "plookup", k, findings)
        table = {t[i] for i in st}
        bad = [i for i in sf if f[i] not in table]
        if bad:
            findings.append(dict(_src("plookup", k, d), n_rows=str(len(bad)), first_row=str(bad[0]), values=[str(x) for x in f[bad[0]]]))
    for k, d in enumerate(pil.get("permutationIdentities") or []):
        f, t, sf, st = _set_sides(R, d, "permutation", k, findings)
        c = collections.Counter(t[i] for i in st)
        c.subtract(collections.Counter(f[i] for i in sf))
        n_f, n_t = sum(-x for x in c.values() if x < 0), sum(x for x in c.values() if x > 0)
        if n_f or n_t:
            ff = next((i for i in sf if c[f[i]] < 0), None)
            ft = next((i for i in st if c[t[i]] > 0), None)
            findings.append(dict(_src("permutation", k, d), n_f_unmatched=str(n_f), n_t_unmatched=str(n_t),
                                 first_f_row=None if ff is None else str(ff), first_t_row=None if ft is None else str(ft),
                                 f_values=None if ff is None else [str(x) for x in f[ff]], t_values=None if ft is None else [str(x) for x in t[ft]]))
    for k, d in enumerate(pil.get("connectionIdentities") or []):
        pols = [R.exp(e).tolist() for e in d["pols"]]
        S = [R.exp(e).tolist() for e in d["connections"]]
        where = identity_cells(n, len(pols))
        unnamed, differ = [], []
        for j in range(len(pols)):
            for i in range(n):
                p = where.get(S[j][i])
                if p is None:
                    unnamed.append((j, i))
                elif pols[j][i] != pols[p[0]][p[1]]:
                    differ.append((j, i, p[0], p[1]))
        if unnamed:
            j, i = unnamed[0]
            findings.append(dict(_src("connection_value", k, d), n_cells=str(len(unnamed)), col=j, row=str(i), value=str(S[j][i])))
        if differ:
            j, i, jj, ii = differ[0]
            findings.append(dict(_src("connection", k, d), n_cells=str(len(differ)), col=j, row=str(i), partner_col=jj, partner_row=str(ii),
                                 value=str(pols[j][i]), partner_value=str(pols[jj][ii])))
    return {"n": n, "publics": [str(p) for p in R.publics()],
            "checked": {"polIdentities": len(pil["polIdentities"]), "plookupIdentities": len(pil.get("plookupIdentities") or []),
                        "permutationIdentities": len(pil.get("permutationIdentities") or []),
                        "connectionIdentities": len(pil.get("connectionIdentities") or [])},
            "findings": findings}


def identity_cells(n, n_pols):
    """{k_j w^i: (j, i)}"""
    w = gl_root(n.bit_length() - 1)
    where, kj = {}, 1
    for j in range(n_pols):
        x = kj
        for i in range(n):
            where[x] = (j, i)
            x = x * w % P
        kj = kj * K % P
    return where
