"""KZG commitments over a powers-of-tau file, on the device: commit to a polynomial, open it at a point, check openings.

    python tools/zkgpu_kzg.py kzg_commit [-c CURVE] --ptau F --poly p.bin [--evals] -o commitment.json [--no-check-srs]
    python tools/zkgpu_kzg.py kzg_open   [-c CURVE] --ptau F --poly p.bin [--poly p2.bin ...] --at Z -o opening.json [--no-check-srs]
    python tools/zkgpu_kzg.py kzg_open   [-c CURVE] --ptau F --poly p.bin --at Z1,Z2,.. [--poly p2.bin --at Z3,.. ...] -o multi_opening.json
    python tools/zkgpu_kzg.py kzg_verify [-c CURVE] --ptau F opening.json [opening.json ...] [--no-check-srs]

p.bin is n x 32 bytes: the coefficients of p, lowest degree first, canonical little-endian; a value that is not below r is refused by its
index.  With --evals the file holds the values of p on the 2^k-point domain of the library's transforms instead.  Z is decimal or 0x hex.
Every subcommand opens the .ptau and runs the file's own check first, as `zkgpu_prove.py groth16_setup --ptau` does; --no-check-srs skips it.
Commitments are in G1 and are NOT hiding.  Points in the JSON files are {"x", "y"} decimal strings, as proof.json writes its G1 points;
the point at infinity is (0, 1).

kzg_open with several --poly opens them all at Z with ONE witness, for f = sum_i gamma^i p_i, and records every commitment and value:
    gamma = SHA-256( curve name in ASCII ("BN128" | "BLS12381")
                     || every commitment in the file's encoding -- x || y, each coordinate little-endian Montgomery, 32 (BN128) or 48
                        (BLS12381) bytes; all zero for infinity -- in the order of the --poly arguments
                     || Z as 32 little-endian bytes ),   the digest read as a big-endian integer, reduced mod r.
kzg_verify recomputes gamma from the opening's own commitments, folds them and the values, and checks all the files' openings in one
randomised pairing equation.  It prints the number of openings and exits 0 when all are accepted; otherwise it prints one line per opening
that is not accepted -- `kzg_verify: FILE: <reason>` -- and exits 1.  CURVE: BN128 | BLS12381; without -c it is read from the .ptau header.

kzg_open with an --at after EVERY --poly (or one --poly and a list Z1,Z2,..) opens polynomial i on its own set of 1 .. 16 distinct points in one
proof of two points, W1 and W2, and writes {"protocol": "kzg-multi", commitments, sets, values, gamma, z, W1, W2}.  gamma and z
are eigen_zkvm_amd.kzg.challenges_of and challenge_z, whose docstrings state the hashed bytes one by one.  kzg_verify takes such files beside the
single-point ones, recomputes gamma and z from the file's own commitments, sets, values and W1, and checks the files of each kind in one batch."""
import argparse, json, pathlib, struct, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CURVES = ("BN128", "BLS12381")
REASONS = {0: "the pairing equation does not hold", -1: "z or y is not below r", -2: "a set is empty, too large, repeats a point or holds z", -3: "a point is not on the curve", -4: "a point is not in the subgroup of order r"}


def curve_of_file(path):
    """the curve a .ptau file's header names by the width of its prime (32 bytes: BN128, 48: BLS12381)"""
    with open(path, "rb") as f:
        head = f.read(28)
    if len(head) < 28 or head[:4] != b"ptau":
        raise SystemExit("zkgpu_kzg: %s is no .ptau file" % path)
    sid, _size, n8 = struct.unpack_from("<IQI", head, 12)
    if sid != 1 or n8 not in (32, 48):
        raise SystemExit("zkgpu_kzg: %s: give the curve with -c" % path)
    return "BN128" if n8 == 32 else "BLS12381"


def _open_handle(a):
    """-> (kzg module, Kzg handle, curve); the file's check first unless --no-check-srs"""
    import importlib
    import eigen_zkvm_amd as zk
    zk.init(0)
    dev, kzg = importlib.import_module("eigen_zkvm_amd.groth16"), importlib.import_module("eigen_zkvm_amd.kzg")
    curve = a.curve or curve_of_file(a.ptau)
    srs = dev.Srs(curve, a.ptau)
    if not a.no_check_srs:                                                # a bad file commits to nothing
        report = srs.check()
        for f in report["findings"]:
            print(dev.srs_check_line(f), file=sys.stderr)
        for k in report["skipped"]:
            print(dev.key_check_skipped_line(k), file=sys.stderr)
        if any(report["counts"].values()):
            raise SystemExit(1)
    h = kzg.Kzg(srs)
    srs.free()
    return kzg, h, curve


def read_poly(kzg, path, curve):
    b = pathlib.Path(path).read_bytes()
    if len(b) % 32:
        raise SystemExit("zkgpu_kzg: %s: %d bytes is no whole number of 32-byte values" % (path, len(b)))
    r = kzg._FR[curve]
    vals = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    for i, v in enumerate(vals):
        if v >= r:
            print("zkgpu_kzg: %s: value %d is not below the scalar field's modulus" % (path, i))
            raise SystemExit(1)
    return vals


def kzg_commit(a):
    kzg, h, curve = _open_handle(a)
    p = read_poly(kzg, a.poly[0], curve)
    c = h.commit_evals(p) if a.evals else h.commit(p)
    out = {"protocol": "kzg", "curve": curve, "n": len(p), "evals": bool(a.evals), "commitment": kzg.point_to_json(c, curve)}
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("kzg_commit: %s, %d %s under %s (power %d) -> %s" % (a.poly[0], len(p), "evaluations" if a.evals else "coefficients", a.ptau, h.power, a.out))
    h.free()
    return 0


def at_groups(a):
    """None for the one-point form (every --poly, then one --at Z); else the sets, one per --poly, as lists of integers"""
    marks = getattr(a, "at_marks", None) or []
    if len(marks) == 1 and "," not in marks[0][1]:
        return None
    if [n for n, _ in marks] != list(range(1, len(a.poly) + 1)):
        raise SystemExit("zkgpu_kzg: kzg_open at several points takes one --at Z1,Z2,.. after every --poly")
    return [[int(v, 0) for v in text.split(",")] for _, text in marks]


def kzg_open_multi(a, sets):
    kzg, h, curve = _open_handle(a)
    r = kzg._FR[curve]
    for i, s in enumerate(sets):
        if not 1 <= len(s) <= kzg.MULTI_MAX_POINTS or len(set(s)) != len(s) or not all(0 <= p < r for p in s):
            print("zkgpu_kzg: --at of polynomial %d: 1 .. %d distinct points below the scalar field's modulus" % (i, kzg.MULTI_MAX_POINTS))
            return 1
    polys = [read_poly(kzg, p, curve) for p in a.poly]
    cs = [h.commit(p) for p in polys]
    values, w1, w2, gamma, z = h.open_multi(polys, sets, commitments=cs)
    out = {"protocol": "kzg-multi", "curve": curve, "commitments": [kzg.point_to_json(c, curve) for c in cs], "sets": [[str(p) for p in s] for s in sets],
           "values": [[str(y) for y in ys] for ys in values], "gamma": str(gamma), "z": str(z), "W1": kzg.point_to_json(w1, curve), "W2": kzg.point_to_json(w2, curve)}
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("kzg_open: %d polynomial(s) at %d point(s) in one two-point proof under %s -> %s" % (len(polys), sum(len(s) for s in sets), a.ptau, a.out))
    h.free()
    return 0


def kzg_open(a):
    sets = at_groups(a)
    if sets is not None:
        return kzg_open_multi(a, sets)
    kzg, h, curve = _open_handle(a)
    z = int(a.at, 0)
    if not 0 <= z < kzg._FR[curve]:
        print("zkgpu_kzg: --at is not below the scalar field's modulus")
        return 1
    polys = [read_poly(kzg, p, curve) for p in a.poly]
    cs = [h.commit(p) for p in polys]
    out = {"protocol": "kzg", "curve": curve, "z": str(z), "commitments": [kzg.point_to_json(c, curve) for c in cs]}
    if len(polys) == 1:
        y, w = h.open(polys[0], z)
        ys = [y]
    else:
        gamma = kzg.gamma_of(curve, cs, z)
        ys, w = h.open_many(polys, z, gamma)
        out["gamma"] = str(gamma)
    out["values"] = [str(y) for y in ys]
    out["witness"] = kzg.point_to_json(w, curve)
    pathlib.Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("kzg_open: %d polynomial(s) at %d under %s -> %s" % (len(polys), z, a.ptau, a.out))
    h.free()
    return 0


def load_multi(kzg, curve, path, js):
    """multi_opening.json -> ("multi", (commitments, sets, values, gamma, z, W1, W2)) with gamma and z recomputed from the file's own contents;
    ("multi", None) when a point or a value is not below r: nothing to hash"""
    cs = [kzg.point_from_json(c, curve) for c in js["commitments"]]
    sets = [[int(p, 0) for p in s] for s in js["sets"]]
    values = [[int(y, 0) for y in ys] for ys in js["values"]]
    if not cs or len(sets) != len(cs) or len(values) != len(cs) or any(len(s) != len(v) for s, v in zip(sets, values)):
        raise SystemExit("zkgpu_kzg: %s: a set and a list of values for every commitment, a value for every point, and at least one commitment" % path)
    w1, w2 = kzg.point_from_json(js["W1"], curve), kzg.point_from_json(js["W2"], curve)
    r = kzg._FR[curve]
    if not all(0 <= v < r for row in sets + values for v in row):
        return "multi", None
    gamma = kzg.challenges_of(curve, cs, sets, values)
    return "multi", (cs, sets, values, gamma, kzg.challenge_z(curve, gamma, w1, avoid=[p for s in sets for p in s]), w1, w2)


def load_opening(kzg, h, curve, path):
    """opening.json -> ("single", (C, z, y, W)) with the several-polynomial form folded by the gamma recomputed from the file's own commitments,
    the proof None for a several-polynomial opening whose z or a value is not below r; multi_opening.json -> load_multi"""
    js = json.loads(pathlib.Path(path).read_text())
    if js.get("curve") != curve:
        raise SystemExit("zkgpu_kzg: %s is an opening on %s, the file is %s" % (path, js.get("curve"), curve))
    if js.get("protocol") == "kzg-multi":
        return load_multi(kzg, curve, path, js)
    return "single", load_single(kzg, h, curve, path, js)


def load_single(kzg, h, curve, path, js):
    cs = [kzg.point_from_json(c, curve) for c in js["commitments"]]
    ys = [int(v, 0) for v in js["values"]]
    z = int(js["z"], 0)
    if len(cs) != len(ys) or not cs:
        raise SystemExit("zkgpu_kzg: %s: as many values as commitments, and at least one" % path)
    w = kzg.point_from_json(js["witness"], curve)
    if len(cs) == 1:
        return cs[0], z, ys[0], w
    r = kzg._FR[curve]
    if not (0 <= z < r and all(0 <= y < r for y in ys)):
        return None                                                       # nothing to fold: the caller reports it
    gamma = kzg.gamma_of(curve, cs, z)
    return h.fold_commitments(cs, gamma), z, h.fold_values(ys, gamma), w


def kzg_verify(a):
    kzg, h, curve = _open_handle(a)
    ops = [load_opening(kzg, h, curve, p) for p in a.openings]
    check = {"single": h.verify, "multi": h.verify_multi}                # the files of each kind batched among themselves
    verdict = 1
    for kind, fn in check.items():
        mine = [op for k, op in ops if k == kind]
        if mine and verdict == 1:
            verdict = 0 if None in mine else fn(mine)[0]
    if verdict == 1:
        print("kzg_verify: %d opening(s) accepted under %s" % (len(ops), a.ptau))
        h.free()
        return 0
    for path, (kind, op) in zip(a.openings, ops):                        # one line per opening that is not accepted
        v = -1 if op is None else check[kind]([op])[0]
        if v != 1:
            print("kzg_verify: %s: %s" % (path, REASONS.get(v, "verdict %d" % v)))
    h.free()
    return 1


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p):
        p.add_argument("-c", "--curve", choices=CURVES, default=None)
        p.add_argument("--ptau", required=True)
        p.add_argument("--no-check-srs", dest="no_check_srs", action="store_true", help="skip the check of the file's points and structure")
    c = sub.add_parser("kzg_commit"); common(c)
    c.add_argument("--poly", action="append", required=True); c.add_argument("--evals", action="store_true"); c.add_argument("-o", dest="out", required=True)
    c.set_defaults(fn=kzg_commit)
    o = sub.add_parser("kzg_open"); common(o)

    class At(argparse.Action):                                            # --at keeps its text, and which --poly it followed: at_groups() reads the groups
        def __call__(self, parser, ns, value, option_string=None):
            ns.at = value
            ns.at_marks = (getattr(ns, "at_marks", None) or []) + [(len(ns.poly or []), value)]
    o.add_argument("--poly", action="append", required=True); o.add_argument("--at", required=True, action=At); o.add_argument("-o", dest="out", required=True)
    o.set_defaults(fn=kzg_open)
    v = sub.add_parser("kzg_verify"); common(v)
    v.add_argument("openings", nargs="+")
    v.set_defaults(fn=kzg_verify)
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "kzg_commit" and len(a.poly) != 1:
        ap.error("kzg_commit takes one --poly")
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
