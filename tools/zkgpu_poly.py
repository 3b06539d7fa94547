"""Polynomial arithmetic over the scalar field on the device, on files: a product, an exact division by X^N - 1, a grand product.

    python tools/zkgpu_poly.py poly_mul       -c CURVE --poly a.bin --poly b.bin -o c.bin
    python tools/zkgpu_poly.py poly_divmod_zh -c CURVE --poly t.bin --log-n K -o q.bin [--rem r.bin]
    python tools/zkgpu_poly.py grand_product  -c CURVE --num n.bin --den d.bin -o z.bin

A file is n x 32 bytes: values below r, canonical little-endian (the p.bin of zkgpu_kzg.py); polynomials are coefficients, lowest degree
first.  A value that is not below r is refused by its index.  CURVE: BN128 | BLS12381.
poly_mul writes the len(a) + len(b) - 1 coefficients of a b.
poly_divmod_zh writes q with t = q (X^N - 1) + rem, N = 2^K (max(len(t) - N, 0) coefficients) and with --rem the N coefficients of rem.  When
X^N - 1 does not divide t it prints how many remainder coefficients are non-zero and the first of them, and exits 1 (the files are written all
the same).
grand_product writes z_0 .. z_(n-1) with z_0 = 1, z_(i+1) = z_i num_i / den_i and prints whether the product closes (z_n = 1: the two
products agree); exit 1 when it does not.  A zero denominator is an error that names its row.
These are the building blocks of eigen_zkvm_amd.frpoly; there is no protocol here."""
import argparse, pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CURVES = ("BN128", "BLS12381")


def _frpoly():
    import importlib
    import eigen_zkvm_amd as zk
    zk.init(0)
    return importlib.import_module("eigen_zkvm_amd.frpoly")


def read_values(fp, path, curve):
    b = pathlib.Path(path).read_bytes()
    if len(b) % 32:
        raise SystemExit("zkgpu_poly: %s: %d bytes is no whole number of 32-byte values" % (path, len(b)))
    r = fp._FR[curve]
    vals = [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]
    for i, v in enumerate(vals):
        if v >= r:
            print("zkgpu_poly: %s: value %d is not below the scalar field's modulus" % (path, i))
            raise SystemExit(1)
    return vals


def write_values(path, vals):
    pathlib.Path(path).write_bytes(b"".join(int(v).to_bytes(32, "little") for v in vals))


def poly_mul(a):
    fp = _frpoly()
    x, y = (read_values(fp, p, a.curve) for p in a.poly)
    if not x or not y:
        print("zkgpu_poly: poly_mul: an operand has no coefficients")
        return 1
    out = fp.poly_mul(x, y, a.curve)
    write_values(a.out, out)
    print("poly_mul: %d x %d coefficients -> %d in %s" % (len(x), len(y), len(out), a.out))
    return 0


def poly_divmod_zh(a):
    fp = _frpoly()
    t = read_values(fp, a.poly[0], a.curve)
    q, rem, bad = fp.divmod_zh(t, a.log_n, a.curve)
    write_values(a.out, q)
    if a.rem:
        write_values(a.rem, rem)
    if bad:
        first = next(i for i, v in enumerate(rem) if v)
        print("poly_divmod_zh: X^%d - 1 does not divide %s: %d non-zero remainder coefficient(s), the first at X^%d" % (1 << a.log_n, a.poly[0], bad, first))
        return 1
    print("poly_divmod_zh: %s = q (X^%d - 1) exactly, %d coefficients of q -> %s" % (a.poly[0], 1 << a.log_n, len(q), a.out))
    return 0


def grand_product(a):
    fp = _frpoly()
    num, den = read_values(fp, a.num, a.curve), read_values(fp, a.den, a.curve)
    if len(num) != len(den):
        print("zkgpu_poly: grand_product: %d numerators, %d denominators" % (len(num), len(den)))
        return 1
    try:
        z, last = fp.grand_product(num, den, a.curve)
    except fp.ZkError as e:
        print("zkgpu_poly: %s" % e)
        return 1
    write_values(a.out, z)
    if last == 1:
        print("grand_product: closes over %d rows (z_n = 1) -> %s" % (len(num), a.out))
        return 0
    print("grand_product: does NOT close over %d rows: z_n = %d -> %s" % (len(num), last, a.out))
    return 1


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p):
        p.add_argument("-c", "--curve", choices=CURVES, required=True)
        p.add_argument("-o", dest="out", required=True)
    m = sub.add_parser("poly_mul"); common(m)
    m.add_argument("--poly", action="append", required=True)
    m.set_defaults(fn=poly_mul)
    d = sub.add_parser("poly_divmod_zh"); common(d)
    d.add_argument("--poly", action="append", required=True); d.add_argument("--log-n", dest="log_n", type=int, required=True); d.add_argument("--rem", default=None)
    d.set_defaults(fn=poly_divmod_zh)
    g = sub.add_parser("grand_product"); common(g)
    g.add_argument("--num", required=True); g.add_argument("--den", required=True)
    g.set_defaults(fn=grand_product)
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "poly_mul" and len(a.poly) != 2:
        ap.error("poly_mul takes two --poly")
    if a.cmd == "poly_divmod_zh" and len(a.poly) != 1:
        ap.error("poly_divmod_zh takes one --poly")
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
