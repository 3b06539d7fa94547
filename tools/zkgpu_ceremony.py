"""Powers-of-tau ceremonies and key contributions with proofs of knowledge, on the device.

    python tools/zkgpu_ceremony.py ptau_new -c CURVE --power K -o FILE
    python tools/zkgpu_ceremony.py ptau_contribute -c CURVE -i IN -o OUT [--check]
    python tools/zkgpu_ceremony.py ptau_beacon -i IN -o OUT --seed HEX --iter-log N
    python tools/zkgpu_ceremony.py ptau_verify -c CURVE FILE [--report OUT.json]
    python tools/zkgpu_ceremony.py key_contribute -c CURVE -p IN -o OUT --transcript T [-v VK]
    python tools/zkgpu_ceremony.py key_verify -c CURVE --initial A --final B --transcript T

ptau_new writes the file of tau = alpha = beta = 1 (no device needed).  ptau_contribute multiplies tau, alpha and beta by three factors
drawn from the operating system -- no flag takes one, and nothing of them survives the call -- and appends a record with proofs of
knowledge to the file's transcript.  ptau_beacon is a contribution whose factors anyone can recompute from the seed.  ptau_verify
checks the file (every point, every section the powers it claims) and the transcript (hash chain, proofs, beacons, the last images
against the file); findings print one per line and the exit status is 1 when there are any.  The result of a verified ceremony feeds
`zkgpu_prove.py groth16_setup --ptau` as it is.
key_contribute is `zkgpu_prove.py groth16_contribute` with a proof of knowledge of the ratio of the two deltas appended to the transcript
file T (created when absent: the chain then starts at IN); key_verify checks the chain and every proof from the initial key to the final
one and that nothing but delta, l and h moved between the two.  Whether the initial key is a delta = 1 key of its circuit stays
`zkgpu_prove.py groth16_key_check --ptau`'s question.  CURVE: BN128 | BLS12381; without -c it is read from the file's header."""
import argparse, json, pathlib, struct, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CURVES = ("BN128", "BLS12381")


def curve_of_file(path):
    """the curve a .ptau file's header names by the width of its prime (32 bytes: BN128, 48: BLS12381)"""
    with open(path, "rb") as f:
        head = f.read(28)
    if len(head) < 28 or head[:4] != b"ptau":
        raise SystemExit("zkgpu_ceremony: %s is no .ptau file" % path)
    sid, _size, n8 = struct.unpack_from("<IQI", head, 12)
    if sid != 1 or n8 not in (32, 48):
        raise SystemExit("zkgpu_ceremony: %s: give the curve with -c" % path)
    return "BN128" if n8 == 32 else "BLS12381"


def _dev():
    import importlib
    import eigen_zkvm_amd as zk
    zk.init(0)
    return zk, importlib.import_module("eigen_zkvm_amd.groth16")


def _verify(dev, curve, path, report_path=None):
    srs = dev.Srs(curve, path)
    rep = srs.verify()
    srs.free()
    if report_path:
        pathlib.Path(report_path).write_text(json.dumps(rep, indent=1) + "\n")
    lines = dev.srs_verify_lines(rep)
    for ln in lines:
        print(ln)
    print("ptau_verify: %s, power %d, %d contribution(s): %s" % (path, rep["power"], rep["contributions"], "%d finding(s)" % len(lines) if lines else "ok"))
    return 1 if lines else 0


def ptau_new(a):
    import importlib
    import eigen_zkvm_amd  # noqa: F401  (the library; no device is opened)
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    dev.srs_new(a.curve, a.power, a.out)
    print("ptau_new: %s, %s, power %d, tau = alpha = beta = 1: a ceremony starts here" % (a.out, a.curve, a.power))
    return 0


def ptau_contribute(a):
    curve = a.curve or curve_of_file(a.inp)
    zk, dev = _dev()
    srs = dev.Srs(curve, a.inp)
    srs.contribute(a.out)
    n = srs.transcript_count()
    srs.free()
    print("ptau_contribute: %s -> %s, contribution %d; the factors are gone" % (a.inp, a.out, max(n, 0) + 1))
    return _verify(dev, curve, a.out) if a.check else 0


def ptau_beacon(a):
    curve = a.curve or curve_of_file(a.inp)
    try:
        seed = bytes.fromhex(a.seed)
    except ValueError:
        seed = b""
    if len(seed) != 32:
        raise SystemExit("ptau_beacon: --seed is 32 bytes as 64 hex digits")
    zk, dev = _dev()
    srs = dev.Srs(curve, a.inp)
    srs.contribute(a.out, beacon=(seed, a.iter_log))
    srs.free()
    print("ptau_beacon: %s -> %s, seed %s, 2^%d iterations" % (a.inp, a.out, a.seed, a.iter_log))
    return 0


def ptau_verify(a):
    curve = a.curve or curve_of_file(a.file)
    zk, dev = _dev()
    return _verify(dev, curve, a.file, a.report)


def key_contribute(a):
    zk, dev = _dev()
    tp = pathlib.Path(a.transcript)
    old = pathlib.Path(a.pk_file).read_bytes()
    new, t = dev.contribute_pok(a.curve, old, tp.read_bytes() if tp.exists() else b"")
    pathlib.Path(a.out_file).write_bytes(new); tp.write_bytes(t)
    if a.vk_file:
        sys.path.insert(0, str(ROOT / "tools"))
        import zkgpu_prove
        pathlib.Path(a.vk_file).write_text(zkgpu_prove._vk_json_of_key(a.curve, new))
    print("key_contribute: %s -> %s, transcript %s; the delta is gone" % (a.pk_file, a.out_file, a.transcript))
    return 0


def key_verify(a):
    zk, dev = _dev()
    rd = lambda p: pathlib.Path(p).read_bytes()
    rep = dev.key_transcript_check(a.curve, rd(a.initial), rd(a.final), rd(a.transcript))
    lines = dev.key_transcript_lines(rep)
    for ln in lines:
        print(ln)
    print("key_verify: %d contribution(s) from %s to %s: %s" % (rep["contributions"], a.initial, a.final, "%d finding(s)" % len(lines) if lines else "ok"))
    return 1 if lines else 0


def build_parser():
    ap = argparse.ArgumentParser(prog="zkgpu_ceremony", description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("ptau_new", help="the file of tau = alpha = beta = 1 with an empty transcript")
    p.add_argument("-c", "--curve", required=True, choices=CURVES); p.add_argument("--power", type=int, required=True)
    p.add_argument("-o", dest="out", required=True); p.set_defaults(fn=ptau_new)
    p = sub.add_parser("ptau_contribute", help="one contribution with factors from the operating system")
    p.add_argument("-c", "--curve", choices=CURVES); p.add_argument("-i", dest="inp", required=True); p.add_argument("-o", dest="out", required=True)
    p.add_argument("--check", action="store_true", help="run ptau_verify on the result"); p.set_defaults(fn=ptau_contribute)
    p = sub.add_parser("ptau_beacon", help="a contribution whose factors anyone can recompute from a public seed")
    p.add_argument("-c", "--curve", choices=CURVES); p.add_argument("-i", dest="inp", required=True); p.add_argument("-o", dest="out", required=True)
    p.add_argument("--seed", required=True, help="32 bytes as hex"); p.add_argument("--iter-log", type=int, required=True, help="SHA-256 is iterated 2^N times over the seed")
    p.set_defaults(fn=ptau_beacon)
    p = sub.add_parser("ptau_verify", help="the file and its transcript; exit 1 with findings")
    p.add_argument("-c", "--curve", choices=CURVES); p.add_argument("file"); p.add_argument("--report", help="also write the report as json")
    p.set_defaults(fn=ptau_verify)
    p = sub.add_parser("key_contribute", help="one contribution to a key's delta with a proof of knowledge in the transcript file")
    p.add_argument("-c", "--curve", required=True, choices=CURVES); p.add_argument("-p", dest="pk_file", required=True); p.add_argument("-o", dest="out_file", required=True)
    p.add_argument("--transcript", required=True, help="read when it exists, written with one more record"); p.add_argument("-v", dest="vk_file", help="also write the new verification key")
    p.set_defaults(fn=key_contribute)
    p = sub.add_parser("key_verify", help="the chain of contributions from the initial key to the final one; exit 1 with findings. "
                       "Whether the initial key is a delta = 1 key of its circuit is `zkgpu_prove.py groth16_key_check --ptau`'s question")
    p.add_argument("-c", "--curve", required=True, choices=CURVES); p.add_argument("--initial", required=True); p.add_argument("--final", required=True)
    p.add_argument("--transcript", required=True); p.set_defaults(fn=key_verify)
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
