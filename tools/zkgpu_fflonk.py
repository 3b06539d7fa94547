"""An fflonk prover and verifier over a powers-of-tau file, on the device (eigen_zkvm_amd.fflonk), on files.

    python tools/zkgpu_fflonk.py fflonk_setup  [-c CURVE] --ptau F --circuit C.npz -v vk.json [--no-check-srs]
    python tools/zkgpu_fflonk.py fflonk_setup  [-c CURVE] --ptau F --r1cs C.r1cs -v vk.json [--no-check-srs]
    python tools/zkgpu_fflonk.py fflonk_prove  [-c CURVE] --ptau F --circuit C.npz --witness w.bin --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_fflonk.py fflonk_prove  [-c CURVE] --ptau F --r1cs C.r1cs --wtns w.wtns --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_fflonk.py fflonk_verify [-c CURVE] -v vk.json --ptau F proof.json:public.json [proof.json:public.json ...] [--no-check-srs]

The files are those of tools/zkgpu_plonk.py: C.npz a gate table (eigen_zkvm_amd.plonk.Circuit.save), w.bin n_vars x 32 little-endian bytes,
C.r1cs / w.wtns a circom circuit and its witness, public.json the public inputs as decimal strings.  vk.json holds ONE point, [C0]; proof.json
four points and 15 values.  There is no proving-key file: fflonk_prove rebuilds the key from the circuit and the .ptau, which must hold
9n + 18 G1 powers for n rows (fflonk_setup prints n, that number and the smallest file power that has them).

fflonk_prove checks the witness against the gates first and names the first row that fails.  fflonk_verify checks all the proofs in one
randomised pairing equation (two pairings) and exits 0 when every proof is accepted; otherwise it checks them one by one, prints one line per
proof that is not accepted -- `fflonk_verify: FILE: <reason>` -- and exits 1."""
import argparse, json, pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import zkgpu_kzg  # noqa: E402

CURVES = ("BN128", "BLS12381")
REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the opening that carries the identities does not hold", -1: "a value or a public input is not below r"})


def _open(a):
    """-> (fflonk module, Kzg handle, curve); the file's check first unless --no-check-srs"""
    import importlib
    _, h, curve = zkgpu_kzg._open_handle(a)
    return importlib.import_module("eigen_zkvm_amd.fflonk"), h, curve


def split_pair(text):
    parts = text.split(":")
    if len(parts) != 2 or not all(parts):
        raise SystemExit("zkgpu_fflonk: fflonk_verify takes proof.json:public.json pairs, not %r" % text)
    return parts[0], parts[1]


def _key(fflonk, h, curve, a):
    try:
        if a.r1cs is not None:
            return fflonk.FflonkKey(h, fflonk.R1csCircuit(pathlib.Path(a.r1cs).read_bytes(), curve))
        return fflonk.FflonkKey(h, fflonk.Circuit.load(a.circuit, curve))
    except fflonk.ZkError as e:
        print("zkgpu_fflonk: %s" % e)
        raise SystemExit(1)


def fflonk_setup(a):
    fflonk, h, curve = _open(a)
    key = _key(fflonk, h, curve, a)
    pathlib.Path(a.vk).write_text(fflonk.vk_to_json(key.vk))
    if a.r1cs is not None:
        print("fflonk_setup: %s: %d constraints -> %d gates, %d auxiliaries" % (a.r1cs, key.circuit.info["n_constraints"], key.circuit.n_gates, key.circuit.n_aux))
    print("fflonk_setup: n = 2^%d = %d rows need 9n + 18 = %d powers (a file of power %d has them)" % (key.log_n, key.n, fflonk.required_powers(key.n), fflonk.file_power(key.log_n)))
    print("fflonk_setup: %s, %d gates and %d public input(s) in n = 2^%d rows under %s (power %d) -> %s" % (a.r1cs or a.circuit, key.circuit.n_gates, key.circuit.n_public, key.log_n,
                                                                                                           a.ptau, h.power, a.vk))
    key.free(); h.free()
    return 0


def fflonk_prove(a):
    fflonk, h, curve = _open(a)
    key = _key(fflonk, h, curve, a)
    witness = a.wtns if a.r1cs is not None else a.witness
    try:
        proof, publics = fflonk.prove(key, pathlib.Path(witness).read_bytes())
    except fflonk.ZkError as e:
        print("zkgpu_fflonk: %s" % e)
        return 1
    finally:
        key.free()
    pathlib.Path(a.proof).write_text(fflonk.proof_to_json(proof, curve))
    pathlib.Path(a.public).write_text(json.dumps([str(x) for x in publics]) + "\n")
    print("fflonk_prove: %s over %s, n = 2^%d -> %s, %s" % (witness, a.r1cs or a.circuit, key.log_n, a.proof, a.public))
    h.free()
    return 0


def fflonk_verify(a):
    fflonk, h, curve = _open(a)
    vk = fflonk.vk_from_json(pathlib.Path(a.vk).read_text(), h)
    if vk.curve != curve:
        raise SystemExit("zkgpu_fflonk: %s is a key on %s, the file is %s" % (a.vk, vk.curve, curve))
    pairs = [split_pair(p) for p in a.pairs]
    proofs = [fflonk.proof_from_json(pathlib.Path(p).read_text(), curve) for p, _ in pairs]
    publics = [[int(x, 0) for x in json.loads(pathlib.Path(x).read_text())] for _, x in pairs]
    verdict, _ = fflonk.verify(vk, publics, proofs, locate=False)
    if verdict == 1:
        print("fflonk_verify: %d proof(s) accepted under %s" % (len(proofs), a.vk))
        h.free()
        return 0
    for (path, _), x, p in zip(pairs, publics, proofs):                   # one line per proof that is not accepted
        v = fflonk.verify(vk, [x], [p])[0]
        if v != 1:
            print("fflonk_verify: %s: %s" % (path, REASONS.get(v, "verdict %d" % v)))
    h.free()
    return 1


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p):
        p.add_argument("-c", "--curve", choices=CURVES, default=None)
        p.add_argument("--ptau", required=True)
        p.add_argument("--no-check-srs", dest="no_check_srs", action="store_true", help="skip the check of the file's points and structure")
    s = sub.add_parser("fflonk_setup"); common(s)
    g = s.add_mutually_exclusive_group(required=True)
    g.add_argument("--circuit", help="a gate table (Circuit.save)"); g.add_argument("--r1cs", help="a circom .r1cs over the curve's scalar field")
    s.add_argument("-v", dest="vk", required=True)
    s.set_defaults(fn=fflonk_setup)
    p = sub.add_parser("fflonk_prove"); common(p)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--circuit", help="a gate table (Circuit.save); goes with --witness"); g.add_argument("--r1cs", help="a circom .r1cs; goes with --wtns")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--witness", help="n_vars x 32 bytes"); g.add_argument("--wtns", help="the .wtns of the .r1cs")
    p.add_argument("--proof", required=True); p.add_argument("--public", required=True)
    p.set_defaults(fn=fflonk_prove)
    v = sub.add_parser("fflonk_verify"); common(v)
    v.add_argument("-v", dest="vk", required=True); v.add_argument("pairs", nargs="+", metavar="proof.json:public.json")
    v.set_defaults(fn=fflonk_verify)
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "fflonk_prove" and (a.r1cs is None) != (a.wtns is None):
        ap.error("--circuit goes with --witness, --r1cs with --wtns")
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
