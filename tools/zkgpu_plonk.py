"""A PLONK prover and verifier over a powers-of-tau file, on the device (eigen_zkvm_amd.plonk), on files.

    python tools/zkgpu_plonk.py plonk_setup  [-c CURVE] --ptau F --circuit C.npz -v vk.json [--no-check-srs]
    python tools/zkgpu_plonk.py plonk_setup  [-c CURVE] --ptau F --r1cs C.r1cs -v vk.json [--no-check-srs]
    python tools/zkgpu_plonk.py plonk_prove  [-c CURVE] --ptau F --circuit C.npz --witness w.bin --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_plonk.py plonk_prove  [-c CURVE] --ptau F --r1cs C.r1cs --wtns w.wtns --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_plonk.py plonk_verify [-c CURVE] -v vk.json --ptau F proof.json:public.json [proof.json:public.json ...] [--no-check-srs]

C.npz is a gate table (eigen_zkvm_amd.plonk.Circuit.save): qL, qR, qO, qM, qC as (m, 4) uint64 canonical words, a, b, c as uint32 variable
ids, n_vars and public (the variable ids of the public inputs).  Row i must satisfy qL a + qR b + qO c + qM a b + qC = 0; one row per public
input is put in front.  w.bin is n_vars x 32 bytes: the value of every variable, canonical little-endian (the p.bin of zkgpu_kzg.py).
C.r1cs is a circom circuit over the curve's scalar field and w.wtns its witness: the file is compiled to a gate table of fan-in 2 and
the auxiliary variables that table adds are computed from the witness on the device at every proof.  --circuit goes with --witness, --r1cs with --wtns.
public.json is the list of the public inputs as decimal strings.  There is no proving-key file: plonk_prove rebuilds the key from the circuit
and the .ptau, which must hold 3n + 6 G1 powers for the n = 2^k >= 8 rows of the padded table (a file of power k + 1 does).
Every subcommand opens the .ptau and runs the file's own check first, as zkgpu_kzg.py does; --no-check-srs skips it.  CURVE: BN128 | BLS12381;
without -c it is read from the .ptau header.
plonk_prove checks the witness against the gates first and names the first row that fails.  plonk_verify checks all the proofs in one
randomised pairing equation (two pairings); it prints the count and exits 0 when all are accepted, otherwise it prints one line per proof that
is not accepted -- `plonk_verify: FILE: <reason>` -- and exits 1."""
import argparse, json, pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import zkgpu_kzg  # noqa: E402

CURVES = ("BN128", "BLS12381")
REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the identity or the pairing equation does not hold", -1: "a value or a public input is not below r"})


def _open(a):
    """-> (plonk module, Kzg handle, curve); the file's check first unless --no-check-srs"""
    import importlib
    _, h, curve = zkgpu_kzg._open_handle(a)
    return importlib.import_module("eigen_zkvm_amd.plonk"), h, curve


def split_pair(text):
    parts = text.split(":")
    if len(parts) != 2 or not all(parts):
        raise SystemExit("zkgpu_plonk: plonk_verify takes proof.json:public.json pairs, not %r" % text)
    return parts[0], parts[1]


def _key(plonk, h, curve, a):
    try:
        if a.r1cs is not None:
            return plonk.PlonkKey(h, plonk.R1csCircuit(pathlib.Path(a.r1cs).read_bytes(), curve))
        return plonk.PlonkKey(h, plonk.Circuit.load(a.circuit, curve))
    except plonk.ZkError as e:
        print("zkgpu_plonk: %s" % e)
        raise SystemExit(1)


def smallest_power(n_powers):
    """the smallest power of a .ptau file that holds n_powers G1 powers: a file of power p has 2^(p + 1) - 1"""
    p = 0
    while (2 << p) - 1 < n_powers:
        p += 1
    return p


def plonk_setup(a):
    plonk, h, curve = _open(a)
    key = _key(plonk, h, curve, a)
    pathlib.Path(a.vk).write_text(plonk.vk_to_json(key.vk))
    if a.r1cs is not None:
        need = plonk.required_powers(key.n)
        print("plonk_setup: %s: %d constraints -> %d gates, %d auxiliaries; n = 2^%d rows need 3n + 6 = %d powers (a file of power %d has them)" % (
            a.r1cs, key.circuit.info["n_constraints"], key.circuit.n_gates, key.circuit.n_aux, key.log_n, need, smallest_power(need)))
    print("plonk_setup: %s, %d gates and %d public input(s) in n = 2^%d rows under %s (power %d) -> %s" % (a.r1cs or a.circuit, key.circuit.n_gates, key.circuit.n_public, key.log_n,
                                                                                                          a.ptau, h.power, a.vk))
    key.free(); h.free()
    return 0


def plonk_prove(a):
    plonk, h, curve = _open(a)
    key = _key(plonk, h, curve, a)
    witness = a.wtns if a.r1cs is not None else a.witness
    try:
        proof, publics = plonk.prove(key, pathlib.Path(witness).read_bytes())
    except plonk.ZkError as e:
        print("zkgpu_plonk: %s" % e)
        return 1
    finally:
        key.free()
    pathlib.Path(a.proof).write_text(plonk.proof_to_json(proof, curve))
    pathlib.Path(a.public).write_text(json.dumps([str(x) for x in publics]) + "\n")
    print("plonk_prove: %s over %s, n = 2^%d -> %s, %s" % (witness, a.r1cs or a.circuit, key.log_n, a.proof, a.public))
    h.free()
    return 0


def plonk_verify(a):
    plonk, h, curve = _open(a)
    vk = plonk.vk_from_json(pathlib.Path(a.vk).read_text(), h)
    if vk.curve != curve:
        raise SystemExit("zkgpu_plonk: %s is a key on %s, the file is %s" % (a.vk, vk.curve, curve))
    pairs = [split_pair(p) for p in a.pairs]
    proofs = [plonk.proof_from_json(pathlib.Path(p).read_text(), curve) for p, _ in pairs]
    publics = [[int(x, 0) for x in json.loads(pathlib.Path(x).read_text())] for _, x in pairs]
    verdict, _ = plonk.verify(vk, publics, proofs, locate=False)
    if verdict == 1:
        print("plonk_verify: %d proof(s) accepted under %s" % (len(proofs), a.vk))
        h.free()
        return 0
    for (path, _), x, p in zip(pairs, publics, proofs):                   # one line per proof that is not accepted
        v = plonk.verify(vk, [x], [p])[0]
        if v != 1:
            print("plonk_verify: %s: %s" % (path, REASONS.get(v, "verdict %d" % v)))
    h.free()
    return 1


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p):
        p.add_argument("-c", "--curve", choices=CURVES, default=None)
        p.add_argument("--ptau", required=True)
        p.add_argument("--no-check-srs", dest="no_check_srs", action="store_true", help="skip the check of the file's points and structure")
    s = sub.add_parser("plonk_setup"); common(s)
    g = s.add_mutually_exclusive_group(required=True)
    g.add_argument("--circuit", help="a gate table (Circuit.save)"); g.add_argument("--r1cs", help="a circom .r1cs over the curve's scalar field")
    s.add_argument("-v", dest="vk", required=True)
    s.set_defaults(fn=plonk_setup)
    p = sub.add_parser("plonk_prove"); common(p)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--circuit", help="a gate table (Circuit.save); goes with --witness"); g.add_argument("--r1cs", help="a circom .r1cs; goes with --wtns")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--witness", help="n_vars x 32 bytes"); g.add_argument("--wtns", help="the .wtns of the .r1cs")
    p.add_argument("--proof", required=True); p.add_argument("--public", required=True)
    p.set_defaults(fn=plonk_prove)
    v = sub.add_parser("plonk_verify"); common(v)
    v.add_argument("-v", dest="vk", required=True); v.add_argument("pairs", nargs="+", metavar="proof.json:public.json")
    v.set_defaults(fn=plonk_verify)
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "plonk_prove" and (a.r1cs is None) != (a.wtns is None):
        ap.error("--circuit goes with --witness, --r1cs with --wtns")
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
