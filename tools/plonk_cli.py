"""The command-line body that tools/zkgpu_plonk.py, tools/zkgpu_fflonk.py, tools/zkgpu_plonk_lookup.py and tools/zkgpu_plonk_next.py share: <prefix>_setup, <prefix>_prove, <prefix>_verify on files, for
a prover over eigen_zkvm_amd.plonk_arith.  A tool is a Tool record and delegates; its own docstring says what its files hold."""
import argparse, collections, importlib, json, pathlib

import zkgpu_kzg

CURVES = ("BN128", "BLS12381")
# name: the tool's, in front of its errors; prefix: of its three commands and of their lines; module: the prover's; key: its key class's name;
# reasons: verdict -> the words <prefix>_verify prints; need(head, key, powers, file_power) -> the lines of <prefix>_setup that say what the
# circuit needs of the file, head being the line of an .r1cs's counts (None for a gate table); about: the parser's description
Tool = collections.namedtuple("Tool", "name prefix module key reasons need about")


def _open(tool, a):
    """-> (the prover's module, Kzg handle, curve); the file's check first unless --no-check-srs"""
    _, h, curve = zkgpu_kzg._open_handle(a)
    return importlib.import_module(tool.module), h, curve


def split_pair(tool, text):
    parts = text.split(":")
    if len(parts) != 2 or not all(parts):
        raise SystemExit("%s: %s_verify takes proof.json:public.json pairs, not %r" % (tool.name, tool.prefix, text))
    return parts[0], parts[1]


def refuse_r1cs(tool, mod, a):
    """a prover whose module names its own circuit class (CIRCUIT) and no class for an .r1cs (R1CS_CIRCUIT) proves gate tables only: --r1cs
    is refused with one line"""
    if a.r1cs is not None and hasattr(mod, "CIRCUIT") and not hasattr(mod, "R1CS_CIRCUIT"):
        print("%s: %s takes no --r1cs: a circuit compiled from an .r1cs has no lookups (tools/zkgpu_plonk.py proves it)" % (tool.name, a.cmd))
        raise SystemExit(1)


def _key(tool, mod, h, curve, a):
    try:
        circuit = getattr(mod, getattr(mod, "R1CS_CIRCUIT", "R1csCircuit"))(pathlib.Path(a.r1cs).read_bytes(), curve) if a.r1cs is not None else getattr(mod, getattr(mod, "CIRCUIT", "Circuit")).load(a.circuit, curve)
        return getattr(mod, tool.key)(h, circuit)
    except mod.ZkError as e:
        print("%s: %s" % (tool.name, e))
        raise SystemExit(1)


def setup(tool, a):
    mod, h, curve = _open(tool, a)
    key = _key(tool, mod, h, curve, a)
    pathlib.Path(a.vk).write_text(mod.vk_to_json(key.vk))
    head = None
    if a.r1cs is not None:
        head = "%s_setup: %s: %d constraints -> %d gates, %d auxiliaries" % (tool.prefix, a.r1cs, key.circuit.info["n_constraints"], key.circuit.n_gates, key.circuit.n_aux)
    powers = mod.required_powers(key.n)
    for line in tool.need(head, key, powers, importlib.import_module("eigen_zkvm_amd.plonk_arith").smallest_power(powers)):
        print(line)
    print("%s_setup: %s, %d gates and %d public input(s) in n = 2^%d rows under %s (power %d) -> %s" % (tool.prefix, a.r1cs or a.circuit, key.circuit.n_gates, key.circuit.n_public,
                                                                                                      key.log_n, a.ptau, h.power, a.vk))
    key.free(); h.free()
    return 0


def prove(tool, a):
    mod, h, curve = _open(tool, a)
    key = _key(tool, mod, h, curve, a)
    witness = a.wtns if a.r1cs is not None else a.witness
    try:
        proof, publics = mod.prove(key, pathlib.Path(witness).read_bytes())
    except mod.ZkError as e:
        print("%s: %s" % (tool.name, e))
        return 1
    finally:
        key.free()
    pathlib.Path(a.proof).write_text(mod.proof_to_json(proof, curve))
    pathlib.Path(a.public).write_text(json.dumps([str(x) for x in publics]) + "\n")
    print("%s_prove: %s over %s, n = 2^%d -> %s, %s" % (tool.prefix, witness, a.r1cs or a.circuit, key.log_n, a.proof, a.public))
    h.free()
    return 0


def verify(tool, a):
    mod, h, curve = _open(tool, a)
    vk = mod.vk_from_json(pathlib.Path(a.vk).read_text(), h)
    if vk.curve != curve:
        raise SystemExit("%s: %s is a key on %s, the file is %s" % (tool.name, a.vk, vk.curve, curve))
    pairs = [split_pair(tool, p) for p in a.pairs]
    which = {"tagged": vk.tagged} if hasattr(vk, "tagged") else {}     # a prover with two protocols reads a proof as one of its key's
    proofs = [mod.proof_from_json(pathlib.Path(p).read_text(), curve, **which) for p, _ in pairs]
    publics = [[int(x, 0) for x in json.loads(pathlib.Path(x).read_text())] for _, x in pairs]
    verdict, _ = mod.verify(vk, publics, proofs, locate=False)
    if verdict == 1:
        print("%s_verify: %d proof(s) accepted under %s" % (tool.prefix, len(proofs), a.vk))
        h.free()
        return 0
    for (path, _), x, p in zip(pairs, publics, proofs):                   # one line per proof that is not accepted
        v = mod.verify(vk, [x], [p])[0]
        if v != 1:
            print("%s_verify: %s: %s" % (tool.prefix, path, tool.reasons.get(v, "verdict %d" % v)))
    h.free()
    return 1


def build_parser(tool):
    ap = argparse.ArgumentParser(description=tool.about)
    sub = ap.add_subparsers(dest="cmd", required=True)

    def common(p, fn):
        p.add_argument("-c", "--curve", choices=CURVES, default=None)
        p.add_argument("--ptau", required=True)
        p.add_argument("--no-check-srs", dest="no_check_srs", action="store_true", help="skip the check of the file's points and structure")
        p.set_defaults(fn=lambda a: fn(tool, a))
    s = sub.add_parser(tool.prefix + "_setup"); common(s, setup)
    g = s.add_mutually_exclusive_group(required=True)
    g.add_argument("--circuit", help="a gate table (Circuit.save)"); g.add_argument("--r1cs", help="a circom .r1cs over the curve's scalar field")
    s.add_argument("-v", dest="vk", required=True)
    p = sub.add_parser(tool.prefix + "_prove"); common(p, prove)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--circuit", help="a gate table (Circuit.save); goes with --witness"); g.add_argument("--r1cs", help="a circom .r1cs; goes with --wtns")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--witness", help="n_vars x 32 bytes"); g.add_argument("--wtns", help="the .wtns of the .r1cs")
    p.add_argument("--proof", required=True); p.add_argument("--public", required=True)
    v = sub.add_parser(tool.prefix + "_verify"); common(v, verify)
    v.add_argument("-v", dest="vk", required=True); v.add_argument("pairs", nargs="+", metavar="proof.json:public.json")
    return ap


def main(tool, argv=None):
    ap = build_parser(tool)
    a = ap.parse_args(argv)
    if a.cmd == tool.prefix + "_prove" and (a.r1cs is None) != (a.wtns is None):
        ap.error("--circuit goes with --witness, --r1cs with --wtns")
    if getattr(a, "r1cs", None) is not None:
        refuse_r1cs(tool, importlib.import_module(tool.module), a)
    return a.fn(a)
