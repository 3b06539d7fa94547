"""A powers-of-tau file from a KNOWN trapdoor, for tests and profiles only:

    python tools/make_test_ptau.py --curve BN128|BLS12381 --power K --tau T --alpha A --beta B -o FILE [--sidecar FILE.json]

Whoever knows tau, alpha and beta of a file can forge proofs for every key made from it, and this tool takes them on its command line:
THE RESULT IS WORTHLESS AS A SETUP.  It exists because the setup from a file must give, byte for byte, the key of the trapdoor
(tau, alpha, beta, 1, 1), and that can only be checked where the trapdoor is known.

The container is snarkjs's .ptau as include/zkgpu.h (zk_srs_open) restates it: "ptau", u32 version 1, u32 section count, sections as
u32 id, u64 size, payload; 1 = n8, q, power, ceremonyPower; 2 = tauG1 (2 * 2^power - 1 points [tau^i] G1), 3 = tauG2 (2^power),
4 = alphaTauG1, 5 = betaTauG1 (2^power each), 6 = betaG2.  Points come from the device's fixed-base kernel (mul_generator_fr) in its own
layout -- uncompressed affine, little-endian Montgomery -- which is the file's."""
import argparse, json, pathlib, struct, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np

CURVES = {
    "BN128": dict(abi="bn254", n8=32, r=21888242871839275222246405745257275088548364400416034343698204186575808495617,
                  q=21888242871839275222246405745257275088696311157297823662689037894645226208583),
    "BLS12381": dict(abi="bls12_381", n8=48, r=0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001,
                     q=0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab),
}


def section_scalars(curve, power, tau, alpha, beta):
    """{section id: (group, the scalars whose multiples of the generator the section holds)}"""
    r = CURVES[curve]["r"]; n = 1 << power
    pw = [1]
    for _ in range(2 * n - 2):
        pw.append(pw[-1] * tau % r)
    return {2: ("g1", pw), 3: ("g2", pw[:n]), 4: ("g1", [alpha * p % r for p in pw[:n]]), 5: ("g1", [beta * p % r for p in pw[:n]]), 6: ("g2", [beta % r])}


def container(curve, power, payloads):
    """the file's bytes from {section id: payload bytes} for ids 2..6"""
    c = CURVES[curve]
    head = struct.pack("<I", c["n8"]) + c["q"].to_bytes(c["n8"], "little") + struct.pack("<II", power, power)
    out = b"ptau" + struct.pack("<II", 1, 6)
    for sid, body in [(1, head)] + [(i, payloads[i]) for i in range(2, 7)]:
        out += struct.pack("<IQ", sid, len(body)) + body
    return out


def build_ptau(zk, curve, power, tau, alpha, beta):
    """the file's bytes; zk: the loaded package (a GPU is needed: the points are made by mul_generator_fr)"""
    c = CURVES[curve]
    payloads = {}
    for sid, (group, ks) in section_scalars(curve, power, tau, alpha, beta).items():
        k = np.array([[(v >> (64 * i)) & (2**64 - 1) for i in range(4)] for v in ks], dtype=np.uint64)
        pts = zk.mul_generator_fr(zk.DevArray.from_host(k.reshape(-1)), c["abi"], group=group).to_host()
        payloads[sid] = pts[:len(ks) * c["n8"] // 8 * (4 if group == "g2" else 2)].astype("<u8").tobytes()
    return container(curve, power, payloads)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--curve", default="BN128", choices=sorted(CURVES))
    ap.add_argument("--power", type=int, required=True)
    for name in ("tau", "alpha", "beta"):
        ap.add_argument("--" + name, type=lambda s: int(s, 0), required=True)
    ap.add_argument("-o", dest="out", required=True)
    ap.add_argument("--sidecar", default=None, help="also write the trapdoor as json (tests read it next to the file)")
    a = ap.parse_args(argv)
    r = CURVES[a.curve]["r"]
    if not all(0 < v < r for v in (a.tau, a.alpha, a.beta)) or not 0 <= a.power <= 20:
        raise SystemExit("make_test_ptau: tau, alpha, beta in [1, r) and 0 <= power <= 20")
    import eigen_zkvm_amd as zk
    zk.init(0)
    b = build_ptau(zk, a.curve, a.power, a.tau, a.alpha, a.beta)
    pathlib.Path(a.out).write_bytes(b)
    if a.sidecar:
        pathlib.Path(a.sidecar).write_text(json.dumps({"curve": a.curve, "power": a.power, "tau": str(a.tau), "alpha": str(a.alpha), "beta": str(a.beta)}, indent=1) + "\n")
    print("make_test_ptau: %s, %d bytes, power %d -- the trapdoor of this file is known: it is WORTHLESS AS A SETUP, tests and profiles only" % (a.out, len(b), a.power))
    return 0


if __name__ == "__main__":
    sys.exit(main())
