"""Groth16 prover timing on a synthetic circom-shaped circuit: python tools/groth16_bench.py [--real-key] [BN128|BLS12381] [log_rows ...]
Rows i: (w[p] + c w[q]) * w[t] = w[new_i] over earlier wires (satisfied; the quotient's top coefficient is checked
to be zero on the device result).  The proving key holds arbitrary valid points ([k]G with random 64-bit k, made
on the device): timing does not depend on the key being a real setup, proofs made here do not verify.
--real-key: the key comes from the library's own key generation (eigen_zkvm_amd.groth16.keygen, trapdoor drawn and
forgotten by the library) -- its time and split are printed, and proofs made with it are valid.
--verify [BN128|BLS12381] [batch ...]: the verification leg instead -- a key and a proof of a 2^8-row circuit made here, then the latency
of one verification and verifications per second at the batch sizes given (default 1 64 4096), proofs and inputs in host memory."""
import importlib, struct, sys, time, pathlib
import numpy as np
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import eigen_zkvm_amd

FR = {"BN128": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
      "BLS12381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}
NAME = {"BN128": "bn254", "BLS12381": "bls12_381"}


def make_circuit(r, log_rows, n_pub=1, n_prv=30, seed=1):
    """-> (r1cs bytes, witness n x 4 u64 canonical)"""
    rng = np.random.default_rng(seed)
    ni = 1 + n_pub
    n_rows = (1 << log_rows) - ni                       # + the prover's input rows = the whole domain
    first_new = ni + n_prv
    n_wires = first_new + n_rows - n_pub
    i = np.arange(n_rows)
    hi = first_new + np.maximum(i - n_pub, 0)           # wires defined before row i
    pick = lambda: (ni + np.floor(rng.random(n_rows) * (hi - ni))).astype(np.int64)
    p, q, t = pick(), pick(), pick()
    tgt = np.where(i < n_pub, 1 + i, first_new + i - n_pub)
    c = rng.integers(1, 1 << 30, size=n_rows)
    w = [0] * n_wires
    w[0] = 1
    for j in range(ni, first_new): w[j] = int(rng.integers(1, 2**62)) * int(rng.integers(1, 2**62)) % r
    for ti, pi, qi, tt, ci in zip(tgt.tolist(), p.tolist(), q.tolist(), t.tolist(), c.tolist()):
        w[ti] = (w[pi] + ci * w[qi]) % r * w[tt] % r
    term = np.dtype([("wire", "<u4"), ("coef", "<u8", 4)])
    row = np.dtype([("na", "<u4"), ("a", term, 2), ("nb", "<u4"), ("b", term, 1), ("nc", "<u4"), ("c", term, 1)])
    rec = np.zeros(n_rows, row)
    rec["na"], rec["nb"], rec["nc"] = 2, 1, 1
    rec["a"]["wire"][:, 0] = p; rec["a"]["coef"][:, 0, 0] = 1
    rec["a"]["wire"][:, 1] = q; rec["a"]["coef"][:, 1, 0] = c
    rec["b"]["wire"][:, 0] = t; rec["b"]["coef"][:, 0, 0] = 1
    rec["c"]["wire"][:, 0] = tgt; rec["c"]["coef"][:, 0, 0] = 1
    hdr = struct.pack("<I", 32) + r.to_bytes(32, "little") + struct.pack("<IIIIQI", n_wires, n_pub, 0, n_prv, n_wires, n_rows)
    body = rec.tobytes()
    wmap = np.arange(n_wires, dtype="<u8").tobytes()
    out = b"r1cs" + struct.pack("<II", 1, 3)
    for ty, sec in ((1, hdr), (2, body), (3, wmap)): out += struct.pack("<IQ", ty, len(sec)) + sec
    wit = np.array([[(v >> (64 * k)) & (2**64 - 1) for k in range(4)] for v in w], dtype=np.uint64)
    return out, wit, ni, n_wires


def random_points_be(zk, dev, curve, n, g2, seed):
    """n valid points as pairing_ce's uncompressed big-endian bytes"""
    if n == 0: return b""
    nl = 4 if curve == "BN128" else 6
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 2**64, size=n, dtype=np.uint64)
    d = zk.g1_mul_generator(zk.DevArray.from_host(k), NAME[curve], group="g2" if g2 else "g1")
    dev.fq_convert(d, curve, to_mont=False)
    a = d.to_host().reshape(n, 4 if g2 else 2, nl)
    if g2: a = a[:, [1, 0, 3, 2], :]                     # x.c1, x.c0, y.c1, y.c0
    return a[:, :, ::-1].astype(">u8").tobytes()


def make_params(zk, dev, curve, ni, n_wires, log_rows, r1cs_density):
    na, nb = r1cs_density
    m = 1 << log_rows
    P = lambda n, g2, s: random_points_be(zk, dev, curve, n, g2, s)
    out = [P(1, False, 1), P(1, False, 2), P(1, True, 3), P(1, True, 4), P(1, False, 5), P(1, True, 6), struct.pack(">I", ni), P(ni, False, 7)]
    for n, g2, s in ((m - 1, False, 8), (n_wires - ni, False, 9), (na, False, 10), (nb, False, 11), (nb, True, 12)):
        out += [struct.pack(">I", n), P(n, g2, s)]
    return b"".join(out)


def density(r1cs_bytes, ni, n_wires):
    """(|inputs| + |aux wires in any A row|, |wires in any B row|) for the fixed row shape of make_circuit"""
    term = np.dtype([("wire", "<u4"), ("coef", "<u8", 4)])
    row = np.dtype([("na", "<u4"), ("a", term, 2), ("nb", "<u4"), ("b", term, 1), ("nc", "<u4"), ("c", term, 1)])
    off = 12 + 12 + 64 + 12                              # file header, section header, 64-byte r1cs header, section header
    n_rows = struct.unpack("<I", r1cs_bytes[84:88])[0]
    rec = np.frombuffer(r1cs_bytes, dtype=row, count=n_rows, offset=off)
    a = np.unique(rec["a"]["wire"]); b = np.unique(rec["b"]["wire"])
    return ni + int((a >= ni).sum()), int(b.size)


def verify_leg(args):
    curve = args.pop(0) if args and args[0] in FR else "BN128"
    zk = eigen_zkvm_amd; zk.init(0)
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    rb, wit, ni, _ = make_circuit(FR[curve], 8)
    pb, vk_json = dev.keygen(curve, rb)
    S = dev.Groth16Setup(curve, rb, pb)
    js, pts = S.prove(wit); S.free()
    pub = [sum(int(v) << (64 * k) for k, v in enumerate(wit[i])) for i in range(1, ni)]
    t = time.perf_counter(); vk = dev.Groth16VerifyingKey(curve, vk_json); t_key = time.perf_counter() - t
    assert vk.verify(js, pub) == dev.ACCEPTED and vk.verify(js, [(pub[0] + 1) % FR[curve]]) == dev.REJECTED
    print(f"{curve}: key prepared in {t_key*1e3:.1f} ms", flush=True)
    for n in [int(a) for a in args] or [1, 64, 4096]:
        batch, pubs = np.tile(np.asarray(pts), n), [pub] * n
        assert vk.verify_batch(batch, pubs).tolist() == [1] * n                 # warm-up and check
        ts = []
        for _ in range(5):
            t = time.perf_counter(); vk.verify_batch(batch, pubs); ts.append(time.perf_counter() - t)
        ts.sort()
        print(f"  batch {n}: median {ts[2]*1e3:.2f} ms (min {ts[0]*1e3:.2f}, max {ts[-1]*1e3:.2f}) -> {n/ts[2]:.0f} verifications/s", flush=True)


def main():
    args = sys.argv[1:]
    if "--verify" in args:
        return verify_leg([a for a in args if a != "--verify"])
    real_key = "--real-key" in args
    args = [a for a in args if a != "--real-key"]
    curve = args.pop(0) if args and args[0] in FR else "BN128"
    zk = eigen_zkvm_amd; zk.init(0)
    dev = importlib.import_module("eigen_zkvm_amd.groth16")
    for log_rows in [int(a) for a in args] or [16, 20]:
        t = time.perf_counter()
        rb, wit, ni, n_wires = make_circuit(FR[curve], log_rows)
        t1 = time.perf_counter()
        if real_key:
            dev.keygen(curve, make_circuit(FR[curve], 8)[0])                # the generator's window tables are built once per process: not this key's time
            ms = []
            t1 = time.perf_counter()
            pb, _vk = dev.keygen(curve, rb, timing=ms)
            print(f"  keygen {(time.perf_counter() - t1)*1e3:.0f} ms: transform {ms[0]:.1f}, column sums {ms[1]:.1f}, G1 points {ms[2]:.1f}, G2 points {ms[3]:.1f}, "
                  f"serialisation {ms[4]:.1f} ms", flush=True)
        else:
            pb = make_params(zk, dev, curve, ni, n_wires, log_rows, density(rb, ni, n_wires))
        t2 = time.perf_counter()
        S = dev.Groth16Setup(curve, rb, pb)
        t3 = time.perf_counter()
        print(f"{curve} 2^{log_rows}: circuit {t1-t:.1f} s, key {t2-t1:.1f} s ({len(pb)/2**20:.0f} MiB), setup {t3-t2:.2f} s; wires {n_wires}", flush=True)
        assert S.domain_log == log_rows
        d_w = zk.DevArray.from_host(wit.reshape(-1))
        d_h = zk.DevArray(4 * ((1 << log_rows) - 1), zero=True)
        S.prove(d_w, 5, 7, d_h=d_h)
        ts = []
        for _ in range(5):
            t = time.perf_counter(); S.prove(d_w, 5, 7); ts.append(time.perf_counter() - t)
        th = []
        for _ in range(3):
            t = time.perf_counter(); S.prove(wit, 5, 7); th.append(time.perf_counter() - t)
        print(f"  prove: {min(ts)*1e3:.1f} ms witness resident, {min(th)*1e3:.1f} ms from host  ({(1 << log_rows)/min(ts)/1e6:.2f} M rows/s)", flush=True)
        # transforms alone
        x = zk.DevArray.from_host(wit[:1].repeat(1 << log_rows, axis=0).reshape(-1) * 0 + np.arange(4 << log_rows, dtype=np.uint64) % 1000)
        dev.fr_ntt(x, curve); zk.lib().zk_dev_sync()
        tn = []
        for _ in range(5):
            t = time.perf_counter(); dev.fr_ntt(x, curve); zk.lib().zk_dev_sync(); tn.append(time.perf_counter() - t)
        print(f"  one transform incl. layout changes: {min(tn)*1e3:.2f} ms", flush=True)
        S.free()


if __name__ == "__main__":
    main()
