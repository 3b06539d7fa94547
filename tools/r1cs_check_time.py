"""wtns_check timing: python tools/r1cs_check_time.py [--prove] [bn128 [log2_constraints]] [gl [log2_uses]]

bn128  a circuit of 2^k constraints (default 20) from oracle.groth16.synthetic_r1cs with one long row of 4096 terms added:
       the time of R1csCheck(...) (parse + upload of the three matrices), of run() on a host witness (upload + conversion + check
       kernel + read-back) and of run() on a device-resident witness (conversion + check kernel + read-back); wall clock around
       the call, which returns after its last read-back; median of 5 after one warm-up.  The split between conversion, check kernel and read-back is the kernel table of
       `rocprofv3 --kernel-trace --stats -- python tools/r1cs_check_time.py bn128` (frn_canon_to_fe_kernel, r1cs_check_kernel).
       --prove adds, for the same circuit, key generation once and the time of prove + verify: the only way to learn that a
       witness is bad without this check.
gl     a with_custom-style circuit of 2^k Poseidon12 uses (default 16) over the plain circuit: the same three times."""
import json, pathlib, random, statistics, sys, time
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests")); sys.path.insert(0, str(ROOT / "oracle"))
import numpy as np
import eigen_zkvm_amd
zk = eigen_zkvm_amd; zk.init(0)
import importlib
R = importlib.import_module("eigen_zkvm_amd.r1cs")
import c12_setup_circuits as CIRC
import c12_setup_ref as REF
import groth16 as G


def timed(fn, reps=5):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3)


def measure(field, b, w, fs):
    t0 = time.perf_counter()
    chk = R.R1csCheck(field, b)
    new_ms = round((time.perf_counter() - t0) * 1e3, 1)
    host = np.frombuffer(b"".join(int(v).to_bytes(fs, "little") for v in w), dtype=np.uint64).copy()
    d = zk.DevArray.from_host(host)
    rep = chk.run(host)
    assert rep["findings"] == [] and not any(rep["n_failing"].values()), rep["findings"][:3]
    out = dict(chk.info, field=field, r1cs_bytes=len(b), new_ms=new_ms, run_host_ms=timed(lambda: chk.run(host)), run_dev_ms=timed(lambda: chk.run(d)))
    host[-fs // 8] ^= 1                                                     # the last wire: one failing row, so the second path is timed too
    d2 = zk.DevArray.from_host(host)
    out["run_dev_one_finding_ms"] = timed(lambda: chk.run(d2))
    d.free(); d2.free(); chk.free()
    return out


args = sys.argv[1:]
prove = "--prove" in args
args = [a for a in args if a != "--prove"] or ["bn128", "gl"]
i = 0
while i < len(args):
    what = args[i]; i += 1
    k = None
    if i < len(args) and args[i].isdigit(): k = int(args[i]); i += 1
    if what == "bn128":
        p = R.FIELDS["BN128"][1]
        r, w = G.synthetic_r1cs(p, 1 << (k or 20), seed=1)
        first = len(w); w.extend([p - 1] * 4096); w.append(4096)
        r["constraints"].append(([(j, p - 1) for j in range(first, first + 4096)], [(0, 1)], [(len(w) - 1, 1)]))
        b = REF.write_r1cs(len(w), r["n_pub_out"], r["n_pub_in"], len(w) - 1 - r["n_pub_out"], r["constraints"], field_size=32, prime=p)
        out = measure("BN128", b, w, 32)
        if prove:
            dev = importlib.import_module("eigen_zkvm_amd.groth16")
            t0 = time.perf_counter(); pk, vk = dev.keygen("BN128", b); out["keygen_s"] = round(time.perf_counter() - t0, 2)
            t0 = time.perf_counter(); S = dev.Groth16Setup("BN128", b, pk); out["setup_s"] = round(time.perf_counter() - t0, 2)
            wa = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in w), dtype=np.uint64).reshape(-1, 4)
            key = dev.Groth16VerifyingKey("BN128", vk)
            pub = [int(v) for v in w[1:S.n_inputs]]
            def prove_verify():
                js, _ = S.prove(wa)
                assert key.verify(js, pub) == dev.ACCEPTED
            prove_verify()
            out["prove_and_verify_ms"] = timed(prove_verify, 3)
            key.free(); S.free()
    elif what == "gl":
        n = 1 << (k or 16)
        rng = random.Random(2)
        b0, w = CIRC.plain_circuit(seed=2)
        uses = []
        rows = CIRC.poseidon_rows([rng.randrange(REF.P) for _ in range(12)])   # every use holds the same states, on wires of its own
        for _ in range(n):
            uses.append((1, list(range(len(w), len(w) + 372)))); w.extend(v for row in rows for v in row)
        b = REF.write_r1cs(len(w), 0, 3, len(w) - 4, REF.read_r1cs(b0)["constraints"], list(CIRC.ALL_TEMPLATES), uses)
        out = measure("GL", b, w, 8)
    else:
        raise SystemExit(__doc__)
    print(json.dumps(out), flush=True)
