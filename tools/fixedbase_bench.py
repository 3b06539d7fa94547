"""Fixed-base multiplication timing: python tools/fixedbase_bench.py [log_n] [reps]
[k_i]G for n = 2^log_n scalars on G1 and G2 of both curves: the window-table kernel with full-width scalars
(zk_*_mul_generator_fr_dev, csrc/fixedbase_impl.hip.h) and, beside it in the same process and alternating with it, the
bit-serial kernel with 64-bit scalars (zk_*_mul_generator_dev).  Host clock around a launch that ends in a device
synchronise; the first call of each kernel (code object, the generator's table) is not timed."""
import sys, time, pathlib
import numpy as np
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import eigen_zkvm_amd

R = {"bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     "bls12_381": 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001}


def main():
    log_n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    zk = eigen_zkvm_amd; zk.init(0)
    n = 1 << log_n
    rng = np.random.default_rng(1)
    sync = zk.lib().zk_dev_sync
    for curve in ("bn254", "bls12_381"):
        k256 = np.concatenate([rng.integers(0, 2**64, size=(n, 3), dtype=np.uint64), rng.integers(0, R[curve] >> 192, size=(n, 1), dtype=np.uint64)], axis=1)
        d256 = zk.DevArray.from_host(k256.reshape(-1))
        d64 = zk.DevArray.from_host(rng.integers(1, 2**64, size=n, dtype=np.uint64))
        for group in ("g1", "g2"):
            new = lambda: zk.mul_generator_fr(d256, curve, group=group)
            old = lambda: zk.g1_mul_generator(d64, curve, group=group)
            new(); old(); sync()
            t_new, t_old = [], []
            for _ in range(reps):
                for fn, ts in ((new, t_new), (old, t_old)):
                    sync(); t = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t)
            f = lambda ts: "min %.2f median %.2f max %.2f ms" % (min(ts) * 1e3, sorted(ts)[len(ts) // 2] * 1e3, max(ts) * 1e3)
            print(f"{curve} {group} n=2^{log_n}: window table, 255-bit scalars: {f(t_new)} = {n / min(t_new) / 1e6:.1f} M points/s | "
                  f"bit-serial, 64-bit scalars: {f(t_old)} = {n / min(t_old) / 1e6:.1f} M points/s", flush=True)


if __name__ == "__main__":
    main()
