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
import pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import plonk_cli, zkgpu_kzg  # noqa: E402

REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the opening that carries the identities does not hold", -1: "a value or a public input is not below r"})


def _need(head, key, powers, file_power):
    """fflonk's setup always says what the file must hold, in a line of its own"""
    return ([head] if head else []) + ["fflonk_setup: n = 2^%d = %d rows need 9n + 18 = %d powers (a file of power %d has them)" % (key.log_n, key.n, powers, file_power)]


TOOL = plonk_cli.Tool("zkgpu_fflonk", "fflonk", "eigen_zkvm_amd.fflonk", "FflonkKey", REASONS, _need, __doc__.splitlines()[0])


def split_pair(text):
    return plonk_cli.split_pair(TOOL, text)


def build_parser():
    return plonk_cli.build_parser(TOOL)


def main(argv=None):
    return plonk_cli.main(TOOL, argv)


if __name__ == "__main__":
    sys.exit(main())
