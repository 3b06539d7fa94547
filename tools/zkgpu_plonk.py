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
import pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import plonk_cli, zkgpu_kzg  # noqa: E402

REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the identity or the pairing equation does not hold", -1: "a value or a public input is not below r"})


def _need(head, key, powers, file_power):
    """PLONK's setup says what the file must hold only with --r1cs, in the line of the file's counts"""
    return [head + "; n = 2^%d rows need 3n + 6 = %d powers (a file of power %d has them)" % (key.log_n, powers, file_power)] if head else []


TOOL = plonk_cli.Tool("zkgpu_plonk", "plonk", "eigen_zkvm_amd.plonk", "PlonkKey", REASONS, _need, __doc__.splitlines()[0])


def smallest_power(n_powers):
    """the smallest power of a .ptau file that holds n_powers G1 powers (plonk_arith.smallest_power)"""
    import importlib
    return importlib.import_module("eigen_zkvm_amd.plonk_arith").smallest_power(n_powers)


def split_pair(text):
    return plonk_cli.split_pair(TOOL, text)


def build_parser():
    return plonk_cli.build_parser(TOOL)


def main(argv=None):
    return plonk_cli.main(TOOL, argv)


if __name__ == "__main__":
    sys.exit(main())
