"""A PLONK prover and verifier whose gate reads the next row, over a powers-of-tau file, on the device (eigen_zkvm_amd.plonk_next), on files.

    python tools/zkgpu_plonk_next.py plonk_next_setup  [-c CURVE] --ptau F --circuit C.npz -v vk.json [--no-check-srs]
    python tools/zkgpu_plonk_next.py plonk_next_setup  [-c CURVE] --ptau F --r1cs C.r1cs -v vk.json [--no-check-srs]
    python tools/zkgpu_plonk_next.py plonk_next_prove  [-c CURVE] --ptau F --circuit C.npz --witness w.bin --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_plonk_next.py plonk_next_prove  [-c CURVE] --ptau F --r1cs C.r1cs --wtns w.wtns --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_plonk_next.py plonk_next_verify [-c CURVE] -v vk.json --ptau F proof.json:public.json [proof.json:public.json ...] [--no-check-srs]

C.npz is a gate table (eigen_zkvm_amd.plonk_next.NextCircuit.save): what tools/zkgpu_plonk.py takes, and optionally qN as (m, 4) uint64 canonical
words.  Row i must satisfy qL a + qR b + qO c + qM a b + qC + qN c' = 0 with c' the c of the row after it (the row after the last is row 0); a
file without qN is the gate table of tools/zkgpu_plonk.py and is proved here with qN = 0.  w.bin is n_vars x 32 bytes, canonical little-endian.
C.r1cs is a circom circuit over the curve's scalar field and w.wtns its witness: the file is compiled under the CHAIN rule -- a sum of m >= 3
signals is a running sum down column c, two terms a row, in ceil(m / 2) gates -- and the auxiliary variables are computed from the witness
on the device at every proof.  --circuit goes with --witness, --r1cs with --wtns.  public.json is the list of the public inputs as decimal strings.
There is no proving-key file: plonk_next_prove rebuilds the key from the circuit and the .ptau, which must hold 3n + 7 G1 powers for the
n = 2^k >= 8 rows of the padded table (a file of power k + 1 does).  Every subcommand opens the .ptau and runs the file's own check first;
--no-check-srs skips it.  CURVE: BN128 | BLS12381; without -c it is read from the .ptau header.
A key or a proof of another tool is refused with one line, as this tool's are there.  plonk_next_prove checks the witness against the gates
first and names the first row that fails.  plonk_next_verify checks all the proofs in one randomised pairing equation (two pairings); it prints
the count and exits 0 when all are accepted, otherwise it prints one line per proof that is not accepted -- `plonk_next_verify: FILE: <reason>`
-- and exits 1."""
import pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import plonk_cli, zkgpu_kzg  # noqa: E402

REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the identity or the pairing equation does not hold", -1: "a value or a public input is not below r"})


def _need(head, key, powers, file_power):
    """what the file must hold, in the line of an .r1cs's counts"""
    return [head + "; n = 2^%d rows need 3n + 7 = %d powers (a file of power %d has them)" % (key.log_n, powers, file_power)] if head else []


TOOL = plonk_cli.Tool("zkgpu_plonk_next", "plonk_next", "eigen_zkvm_amd.plonk_next", "NextKey", REASONS, _need, __doc__.splitlines()[0])


def split_pair(text):
    return plonk_cli.split_pair(TOOL, text)


def build_parser():
    return plonk_cli.build_parser(TOOL)


def main(argv=None):
    """a key or a proof of another tool, or a malformed one, is one line and exit 1"""
    import eigen_zkvm_amd
    try:
        return plonk_cli.main(TOOL, argv)
    except eigen_zkvm_amd.ZkError as e:
        print("zkgpu_plonk_next: %s" % e)
        return 1


if __name__ == "__main__":
    sys.exit(main())
