"""An fflonk prover and verifier with lookups over a powers-of-tau file, on the device (eigen_zkvm_amd.fflonk_lookup), on files.

    python tools/zkgpu_fflonk_lookup.py fflonk_lookup_setup  [-c CURVE] --ptau F --circuit C.npz -v vk.json [--no-check-srs]
    python tools/zkgpu_fflonk_lookup.py fflonk_lookup_prove  [-c CURVE] --ptau F --circuit C.npz --witness w.bin --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_fflonk_lookup.py fflonk_lookup_verify [-c CURVE] -v vk.json --ptau F proof.json:public.json [proof.json:public.json ...] [--no-check-srs]

C.npz is the gate table with lookups of tools/zkgpu_plonk_lookup.py (eigen_zkvm_amd.plonk_lookup.LookupCircuit.save), the same file: a row
with qK = 1 claims that its (a, b, c) is a row of the table, by the log-derivative argument; n = 2^k >= 8 holds the public rows, the gates and
the table, which is padded by repeating its last row.  w.bin, public.json, --no-check-srs and CURVE are as for tools/zkgpu_plonk.py.
vk.json holds TWO points, [C0] and [C0L]; proof.json five points and 22 values.  There is no proving-key file: fflonk_lookup_prove rebuilds
the key from the circuit and the .ptau, which must hold 8n + 8 G1 powers for n rows (fflonk_lookup_setup prints n, that number and the
smallest file power that has them).  --r1cs is refused: a circuit compiled from an .r1cs has no lookups.
fflonk_lookup_prove checks the witness against the gates first, then against the table, and names the first row that fails with the number
of such rows.  fflonk_lookup_verify checks all the proofs in one randomised pairing equation (two pairings) and exits 0 when every proof is
accepted; otherwise it checks them one by one, prints one line per proof that is not accepted -- `fflonk_lookup_verify: FILE: <reason>` --
and exits 1.  A key or a proof of tools/zkgpu_plonk.py, tools/zkgpu_fflonk.py or tools/zkgpu_plonk_lookup.py is refused here, and this
tool's are refused there."""
import pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import plonk_cli, zkgpu_kzg  # noqa: E402

REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the opening that carries the identities does not hold", -1: "a value or a public input is not below r"})


def _need(head, key, powers, file_power):
    """what the file must hold, and the table's size beside the gates': it may be what sets n"""
    return ["fflonk_lookup_setup: n = 2^%d = %d rows need 8n + 8 = %d powers (a file of power %d has them)" % (key.log_n, key.n, powers, file_power),
            "fflonk_lookup_setup: a table of %d rows, %d of the gates look a row up" % (key.circuit.n_table, int(key.circuit.gates["qK"][:, 0].sum()))]


TOOL = plonk_cli.Tool("zkgpu_fflonk_lookup", "fflonk_lookup", "eigen_zkvm_amd.fflonk_lookup", "FflonkLookupKey", REASONS, _need, __doc__.splitlines()[0])


def split_pair(text):
    return plonk_cli.split_pair(TOOL, text)


def build_parser():
    return plonk_cli.build_parser(TOOL)


def main(argv=None):
    return plonk_cli.main(TOOL, argv)


if __name__ == "__main__":
    sys.exit(main())
