"""An fflonk prover and verifier with tagged lookups (several tables in one circuit) over a powers-of-tau file, on the device (eigen_zkvm_amd.fflonk_lookup_tagged), on files.

    python tools/zkgpu_fflonk_lookup_tagged.py fflonk_lookup_tagged_setup  [-c CURVE] --ptau F --circuit C.npz -v vk.json [--no-check-srs]
    python tools/zkgpu_fflonk_lookup_tagged.py fflonk_lookup_tagged_prove  [-c CURVE] --ptau F --circuit C.npz --witness w.bin --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_fflonk_lookup_tagged.py fflonk_lookup_tagged_verify [-c CURVE] -v vk.json --ptau F proof.json:public.json [proof.json:public.json ...] [--no-check-srs]

C.npz is the TAGGED gate table with lookups of tools/zkgpu_plonk_lookup.py (eigen_zkvm_amd.plonk_lookup.LookupCircuit(tables=...).save), the
same file: it holds table_tag, qK is 0 .. K per gate and names the table a row is looked up in.  A C.npz of one untagged table is refused with
one line: tools/zkgpu_fflonk_lookup.py proves it.  w.bin, public.json, --no-check-srs and CURVE are as for tools/zkgpu_plonk.py.
vk.json holds TWO points, [C0] and [C0L]; proof.json five points and 23 values.  There is no proving-key file: fflonk_lookup_tagged_prove
rebuilds the key from the circuit and the .ptau, which must hold 8n + 8 G1 powers for n rows (fflonk_lookup_tagged_setup prints n, that
number, the smallest file power that has them, the number of tables and their sizes).  --r1cs is refused: a circuit compiled from an .r1cs
has no lookups.
fflonk_lookup_tagged_prove checks the witness against the gates first, then against the tables, and names the first row that fails with the
number of such rows and the table its qK names.  fflonk_lookup_tagged_verify checks all the proofs in one randomised pairing equation (two
pairings) and exits 0 when every proof is accepted; otherwise it checks them one by one, prints one line per proof that is not accepted --
`fflonk_lookup_tagged_verify: FILE: <reason>` -- and exits 1.  A key or a proof of tools/zkgpu_plonk.py, tools/zkgpu_fflonk.py,
tools/zkgpu_plonk_lookup.py or tools/zkgpu_fflonk_lookup.py is refused here with one line, and this tool's are refused there."""
import importlib, pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import plonk_cli, zkgpu_kzg  # noqa: E402

REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the opening that carries the identities does not hold", -1: "a value or a public input is not below r"})


def _need(head, key, powers, file_power):
    """what the file must hold, and the tables' sizes beside the gates': they may be what sets n"""
    c = key.circuit
    return ["fflonk_lookup_tagged_setup: n = 2^%d = %d rows need 8n + 8 = %d powers (a file of power %d has them)" % (key.log_n, key.n, powers, file_power),
            "fflonk_lookup_tagged_setup: %d tagged tables of %s rows (%d in all), %d of the gates look a row up" % (len(c.table_sizes), ", ".join(str(s) for s in c.table_sizes), c.n_table,
                                                                                                                  int((c.gates["qK"][:, 0] != 0).sum()))]


TOOL = plonk_cli.Tool("zkgpu_fflonk_lookup_tagged", "fflonk_lookup_tagged", "eigen_zkvm_amd.fflonk_lookup_tagged", "FflonkLookupTaggedKey", REASONS, _need, __doc__.splitlines()[0])


def split_pair(text):
    return plonk_cli.split_pair(TOOL, text)


def build_parser():
    return plonk_cli.build_parser(TOOL)


def main(argv=None):
    """a key or a proof file of another prover is refused with one line and exit code 1"""
    try:
        return plonk_cli.main(TOOL, argv)
    except importlib.import_module("eigen_zkvm_amd").ZkError as e:
        print("%s: %s" % (TOOL.name, e))
        return 1


if __name__ == "__main__":
    sys.exit(main())
