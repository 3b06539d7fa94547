"""A PLONK prover and verifier with lookups over a powers-of-tau file, on the device (eigen_zkvm_amd.plonk_lookup), on files.

    python tools/zkgpu_plonk_lookup.py plonk_lookup_setup  [-c CURVE] --ptau F --circuit C.npz -v vk.json [--no-check-srs]
    python tools/zkgpu_plonk_lookup.py plonk_lookup_prove  [-c CURVE] --ptau F --circuit C.npz --witness w.bin --proof proof.json --public public.json [--no-check-srs]
    python tools/zkgpu_plonk_lookup.py plonk_lookup_verify [-c CURVE] -v vk.json --ptau F proof.json:public.json [proof.json:public.json ...] [--no-check-srs]

C.npz is a gate table with lookups (eigen_zkvm_amd.plonk_lookup.LookupCircuit.save): what tools/zkgpu_plonk.py's C.npz holds, and qK as (m, 4)
uint64 words (0 or 1 per gate) and table as (T, 3, 4) uint64 canonical words (the T rows t1, t2, t3).  A row with qK = 1 claims that its
(a, b, c) is a row of the table, by the log-derivative argument; n = 2^k >= 8 holds the public rows, the gates and the table, which is padded
by repeating its last row.  w.bin, public.json, the .ptau (3n + 6 G1 powers), --no-check-srs and CURVE are as for tools/zkgpu_plonk.py.
--r1cs is refused: a circuit compiled from an .r1cs has no lookups.
A C.npz that also holds table_tag ((T,) uint32: 1 .. K, the number of each row's table, in order) is a circuit of K >= 2 TAGGED tables
(LookupCircuit(tables=...)): qK is 0 .. K per gate and names the table a row is looked up in.  Nothing changes on the command
line: plonk_lookup_setup prints the number of tables and their sizes, the key and the proofs are of the protocol
"plonk-shplonk-lookup-tagged", a bad lookup is named with its row and the table its qK names, and plonk_lookup_verify refuses a proof of the
single-table protocol under a tagged key and the reverse.
plonk_lookup_prove checks the witness against the gates first, then against the table, and names the first row that fails with the number of
such rows.  plonk_lookup_verify checks all the proofs in one randomised pairing equation; it prints the count and exits 0 when all are
accepted, otherwise it prints one line per proof that is not accepted -- `plonk_lookup_verify: FILE: <reason>` -- and exits 1.  A key or a
proof of tools/zkgpu_plonk.py is refused here, and this tool's are refused there."""
import pathlib, sys
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools"))

import plonk_cli, zkgpu_kzg  # noqa: E402

REASONS = dict(zkgpu_kzg.REASONS)
REASONS.update({0: "the identity or the pairing equation does not hold", -1: "a value or a public input is not below r"})


def _need(head, key, powers, file_power):
    """the table's size beside the gates': it may be what sets n; of a tagged circuit, the number of tables and their sizes"""
    c = key.circuit
    if c.tagged:
        return ["plonk_lookup_setup: %d tagged tables of %s rows (%d in all), %d of the gates look a row up" % (len(c.table_sizes), ", ".join(str(s) for s in c.table_sizes), c.n_table,
                                                                                                             int((c.gates["qK"][:, 0] != 0).sum()))]
    return ["plonk_lookup_setup: a table of %d rows, %d of the gates look a row up" % (key.circuit.n_table, int(key.circuit.gates["qK"][:, 0].sum()))]


TOOL = plonk_cli.Tool("zkgpu_plonk_lookup", "plonk_lookup", "eigen_zkvm_amd.plonk_lookup", "LookupKey", REASONS, _need, __doc__.splitlines()[0])


def split_pair(text):
    return plonk_cli.split_pair(TOOL, text)


def build_parser():
    return plonk_cli.build_parser(TOOL)


def main(argv=None):
    return plonk_cli.main(TOOL, argv)


if __name__ == "__main__":
    sys.exit(main())
