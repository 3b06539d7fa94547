"""Writes tests/golden/rust_shim_reference.json: what tests/test_rust_shim_traits.py checks the Rust shim against, taken once from
a checkout of the reference crates -- the MerkleTree / Transcript trait signatures (starky/src/traits.rs), the fft / ifft /
interpolate (fft_p.rs) and stark_prove (prove.rs) signatures, the public modules and item names of the starky and fields crates,
and the argument counts of StarkSetup::new, stark_verify and pil2circom with the fields of StarkOption.  Names and parsed
signatures only, in the test's own normal form (its parser).

usage: python tools/gen_rust_shim_golden.py REFERENCE_CHECKOUT"""
import json
import pathlib
import re
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import test_rust_shim_traits as T                                   # the parser the test applies to the shim

ITEM = re.compile(r"pub\s+(?:struct|enum|trait|fn|type|const|static|mod)\s+(\w+)\b")


def _pub_use_words(text):
    """every identifier of every `pub use ...;` -- the test asks whether an item is named in one"""
    return sorted({w for m in re.finditer(r"pub\s+use\s+([^;]*)", text) for w in re.findall(r"\w+", m.group(1))})


def _crate(src):
    lib = T._strip((src / "lib.rs").read_text())
    mods = re.findall(r"pub\s+mod\s+(\w+)\s*;", lib)
    modules = {}
    for m in mods:
        f = src / (m + ".rs")
        if f.exists():
            text = T._strip(f.read_text())
            modules[m] = {"pub_items": sorted(set(ITEM.findall(text))), "pub_use_words": _pub_use_words(text)}
    return {"lib_pub_mods": sorted(mods), "lib_pub_use_words": _pub_use_words(lib), "modules": modules}


def main(ref):
    ref = pathlib.Path(ref)
    st = ref / "starky" / "src"
    traits = {}
    tsrc = T._strip((st / "traits.rs").read_text())
    for trait in ("MerkleTree", "Transcript"):
        block = T._block(tsrc, r"pub\s+trait\s+%s\b" % trait)
        traits[trait] = {"methods": T._fns(block), "assoc_types": sorted(set(re.findall(r"\btype\s+(\w+)\s*[:;]", block)))}
    fft = T._fns(T._strip((st / "fft_p.rs").read_text()))
    p2c_src = T._strip((st / "pil2circom.rs").read_text())
    out = {
        "traits": traits,
        "fns": {"fft_p": {k: fft[k] for k in ("fft", "ifft", "interpolate")},
                "prove": {"stark_prove": T._fns(T._strip((st / "prove.rs").read_text()))["stark_prove"]}},
        "crates": {"starky": _crate(st), "fields": _crate(ref / "fields" / "src")},
        "arity": {
            "StarkSetup::new": len(T._fns(T._block(T._strip((st / "stark_setup.rs").read_text()), r"impl<[^>]*>\s*StarkSetup<[^>]*>"))["new"][2]),
            "stark_verify": len(T._fns(T._strip((st / "stark_verify.rs").read_text()))["stark_verify"][2]),
            "pil2circom": len(T._fns(p2c_src)["pil2circom"][2]),
        },
        "StarkOption_fields": sorted(set(re.findall(r"pub\s+(\w+)\s*:", T._block(p2c_src, r"pub\s+struct\s+StarkOption\b")))),
    }
    (ROOT / "tests" / "golden" / "rust_shim_reference.json").write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
