"""tools/pilc.py (the stand-in for pilcom, which the image lacks): the compiled PoseidonG fixture it made
(tests/golden/poseidong.pil.json) and the language on sources of its own.  Its agreement with pilcom on the reference's
source <-> compiled pairs needs the reference's .pil sources, which are not part of this repository."""
import json
import pathlib
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))


def test_poseidong_fixture_shape():
    """poseidong.pil:5-15: 4 + 12 + 2 constant and 12 + 4 + 3 committed columns, 12 publics, 38 identities"""
    d = json.load(open(ROOT / "tests" / "golden" / "poseidong.pil.json"))
    assert (d["nCommitments"], d["nConstants"], len(d["publics"]), len(d["polIdentities"])) == (19, 18, 12, 38)
    assert d["references"]["PoseidonG.C"] == {"type": "constP", "id": 4, "polDeg": 1024, "isArray": True, "len": 12}
    assert [p["idx"] for p in d["publics"]] == [0] * 8 + [1023] * 4
    assert all(d["expressions"][p["e"]]["deg"] <= 2 for p in d["polIdentities"])


def test_small_language_cases(tmp_path):
    import pilc
    src = """
    constant %N = 2**4;
    namespace T(%N);
      pol constant K[3], L;
      pol commit a[2], b;
      pol sq = a[1]*a[1];          // degree 2, referenced below -> quotient-reduced
      pol lin = 3*b + 0x10 - 2*8;  // folds to 3*b + 0
      public o = b(%N-1);
      (a[0]' - sq) * (1 - L) = 0;
      K[2]*(b - :o) = 0;
      {a[0], sq} in {K[0], K[1]};
    """
    f = tmp_path / "t.pil"; f.write_text(src)
    d = pilc.compile_pil(str(f))
    assert d["references"]["T.K"]["len"] == 3 and d["references"]["T.L"]["id"] == 3 and d["references"]["T.b"]["id"] == 2
    sq = d["expressions"][d["references"]["T.sq"]["id"]]
    assert sq["idQ"] == 0 and sq["deg"] == 1 and d["nQ"] == 1 and d["nIm"] == 2
    lin = d["expressions"][d["references"]["T.lin"]["id"]]
    assert lin["op"] == "sub" and lin["values"][0]["op"] == "add" and lin["values"][0]["values"][1] == {"op": "number", "deg": 0, "value": "16"}
    assert d["publics"] == [{"polType": "cmP", "polId": 2, "idx": 15, "id": 0, "name": "o"}]
    assert d["plookupIdentities"][0]["selF"] is None and len(d["plookupIdentities"][0]["f"]) == 2
    with pytest.raises(pilc.PilError, match="degree too high"):
        f.write_text("namespace T(8); pol commit a; a*a*a = 0;"); pilc.compile_pil(str(f))
    with pytest.raises(pilc.PilError, match="not defined"):
        f.write_text("namespace T(8); pol commit a; a*zz = 0;"); pilc.compile_pil(str(f))
