"""The lines `zkgpu_prove.py groth16_key_check` prints, one per finding of a groth16.key_check report.  Plain text work: this module
imports nothing of the package, so it loads where the library is not built."""
POINT_CLASSES = ("infinity", "coordinate_range", "not_on_curve", "not_in_subgroup")


def key_check_line(f):
    """one finding of a key_check report as the line the command-line tool prints"""
    k = f["kind"]
    if k == "size":
        return "size: section %s has %d points, the circuit needs %d (the key of another circuit?)" % (f["section"], f["have"], f["want"])
    if k in POINT_CLASSES:
        return "%s: section %s: %d point%s, first at index %d" % (k, f["section"], f["n_points"], "" if f["n_points"] == 1 else "s", f["first_index"])
    if k == "g1_g2_mismatch":
        return "g1_g2_mismatch: %s: the G1 and G2 halves differ, first at index %d" % (f["section"], f["first_index"])
    return "vk_mismatch: %s differs from the key's embedded copy" % f["field"]


def key_check_skipped_line(s):
    """one entry of a report's "skipped" list"""
    return "skipped: %s of %s: %s" % (s["check"], s["section"], s["reason"])
