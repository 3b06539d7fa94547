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


def srs_check_line(f):
    """one finding of an Srs.check report"""
    k = f["kind"]
    if k in POINT_CLASSES:
        return key_check_line(f)
    if k == "not_generator":
        return "not_generator: section %s does not start with the group's generator" % f["section"]
    if k == "not_powers":
        return "not_powers: section %s is not the sequence of powers of tau it claims to be" % f["section"]
    return "beta_mismatch: %s is not the beta of betaTauG1" % f["section"]


def contribution_check_line(f):
    """one finding of a contribution_check report"""
    k = f["kind"]
    if k == "size":
        return "size: section %s has %d points, the old key has %d" % (f["section"], f["have"], f["want"])
    if k in POINT_CLASSES:
        return key_check_line(f)
    if k == "changed":
        return "changed: section %s differs from the old key, first at index %d (a contribution touches delta, l and h only)" % (f["section"], f["first_index"])
    if k == "delta_mismatch":
        return "delta_mismatch: delta_g1 and delta_g2 of the new key hold different scalars"
    return "not_scaled: section %s of the new key is not the old one divided by the ratio of the two deltas" % f["section"]


def key_check_srs_line(f):
    """one finding of a groth16.key_check_srs report"""
    if f["kind"] == "query_mismatch":
        where = "index %d" % f["first_index"] + (" (wire %d)" % f["wire"] if "wire" in f else "")
        return "query_mismatch: section %s is not the circuit's over this powers-of-tau file, first at %s" % (f["section"], where)
    return "vk_mismatch: %s differs from the powers-of-tau file's" % f["field"]
