"""First / middle / last pass of the three-pass transforms in a rocprofv3 kernel trace of bench.py: the two <4,4,false,*> launches
of a transform are told apart by their order behind the <4,4,true,*> launch.  usage: ntt_pass_split.py DIR_OR_CSV [skip_transforms]"""
import csv, glob, statistics, sys


def main():
    src = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    files = [src] if src.endswith(".csv") else glob.glob(f"{src}/**/*kernel_trace.csv", recursive=True)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "ntt_pass_kernel<4,4" in r["Kernel_Name"].replace(" ", "") or "ntt_pass_kernelILi4ELi4E" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    cls, pos, seen = {}, 0, 0
    for s, e, name in rows:
        n = name.replace(" ", "")
        kmode = "4,4,true" in n or "Lb1ELb" in n
        inv = n.split(">")[0].endswith("true") or "ELb1EEE" in n
        if kmode:
            pos, seen = 0, seen + 1
        else:
            pos += 1
        if seen <= skip or pos > 2:
            continue
        cls.setdefault((("first", "middle", "last")[pos], "inverse" if inv else "forward"), []).append((e - s) / 1000.0)
    for k in sorted(cls):
        v = cls[k]
        print(f"{k[0]:6s} {k[1]:7s} n={len(v):3d} min {min(v):6.2f} median {statistics.median(v):6.2f} mean {statistics.mean(v):6.2f} max {max(v):6.2f} us")


if __name__ == "__main__":
    main()
