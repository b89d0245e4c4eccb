"""How the known-key check's short kernels sit against k_fast_sums (DESIGN §5
round 12), from rocprofv3 CSVs of `bench.py --gpus 1`:

    python scripts/sums_overlap_report.py trace <kernel_trace.csv> [skip_first_sums]
    python scripts/sums_overlap_report.py pmc <counter_collection.csv>

trace: over consecutive k_fast_sums launches of all streams (ordered by
start), the time from one's end to the next's start (negative: the two
overlap), the kernels that start in a positive gap, how often two sums
overlap, each kernel's mean in-flight time and the share of it spent beside a
running k_fast_sums of another stream.  The first launches (table builds, warm-up) are skipped.
pmc: per kernel, the mean of every counter per launch (first launch of each
kernel skipped) with VGPR count and LDS block size.  One JSON object each."""
import csv
import json
import sys
from collections import defaultdict


def name(k):
    k = k.replace("(anonymous namespace)::", "").replace("void ", "")
    return k.split("(")[0]


def trace(path, skip):
    rows = list(csv.DictReader(open(path)))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name(r["Kernel_Name"]), r["Stream_Id"]) for r in rows)
    sums = [e for e in ev if e[2].startswith("k_fast_sums")][skip:]
    if len(sums) < 3:
        sys.exit("fewer than 3 k_fast_sums launches")
    t0, t1 = sums[0][0], sums[-1][1]
    gaps, inside = [], defaultdict(lambda: [0, 0.0])
    for a, b in zip(sums[:-1], sums[1:]):
        g = (b[0] - a[1]) / 1e3
        gaps.append(g)
        if g > 0:
            for e in ev:
                if a[1] <= e[0] < b[0] and not e[2].startswith("k_fast_sums"):
                    inside[e[2]][0] += 1
                    inside[e[2]][1] += (e[1] - e[0]) / 1e3
    # merged sums intervals: the time with at least one sums running
    busy, cur = 0, None
    for s, e, _, _ in sums:
        if cur is None or s > cur[1]:
            if cur:
                busy += cur[1] - cur[0]
            cur = [s, e]
        else:
            cur[1] = max(cur[1], e)
    busy += cur[1] - cur[0]
    # per kernel: in-flight time, and how much of it another stream's sums was running
    per = defaultdict(lambda: [0, 0.0, 0.0])
    win = [e for e in ev if t0 <= e[0] and e[1] <= t1]
    for e in win:
        p = per[e[2]]
        p[0] += 1
        p[1] += (e[1] - e[0]) / 1e3
        for s in sums:
            if s[3] != e[3] and s[0] < e[1] and e[0] < s[1]:
                p[2] += (min(e[1], s[1]) - max(e[0], s[0])) / 1e3
    pos = [g for g in gaps if g > 0]
    steps = len(sums) - 1
    return {
        "sums_launches": len(sums), "window_us": (t1 - t0) / 1e3, "us_per_sums_launch": (t1 - t0) / 1e3 / steps,
        "sums_running_share": busy / (t1 - t0),
        "sums_mean_us": sum(s[1] - s[0] for s in sums) / 1e3 / len(sums),
        "gap_mean_us": sum(gaps) / len(gaps), "gap_median_us": sorted(gaps)[len(gaps) // 2],
        "gap_positive_share": len(pos) / len(gaps), "gap_positive_mean_us": sum(pos) / max(1, len(pos)),
        "gap_positive_us_per_step": sum(pos) / steps,
        "no_sums_running_us_per_step": ((t1 - t0) - busy) / 1e3 / steps,
        "sums_overlapping_share": sum(1 for g in gaps if g < 0) / len(gaps),
        "started_in_gaps": {k: {"launches_per_gap": v[0] / max(1, len(pos)), "mean_us": v[1] / v[0]}
                            for k, v in sorted(inside.items())},
        "kernels": {k: {"launches": v[0], "mean_us": v[1] / v[0], "beside_other_sums_share": v[2] / v[1] if v[1] else 0.0}
                    for k, v in sorted(per.items())},
    }


def pmc(path):
    disp = defaultdict(dict)
    for r in csv.DictReader(open(path)):
        e = disp[int(r["Dispatch_Id"])]
        e["name"] = name(r["Kernel_Name"])
        e["grid"] = int(r["Grid_Size"])
        e["vgpr"] = int(r["VGPR_Count"])
        e["lds"] = int(r["LDS_Block_Size"])
        c = e.setdefault("c", {})
        c[r["Counter_Name"]] = c.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    out, seen = defaultdict(lambda: {"launches": 0, "c": defaultdict(float)}), set()
    for did in sorted(disp):
        e = disp[did]
        key = e["name"]
        if key not in seen:
            seen.add(key)
            continue
        o = out[key]
        o["launches"] += 1
        o["vgpr"], o["lds"], o["grid"] = e["vgpr"], e["lds"], e["grid"]
        for k, v in e["c"].items():
            o["c"][k] += v
    return {k: {"launches": o["launches"], "vgpr": o["vgpr"], "lds": o["lds"], "grid": o["grid"],
                **{c: v / o["launches"] for c, v in sorted(o["c"].items())}} for k, o in sorted(out.items())}


if __name__ == "__main__":
    if sys.argv[1] == "trace":
        print(json.dumps(trace(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 12), indent=1))
    else:
        print(json.dumps(pmc(sys.argv[2]), indent=1))
