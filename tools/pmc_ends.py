"""Per-dispatch counter averages of the C2 frame's two streaming ends (the stem and the logits up-sample) from rocprofv3 --pmc passes
over tools/profile_frame.py (counters only: one pass per counter group, never together with a trace).

    python tools/pmc_ends.py <out.json> <counter_collection.csv> [<counter_collection.csv> ...]

Counters are summed over their instances per dispatch (GRBM_GUI_ACTIVE: the maximum) and averaged over the dispatches of the later three
quarters of each kernel's calls (the first quarter holds the warm-up and, in a run that tunes, the tuner's launches)."""
import collections, csv, json, re, sys

ENDS = ("stem_mfma_kernel", "bilinear_fwd_nchw_kernel", "bilinear_fwd_nchw_tiled_kernel")


def short(name):
    return re.sub(r"[<(].*$", "", re.sub(r"^void ", "", name)).replace("fs::", "")


def main():
    out = collections.defaultdict(dict)
    for path in sys.argv[2:]:
        disp = {}
        for r in csv.DictReader(open(path)):
            k = short(r["Kernel_Name"])
            if k not in ENDS:
                continue
            e = disp.setdefault(r["Dispatch_Id"], (k, collections.defaultdict(float)))
            v, n = float(r["Counter_Value"]), r["Counter_Name"]
            e[1][n] = max(e[1][n], v) if n == "GRBM_GUI_ACTIVE" else e[1][n] + v
        per = collections.defaultdict(list)
        for did in sorted(disp, key=int):
            per[disp[did][0]].append(disp[did][1])
        for k, rows in per.items():
            rows = rows[len(rows) // 4:]
            out[k]["dispatches"] = len(rows)
            for n in rows[0]:
                out[k][n] = sum(r[n] for r in rows) / len(rows)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
