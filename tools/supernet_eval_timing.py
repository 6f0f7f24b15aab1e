"""ms / image of the supernet validation (search_eval.SupernetEvaluator) on one GPU: the shared forward (one forward_lowres + one
fs_heads_confusion per image) against the reference's order (five sweeps, one head each: five forwards per image), and the
fs_heads_confusion kernel's own time from the library's census.

The F12.L16 search supernet (search/config_search.py: layers 16, Fch 12, five widths, prun_modes max / arch_ratio) with seeded
weights, `--images` seeded 512 x 1024 frames (the val split at down_sampling = 2), prun_mode "max" (fixed widths: both orders
compute the same counts).  Per dtype:
  shared_ms_per_image   device events around one run() after `--warmup` runs, divided by the image count;
  sweeps_ms_per_image   the same for share_forward=False;
  heads_confusion       one shared run() under the census (level 2: every launch of the library carries a start / stop event pair):
                        launches, device us per launch and algorithmic HBM bytes -> GB/s.
Prints one JSON line per dtype; --out writes them all to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
WML = [4. / 12, 6. / 12, 8. / 12, 10. / 12, 1.]


def build_supernet():
    from fasterseg_amd import archs, model_search
    net = model_search.Network_Multi_Path(19, 16, None, 12, WML, ['max', 'arch_ratio'], [(1, 1), (8. / 12, 8. / 12)])
    archs.init_weight(net, 12345)
    net = net.cuda().eval()
    net.arch_idx, net.prun_mode = 0, "max"
    return net


def source(n, H=512, W=1024):
    from fasterseg_amd.dataloader import ArraySource
    rng = np.random.RandomState(2024)
    imgs = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]
    lbls = []
    for _ in range(n):
        lbl = rng.randint(0, 19, (H, W)).astype(np.uint8)
        lbl[rng.rand(H, W) < 0.1] = 255
        lbls.append(lbl)
    return ArraySource(imgs, lbls, down_sampling=1)


def timed_run(ev, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        e0.record()
        ev.run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def measure(net, src, dtype, reps, warmup, census):
    from fasterseg_amd import census as C
    from fasterseg_amd.search_eval import SupernetEvaluator
    n = len(src)
    shared = SupernetEvaluator(net, 19, MEAN, STD, src, dtype=dtype, share_forward=True)
    sweeps = SupernetEvaluator(net, 19, MEAN, STD, src, dtype=dtype, share_forward=False)
    for _ in range(warmup):
        shared.run()
    torch.cuda.synchronize()
    row = {"dtype": "bf16" if dtype == torch.bfloat16 else "fp32", "images": n, "size": list(src.size(0)), "prun_mode": net.prun_mode}
    row["shared_ms_per_image"] = timed_run(shared, reps) / n
    row["sweeps_ms_per_image"] = timed_run(sweeps, reps) / n
    row["speedup"] = row["sweeps_ms_per_image"] / row["shared_ms_per_image"]
    a, b = shared.run(), sweeps.run()
    row["same_mIoUs"] = a == b
    if census:
        with C.recording(level=2) as rec:
            shared.run()
        for name, (count, ms) in rec.kernels.items():
            if name.startswith("heads_confusion"):
                by = rec.kernel_bytes.get(name, 0.0)
                row["heads_confusion"] = {"kernel": name, "launches": count, "us_per_launch": round(1e3 * ms / count, 2),
                                          "MB_per_launch": round(by / 1e6 / count, 3),
                                          "GB_per_s": round(by / 1e9 / (ms / 1e3), 1) if ms > 0 else None}
        row["census_ms_per_image"] = round(sum(ms for _, ms in rec.kernels.values()) / n, 3)
    torch.cuda.synchronize()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["bf16", "fp32", "both"], default="both")
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    net = build_supernet()
    src = source(a.images)
    rows = []
    for dt in ([torch.float32, torch.bfloat16] if a.dtype == "both" else [torch.bfloat16 if a.dtype == "bf16" else torch.float32]):
        with torch.no_grad():
            row = measure(net, src, dt, a.reps, a.warmup, not a.no_census)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
