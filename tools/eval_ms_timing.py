"""ms / frame of the Cityscapes multi-scale + flip evaluation protocol on one GPU (SegEvaluator.sliding_eval), and its split between
the network passes and the three post-processing kernels (fs_eval_window_input, fs_eval_score_accumulate, fs_eval_rescale_accumulate).

arch_1 with seeded weights, a seeded 1024 x 2048 uint8 image, scales (0.5, 0.75, 1, 1.25, 1.5, 1.75), flip, crop 1024, stride 5/6:
28 windows, 56 network passes per frame.  Per dtype:
  frame_ms       device events around `--frames` synchronised frames after `--warmup` frames;
  network_ms     the same number of engine passes (28 replays of the (2, 3, 1024, 1024) "lowres" engine), timed alone;
  kernels        one eager frame under the library's census (level 2: every launch of the library carries a start / stop event
                 pair), per kernel: launches, device ms and algorithmic HBM bytes -> GB/s.
  post_ms        frame_ms - network_ms (the three kernels, the canvas clears and the launch gaps between them).
For a rocprofv3 kernel table run it separately:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/eval_ms_timing.py --frames 2
Prints one JSON line per dtype; --out writes them all to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def build_net():
    from fasterseg_amd import archs
    from oracle.seeded import seeded_state
    net = archs.build_derived(1, training=False, lasts=[2, 1])
    net.load_state_dict(seeded_state(net.state_dict(), 12345))
    return net.cuda().eval()


def measure(net, img, dtype, frames, warmup, census):
    from fasterseg_amd import census as C
    from fasterseg_amd.evaluator import SegEvaluator
    ev = SegEvaluator(net, 19, MEAN, STD, image_shape=img.shape[:2], dtype=dtype, multi_scales=SCALES, is_flip=True, crop_size=1024)
    dimg = torch.from_numpy(img).cuda()
    for _ in range(warmup):
        ev.sliding_eval(dimg, 1024, 5 / 6)
    torch.cuda.synchronize()
    plans = ev._plan(ev._states[img.shape[:2]], img.shape[0], img.shape[1], 1024, 5 / 6)
    n_windows = sum(len(p.windows) for p in plans)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(frames):
        e0.record()
        ev.sliding_eval(dimg, 1024, 5 / 6)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    eng = ev._lowres_engine((2, 3, 1024, 1024))
    net_times = []
    for _ in range(frames):
        e0.record()
        for _ in range(n_windows):
            eng.run()
        e1.record()
        e1.synchronize()
        net_times.append(e0.elapsed_time(e1))
    row = {"dtype": "bf16" if dtype == torch.bfloat16 else "fp32", "scales": list(SCALES), "flip": True, "crop": 1024,
           "windows": n_windows, "passes": 2 * n_windows, "frames": frames,
           "frame_ms": float(np.median(times)), "frame_ms_min": float(np.min(times)),
           "network_ms": float(np.median(net_times))}
    row["post_ms"] = row["frame_ms"] - row["network_ms"]
    row["post_share"] = row["post_ms"] / row["frame_ms"]
    if census:
        with C.recording(level=2) as rec:
            ev.sliding_eval(dimg, 1024, 5 / 6)
        kernels = {}
        for name, (count, ms) in rec.kernels.items():
            if "eval_" in name:
                b = rec.kernel_bytes.get(name, 0.0)
                kernels[name] = {"launches": count, "ms": round(ms, 4), "GB": round(b / 1e9, 4),
                                 "GB_per_s": round(b / 1e9 / (ms / 1e3), 1) if ms > 0 else None}
        row["kernels"] = kernels
        row["kernels_ms"] = round(sum(k["ms"] for k in kernels.values()), 4)
    del ev
    torch.cuda.synchronize()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32", "both"], default="both")
    ap.add_argument("--no-census", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    img = np.random.RandomState(2024).randint(0, 256, size=(1024, 2048, 3)).astype(np.uint8)
    net = build_net()
    rows = []
    for dt in ([torch.bfloat16, torch.float32] if a.dtype == "both" else [torch.bfloat16 if a.dtype == "bf16" else torch.float32]):
        with torch.no_grad():
            row = measure(net, img, dt, a.frames, a.warmup, not a.no_census)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
