"""ms per launch and achieved GB/s of fs_render_prediction at 1024 x 2048, and SegTester's frames per second.

Launch rows (device events around `--launches` consecutive launches, after a warm-up; bytes = what the launch has to read and write,
computed here from the shapes: per panel 3 image bytes in and 3 out per pixel, 1 class byte per overlay panel, the pivots, and for the
label-ID map 1 byte in (when no overlay reads the map anyway) and 1 out):
  ids         the label-ID map alone (SegTester without show_prediction)
  ids+pred    the label-ID map and the show_prediction overlay (SegTester with show_prediction)
  show_img    image | prediction | ground truth with two 15-column pivots (SegEvaluator with show_image)
Tester rows (a host clock around run_online over `--frames` seeded frames already on the device, which ends with the last file on
disk / a device synchronise; the arch_1 student in bf16, seeded weights):
  tester      SegTester(show_prediction=True) with its PredictionWriter (PNG encoding on `--workers` host threads)
  tester-dry  the same with write=False: every frame rendered, no copy to the host, no file
Prints one JSON line per row; --out writes them all to a file."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
H, W = 1024, 2048


def tables():
    """A 19-class table drawn from a seed: the timing does not depend on the colours."""
    from fasterseg_amd.visualize import LabelSpec
    rs = np.random.RandomState(1)
    return LabelSpec(rs.randint(0, 256, size=(19, 3)).tolist(), ["class %d" % i for i in range(19)], list(range(7, 26)))


def launches(spec, n, warmup):
    from fasterseg_amd import kernels as K
    from fasterseg_amd import visualize as V
    from fasterseg_amd.devtime import block_ms
    rs = np.random.RandomState(2)
    img = torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda()
    pred = torch.from_numpy(np.kron(rs.randint(0, 19, size=(H // 32, W // 32)), np.ones((32, 32))).astype(np.uint8)).cuda()
    gt = pred.clone()
    gt[::7] = 255
    palette, lut = spec.tables("cuda")
    ids = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    one = V.padded_rows(H, W, "cuda")
    strip = V.padded_rows(H, 3 * W + 2 * V.PIVOT, "cuda")
    px = H * W
    cases = {
        "ids": (lambda: K.render_prediction(None, [pred], None, lut=lut, ids=ids), 2 * px),
        "ids+pred": (lambda: K.render_prediction(img, [pred], palette, one, gap=0, show255=[False], weights=[1], lut=lut, ids=ids), 8 * px),
        "show_img": (lambda: K.render_prediction(img, [pred, gt], palette, strip, image_panel=True, gap=V.PIVOT, show255=[False, True],
                                                 weights=[0.55, 0.55]), 20 * px + 2 * 3 * V.PIVOT * H),
    }
    rows = []
    for name, (fn, nbytes) in cases.items():
        ms = block_ms(fn, n, warm=warmup)
        rows.append({"case": name, "shape": [H, W], "launches": n, "ms_per_launch": round(ms, 4), "MB": round(nbytes / 1e6, 2),
                     "GB_per_s": round(nbytes / 1e9 / (ms / 1e3), 1)})
    return rows


def tester_rows(spec, frames, workers, slots):
    from fasterseg_amd import archs
    from fasterseg_amd.tester import SegTester
    net = archs.build_derived(1, training=False, lasts=[2, 1])
    archs.init_weight(net)
    net = net.cuda().eval()
    rs = np.random.RandomState(3)
    pool = [torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda() for _ in range(4)]
    rows = []
    for name, write in (("tester", True), ("tester-dry", False)):
        with tempfile.TemporaryDirectory() as tmp:
            t = SegTester(net, 19, MEAN, STD, spec, save_dir=tmp, show_prediction=True, slots=slots, workers=workers, write=write,
                          image_shape=(H, W))
            data = [{"data": pool[i % len(pool)], "label": None, "fn": "frame_%04d" % i} for i in range(frames)]
            t.run_online(data[:4])                                # warm-up: code objects, slots, the PNG encoder
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.run_online(data)
            dt = time.perf_counter() - t0
            t.close()
            files = len(os.listdir(tmp))
        rows.append({"case": name, "shape": [H, W], "frames": frames, "files": files, "workers": workers if write else 0, "slots": slots,
                     "frames_per_s": round(frames / dt, 2), "ms_per_frame": round(dt / frames * 1e3, 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--no-tester", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "render_timing.py measures on the GPU"
    spec = tables()
    rows = launches(spec, a.launches, a.warmup)
    for r in rows:
        print(json.dumps(r), flush=True)
    if not a.no_tester:
        more = tester_rows(spec, a.frames, a.workers, a.slots)
        for r in more:
            print(json.dumps(r), flush=True)
        rows += more
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
