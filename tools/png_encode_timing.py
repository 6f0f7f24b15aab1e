"""fs_png_deflate at 1024 x 2048: what the two launches cost, what the files weigh, and whether PredictionWriter(device_png=True) writes
frames faster than the host encoder it replaces.

Kernel rows (three contents: one class, a smooth 19-class map, uniform byte noise): device time of one fs_png_deflate - both launches -
from devtime.captured_ms (the call copied `--copies` times into a graph, min of 3 replays) and from devtime.block_ms (`--launches`
eager calls between two events, Python included); GB/s = the map's bytes over the captured time; us_by_kernel = the two launches
apart, from the library's launch census (an event pair round each of 50 launches).
Size rows: bytes of the device's file against PIL compress_level=1 on the same map and against the raw map.  Recorded, not gated.
Frame rows (a host clock around run_online over `--frames` seeded frames already on the device, ending with the last file on disk;
arch_1 student in bf16, seeded weights, engine plan without autotune; `--workers` encoder threads, `--slots` slots): PseudoLabeler
without and with save_confidence and SegTester(show_prediction=False), each built twice, device_png False (the host path) and True,
and run in alternating blocks (`--blocks` of each kind) in this one process.  The verdict of a row pair compares the gap between the
two kinds' mean frames/s with the spread (max - min) of the blocks of one kind: "device faster" / "host faster" only beyond it.
Prints one JSON line per row; --out writes the same lines to a file."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("FS_ENGINE_AUTOTUNE", "0")

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
H, W = 1024, 2048


def contents():
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = (((np.sin(xx / 148.0) + np.cos(yy / 92.0) + np.sin((xx + yy) / 204.0)) * 3 + 9).astype(np.uint8) % 19).astype(np.uint8)
    rs = np.random.RandomState(4)
    return [("one class", np.full((H, W), 7, np.uint8)), ("smooth 19 classes", smooth), ("noise 0..255", rs.randint(0, 256, size=(H, W)).astype(np.uint8))]


def kernel_rows(copies, launches):
    from PIL import Image
    from fasterseg_amd import census
    from fasterseg_amd import kernels as K
    from fasterseg_amd.devtime import block_ms, captured_ms
    from fasterseg_amd.png import png_bytes
    rpb = K.png_rows_per_band(H, W)
    bound, ws = K.png_deflate_sizes(H, W, rpb)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = []
    for name, a in contents():
        m = torch.from_numpy(a).cuda()

        def issue(st=None):
            K.png_deflate(m, rpb, out=out, workspace=work, out_bytes=n)
        cap = captured_ms(issue, copies=copies)
        eager = block_ms(issue, launches, warm=10)
        with census.recording(2) as rec:                          # each launch between its own event pair: the two kernels apart
            for _ in range(50):
                issue()
        split = {k: round(ms / count * 1e3, 2) for k, (count, ms) in rec.kernels.items() if k.startswith("png_")}
        size = int(n.item())
        data = png_bytes(H, W, 1, out[:size].cpu().numpy())
        with Image.open(io.BytesIO(data)) as im:
            assert np.array_equal(np.asarray(im), a), name
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG", compress_level=1)
        rows.append({"case": "kernel", "content": name, "shape": [H, W], "rows_per_band": rpb, "bands": -(-H // rpb), "us_captured": round(cap * 1e3, 2),
                     "us_eager": round(eager * 1e3, 2), "us_by_kernel": split, "GB_per_s_in": round(a.size / 1e9 / (cap / 1e3), 1), "file_bytes": len(data),
                     "pil_level1_bytes": len(buf.getvalue()), "raw_bytes": int(a.size), "bound_bytes": bound})
    return rows


def frame_rows(frames, blocks, workers, slots):
    from fasterseg_amd import archs
    from fasterseg_amd.tester import PseudoLabeler, SegTester
    from fasterseg_amd.visualize import LabelSpec
    net = archs.build_derived(1, training=False, lasts=[2, 1])
    archs.init_weight(net)
    net = net.cuda().eval()
    rs = np.random.RandomState(3)
    spec = LabelSpec(rs.randint(0, 256, size=(19, 3)).tolist(), ["class %d" % i for i in range(19)], list(range(7, 26)))
    pool = [torch.from_numpy(rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)).cuda() for _ in range(4)]
    data = [{"data": pool[i % len(pool)], "label": None, "fn": "frame_%04d" % i} for i in range(frames)]
    kw = dict(slots=slots, workers=workers, image_shape=(H, W))
    makers = {
        "PseudoLabeler": lambda tmp, dp: PseudoLabeler(net, 19, MEAN, STD, tmp, min_confidence=0.5, device_png=dp, **kw),
        "PseudoLabeler(save_confidence)": lambda tmp, dp: PseudoLabeler(net, 19, MEAN, STD, tmp, min_confidence=0.5, save_confidence=True, device_png=dp, **kw),
        "SegTester(show_prediction=False)": lambda tmp, dp: SegTester(net, 19, MEAN, STD, spec, save_dir=tmp, device_png=dp, **kw),
    }
    rows = []
    for name, make in makers.items():
        with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
            dirs = {False: t0, True: t1}
            with torch.no_grad():
                runners = {dp: make(dirs[dp], dp) for dp in (False, True)}
            for dp in (False, True):
                runners[dp].run_online(data[:4])                  # warm-up: code objects, slots, the encoders
            torch.cuda.synchronize()
            fps = {False: [], True: []}
            for _ in range(blocks):
                for dp in (False, True):
                    t = time.perf_counter()
                    runners[dp].run_online(data)
                    fps[dp].append(frames / (time.perf_counter() - t))
            for dp in (False, True):
                runners[dp].close()
            sizes = {dp: sum(os.path.getsize(os.path.join(dirs[dp], f)) for f in os.listdir(dirs[dp])) / len(os.listdir(dirs[dp])) for dp in (False, True)}
        mean = {dp: sum(v) / len(v) for dp, v in fps.items()}
        spread = max(max(v) - min(v) for v in fps.values())
        gap = mean[True] - mean[False]
        verdict = "no difference beyond the spread" if abs(gap) <= spread else ("device faster" if gap > 0 else "host faster")
        rows.append({"case": "frames", "path": name, "shape": [H, W], "frames_per_block": frames, "workers": workers, "slots": slots,
                     "host_frames_per_s": [round(v, 1) for v in fps[False]], "device_frames_per_s": [round(v, 1) for v in fps[True]],
                     "host_mean": round(mean[False], 1), "device_mean": round(mean[True], 1), "spread": round(spread, 1), "verdict": verdict,
                     "host_bytes_per_file": int(sizes[False]), "device_bytes_per_file": int(sizes[True])})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=20)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--workers", type=int, default=4)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--no-frames", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "png_encode_timing.py measures on the GPU"
    rows = kernel_rows(a.copies, a.launches)
    for r in rows:
        print(json.dumps(r), flush=True)
    if not a.no_frames:
        for r in frame_rows(a.frames, a.blocks, a.workers, a.slots):
            print(json.dumps(r), flush=True)
            rows.append(r)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in rows))


if __name__ == "__main__":
    main()
