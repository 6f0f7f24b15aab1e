"""What a uint8 frame costs in front of the student's inference frame, and what the uint8 engine saves.

    python tools/frame_input_timing.py [--alternations 6] [--frames 300] [--warmup 30] [--out FILE]

One MI355X, one process.  Student (arch_1, eval build) at 1 x 3 x 1024 x 2048, bf16, output="classes", default engine settings.  A
uint8 (H, W, 3) frame is resident on the device; two paths turn it into a class map, both through the engine's tuned plan:

  (a) the chain in front of a float engine: SegEvaluator.process_image (permute + float, / 255, - mean, / std) and engine(x), which
      copies x into engine.input and replays;
  (b) the uint8 engine: engine(frame) copies 6 MB into engine.input, the stem normalises while it stages the image.

The paths alternate in blocks of --frames frames (a, b, a, b, ...), each block between two device events after a synchronise; ms per
frame is printed for every block.  Then profile_in_frame() gives the stem launch's in-frame device time in both engines, with GB/s
from the plan's `bytes` field, and the class maps of the two paths are compared (a figure, not a bar: torch may evaluate `/ 255.0`
as a multiplication by the reciprocal)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fasterseg_amd.devtime import block_ms  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_input_timing: no GPU - nothing is measured on a CPU")
    from fasterseg_amd import archs
    from fasterseg_amd.evaluator import SegEvaluator
    H, W = a.height, a.width
    net = archs.build_derived(1, training=False)
    archs.init_weight(net, seed=12345)
    net = net.cuda().eval()
    with torch.no_grad():
        ev_a = SegEvaluator(net, 19, MEAN, STD, image_shape=(H, W))
        ev_b = SegEvaluator(net, 19, MEAN, STD, image_shape=(H, W), uint8_input=True)
    eng_a, eng_b = ev_a.engine, ev_b.engine
    frame = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).cuda()
    step_a = lambda: eng_a(ev_a.process_image(frame))
    step_b = lambda: eng_b(frame)
    for _ in range(a.warmup):
        step_a()
        step_b()
    torch.cuda.synchronize()
    rows = []
    print("%d x %d x 3 uint8 frame on the device, bf16, output=classes; %d frames per block" % (H, W, a.frames))
    print("block   (a) process_image + engine(x) ms/frame   (b) uint8 engine(frame) ms/frame   a / b")
    for k in range(a.alternations):
        ma = block_ms(step_a, a.frames)
        mb = block_ms(step_b, a.frames)
        rows.append((ma, mb))
        print("%5d   %38.4f   %32.4f   %5.3f" % (k, ma, mb, ma / mb))
    ratios = [x / y for x, y in rows]
    print("(b) faster than (a) in %d of %d alternations; a / b min %.3f median %.3f max %.3f" % (
        sum(y < x for x, y in rows), len(rows), min(ratios), sorted(ratios)[len(ratios) // 2], max(ratios)))
    run_a = block_ms(eng_a.run, a.frames)
    run_b = block_ms(eng_b.run, a.frames)
    print("replay alone (input already in engine.input): float engine %.4f ms/frame, uint8 engine %.4f ms/frame" % (run_a, run_b))
    stems = {}
    for name, eng in (("float", eng_a), ("uint8", eng_b)):
        prof = eng.profile_in_frame()
        row = [r for r in prof if r["family"] == "stem"][0]
        stems[name] = dict(label=row["label"], us=row["ms"] * 1e3, bytes=row["bytes"], GBps=row["bytes"] / (row["ms"] * 1e-3) / 1e9,
                           frame_us=sum(r["ms"] for r in prof) * 1e3)
        print("stem in frame, %s engine: %-36s %7.2f us   %6.1f MB   %7.1f GB/s   (sum of the frame's launches %.1f us)" % (
            name, row["label"], stems[name]["us"], row["bytes"] / 1e6, stems[name]["GBps"], stems[name]["frame_us"]))
    ca, cb = step_a()[0].clone(), step_b()[0].clone()
    differ = float((ca != cb).float().mean())
    print("class maps of the two paths: %.6f of the pixels differ" % differ)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=[1, 3, H, W], frames=a.frames, blocks=[dict(a_ms=x, b_ms=y) for x, y in rows], replay_ms=dict(float=run_a, uint8=run_b),
                           stem=stems, class_map_differ=differ), f)


if __name__ == "__main__":
    main()
