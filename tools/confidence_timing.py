"""What the confidence byte costs beside the class map, and what it saves over the logits route.

    python tools/confidence_timing.py [--alternations 6] [--frames 200] [--launches 50] [--tuned] [--out FILE]

One MI355X, one process, alternating blocks.

(a) The kernel alone, 1 x 19 x 128 x 256 (channel stride 32) -> 1024 x 2048, bf16 and fp32: fs_bilinear_argmax and
    fs_bilinear_argmax_conf, each captured --launches times back to back into one hipGraph whose replay is bracketed by two device events
    (kernel duration + one dependent-kernel boundary, no Python between launches); us per launch and GB/s on the algorithmic bytes
    (logits read once + 1 or 2 bytes per output pixel).
(b) The frame, student (arch_1, eval build) at 1 x 3 x 1024 x 2048, bf16, input already in engine.input, frames/s of
      classes              engine(output="classes").run()
      classes+confidence   engine(output="classes+confidence").run()
      logits + torch       engine(output="logits").run(), then softmax(1).max(1), the uint8 conversion of the probability and the
                           comparison with the threshold: what a user does today for the same two maps.
    The three engines are built with nothing timed (FS_ENGINE_AUTOTUNE=0, FS_ENGINE_FUSE_CELLS=1, FS_ENGINE_FOLD_RESIZE=0,
    FS_ENGINE_FUSE_HEAD=2), so they share every launch but the last; --tuned leaves the engine settings to the environment.
The condition this tool checks and prints: classes+confidence is faster than logits + torch in every alternation."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


from fasterseg_amd.devtime import block_ms, capture  # noqa: E402


def captured(fn, launches):
    g = capture(lambda st: fn(), launches)         # the kernels wrappers launch on the current stream: the capturing one
    torch.cuda.synchronize()
    return g


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--min-confidence", type=float, default=0.9)
    ap.add_argument("--tuned", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("confidence_timing: no GPU - nothing is measured on a CPU")
    if not a.tuned:
        os.environ.update(FS_ENGINE_AUTOTUNE="0", FS_ENGINE_FUSE_CELLS="1", FS_ENGINE_FOLD_RESIZE="0", FS_ENGINE_FUSE_HEAD="2")
    from fasterseg_amd import archs, engine
    from fasterseg_amd import kernels as K
    H, W = a.height, a.width
    h, w = H // 8, W // 8
    result = dict(shape=[1, 3, H, W], kernel={}, frame={})

    # ---- (a) the kernel alone ------------------------------------------------------------------------------------------------
    print("(a) kernel alone: 1 x 19 x %d x %d (stride 32) -> %d x %d; %d launches per graph, %d replays per block" % (h, w, H, W, a.launches, a.replays))
    print("dtype  block   argmax us   argmax GB/s   argmax+conf us   argmax+conf GB/s   ratio")
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        g = torch.Generator().manual_seed(5)
        x = K.empty_nhwc(1, 19, h, w, dtype, "cuda", cs=32)
        x.copy_((2 * torch.randn((1, 19, h, w), generator=g)).cuda())
        classes = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        conf = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        plain = captured(lambda: K.bilinear_argmax(x, (H, W), classes=classes), a.launches)
        both = captured(lambda: K.bilinear_argmax_conf(x, (H, W), a.min_confidence, 255, classes=classes, conf=conf), a.launches)
        in_bytes = h * w * 19 * x.element_size()
        rows = []
        for k in range(a.alternations):
            up = block_ms(plain.replay, a.replays) / a.launches * 1e3
            ub = block_ms(both.replay, a.replays) / a.launches * 1e3
            rows.append((up, ub))
            print("%-5s  %5d   %9.2f   %11.1f   %14.2f   %16.1f   %5.3f" % (name, k, up, (in_bytes + H * W) / up / 1e3, ub,
                                                                           (in_bytes + 2 * H * W) / ub / 1e3, ub / up))
        mp, mb = median([r[0] for r in rows]), median([r[1] for r in rows])
        print("%-5s median: argmax %.2f us, argmax+conf %.2f us (+%.2f us, x%.3f)" % (name, mp, mb, mb - mp, mb / mp))
        result["kernel"][name] = dict(blocks=rows, argmax_us=mp, argmax_conf_us=mb)

    # ---- (b) the frame ---------------------------------------------------------------------------------------------------------
    net = archs.build_derived(1, training=False)
    archs.init_weight(net, seed=12345)
    net = net.cuda().eval()
    with torch.no_grad():
        e_cls = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.bfloat16, output="classes")
        e_both = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.bfloat16, output="classes+confidence", min_confidence=a.min_confidence)
        e_log = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.bfloat16, output="logits")
    frame = torch.randn((1, 3, H, W), generator=torch.Generator().manual_seed(11)).cuda()
    for e in (e_cls, e_both, e_log):
        e.input.copy_(frame)
    cut = K.confidence_threshold(a.min_confidence)

    def torch_route():
        logits = e_log.run()
        p, c = torch.softmax(logits, 1).max(1)
        q = (p * 255 + 0.5).to(torch.uint8)
        return torch.where(q >= cut, c.to(torch.uint8), torch.full_like(q, 255)), q
    steps = (("classes", e_cls.run), ("classes+confidence", e_both.run), ("logits + torch", torch_route))
    for _, s in steps:
        for _ in range(a.warmup):
            s()
    torch.cuda.synchronize()
    print("(b) frame: student at 1 x 3 x %d x %d, bf16, %s plan; %d frames per block" % (H, W, "tuned" if a.tuned else "fixed", a.frames))
    print("block   classes ms (fps)      classes+confidence ms (fps)   logits + torch ms (fps)   c+c / classes   torch / c+c")
    rows = []
    for k in range(a.alternations):
        ms = [block_ms(s, a.frames) for _, s in steps]
        rows.append(ms)
        print("%5d   %8.4f (%7.1f)    %8.4f (%7.1f)            %8.4f (%7.1f)        %6.3f          %6.3f" % (
            k, ms[0], 1e3 / ms[0], ms[1], 1e3 / ms[1], ms[2], 1e3 / ms[2], ms[1] / ms[0], ms[2] / ms[1]))
    med = [median([r[i] for r in rows]) for i in range(3)]
    print("median: classes %.4f ms (%.1f fps), classes+confidence %.4f ms (%.1f fps), logits + torch %.4f ms (%.1f fps)" % (
        med[0], 1e3 / med[0], med[1], 1e3 / med[1], med[2], 1e3 / med[2]))
    print("classes+confidence costs %.1f us per frame over classes (x%.3f); the logits + torch route takes x%.2f its time" % (
        (med[1] - med[0]) * 1e3, med[1] / med[0], med[2] / med[1]))
    faster = sum(r[1] < r[2] for r in rows)
    print("condition: classes+confidence faster than logits + torch in %d of %d alternations: %s" % (
        faster, len(rows), "MET" if faster == len(rows) else "NOT MET"))
    for name, e in (("classes", e_cls), ("classes+confidence", e_both)):
        row = e.profile_in_frame()[-1]
        print("final launch in frame, %-18s: %-58s %7.2f us   %5.2f MB   %6.1f GB/s" % (
            name, row["label"], row["ms"] * 1e3, row["bytes"] / 1e6, row["bytes"] / (row["ms"] * 1e-3) / 1e9))
        result["frame"][name + " final launch us"] = row["ms"] * 1e3
    # the two routes give the same maps but for the last bits of the probability
    (c1, q1), (c2, q2) = [t.clone() for t in e_both.run()], torch_route()
    dq = (q1.int() - q2.int()).abs()
    print("engine vs torch route: confidence bytes differ at %.5f of the pixels (max %d), class maps at %.5f" % (
        float((dq > 0).float().mean()), int(dq.max()), float((c1 != c2).float().mean())))
    result["frame"].update(blocks=rows, median_ms=dict(zip([n for n, _ in steps], med)), condition_met=(faster == len(rows)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f)
    return 0 if faster == len(rows) else 1


if __name__ == "__main__":
    sys.exit(main())
