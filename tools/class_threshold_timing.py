"""What per-class thresholds cost beside one global threshold, and what the confidence histogram costs.

    python tools/class_threshold_timing.py [--alternations 6] [--launches 50] [--tuned] [--out FILE]

One MI355X, one process, alternating blocks, medians, device events.  1024 x 2048, C = 19.

(a) The final launch alone, 1 x 19 x 128 x 256 (channel stride 32) -> 1024 x 2048, bf16 and fp32: fs_bilinear_argmax_conf against
    fs_bilinear_argmax_conf_pc, each captured --launches times back to back into one hipGraph whose replay is bracketed by two device
    events; us per launch.  The same for fs_score_confidence against fs_score_confidence_pc on a (1024 x 2048, 20) fp32 score buffer.
(b) fs_confidence_hist on 1024 x 2048 maps, without labels and with uint8 labels, us per launch and GB/s on the bytes read (2 or 3 per
    pixel), on three inputs: uniform random (class, byte) keys; every pixel in one bin; the two maps of a real engine frame (student,
    arch_1, eval build, bf16, fixed plan unless --tuned; labels: the class map with a seeded 20 % altered).  Printed with it: one-bin
    time / uniform time - whether the contention handling works.
No ratio is a pass / fail condition here: the scalar launches are the yardstick, and the spread of the alternating blocks is printed
beside every median so that a gap can be told from noise."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C = 19


from fasterseg_amd.devtime import block_ms, capture  # noqa: E402


def captured(fn, launches):
    g = capture(lambda st: fn(), launches)         # the kernels wrappers launch on the current stream: the capturing one
    torch.cuda.synchronize()
    return g


def median(v):
    return sorted(v)[len(v) // 2]


def alternate(graphs, a):
    """us per launch of each captured graph over a.alternations alternating blocks: (rows, medians, (min, max) per graph)"""
    rows = [[block_ms(g.replay, a.replays) / a.launches * 1e3 for g in graphs] for _ in range(a.alternations)]
    cols = list(zip(*rows))
    return rows, [median(c) for c in cols], [(min(c), max(c)) for c in cols]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=6)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--min-confidence", type=float, default=0.9)
    ap.add_argument("--tuned", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("class_threshold_timing: no GPU - nothing is measured on a CPU")
    if not a.tuned:
        os.environ.update(FS_ENGINE_AUTOTUNE="0", FS_ENGINE_FUSE_CELLS="1", FS_ENGINE_FOLD_RESIZE="0", FS_ENGINE_FUSE_HEAD="2")
    from fasterseg_amd import archs, engine
    from fasterseg_amd import kernels as K
    H, W = a.height, a.width
    h, w = H // 8, W // 8
    cut = K.confidence_threshold(a.min_confidence)
    result = dict(shape=[1, 3, H, W], launch={}, score={}, hist={})
    # per-class thresholds around the scalar one, so that both forms mask a comparable share
    spread = np.clip(cut + np.arange(C) - C // 2, 0, 255).astype(np.uint8)
    table = K.class_threshold_table(spread, C, "cuda")

    # ---- (a) the launches alone ----------------------------------------------------------------------------------------------
    print("(a) final launch alone: 1 x %d x %d x %d (stride 32) -> %d x %d; %d launches per graph, %d replays per block" % (C, h, w, H, W, a.launches, a.replays))
    print("dtype  block   scalar us   per-class us   ratio")
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        g = torch.Generator().manual_seed(5)
        x = K.empty_nhwc(1, C, h, w, dtype, "cuda", cs=32)
        x.copy_((2 * torch.randn((1, C, h, w), generator=g)).cuda())
        classes = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        conf = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        scalar = captured(lambda: K.bilinear_argmax_conf(x, (H, W), a.min_confidence, 255, classes=classes, conf=conf), a.launches)
        pc = captured(lambda: K.bilinear_argmax_conf(x, (H, W), ignore_label=255, classes=classes, conf=conf, class_thresholds=table), a.launches)
        rows, med, rng = alternate((scalar, pc), a)
        for k, (us, up) in enumerate(rows):
            print("%-5s  %5d   %9.2f   %12.2f   %5.3f" % (name, k, us, up, up / us))
        print("%-5s median: fs_bilinear_argmax_conf %.2f us (%.2f..%.2f), fs_bilinear_argmax_conf_pc %.2f us (%.2f..%.2f): %+.2f us, x%.3f" % (
            name, med[0], rng[0][0], rng[0][1], med[1], rng[1][0], rng[1][1], med[1] - med[0], med[1] / med[0]))
        result["launch"][name] = dict(blocks=rows, scalar_us=med[0], per_class_us=med[1])
    score = torch.rand((H * W, 20), generator=torch.Generator().manual_seed(6)).cuda()
    classes = torch.empty((H * W,), dtype=torch.uint8, device="cuda")
    conf = torch.empty((H * W,), dtype=torch.uint8, device="cuda")
    scalar = captured(lambda: K.score_confidence(score, C, a.min_confidence, 255, classes=classes, conf=conf), a.launches)
    pc = captured(lambda: K.score_confidence(score, C, ignore_label=255, classes=classes, conf=conf, class_thresholds=table), a.launches)
    rows, med, rng = alternate((scalar, pc), a)
    print("score buffer (%d, 20) fp32: fs_score_confidence %.2f us (%.2f..%.2f), fs_score_confidence_pc %.2f us (%.2f..%.2f): %+.2f us, x%.3f" % (
        H * W, med[0], rng[0][0], rng[0][1], med[1], rng[1][0], rng[1][1], med[1] - med[0], med[1] / med[0]))
    result["score"] = dict(blocks=rows, scalar_us=med[0], per_class_us=med[1])

    # ---- the maps of a real engine frame, for (b) ---------------------------------------------------------------------------------
    net = archs.build_derived(1, training=False)
    archs.init_weight(net, seed=12345)
    net = net.cuda().eval()
    frame = torch.randn((1, 3, H, W), generator=torch.Generator().manual_seed(11)).cuda()
    with torch.no_grad():
        eng = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.bfloat16, output="classes+confidence")
    real_k, real_q = (t[0].clone() for t in eng(frame))

    # ---- (b) the histogram -------------------------------------------------------------------------------------------------------
    n = H * W
    gen = torch.Generator().manual_seed(7)
    uni_k = torch.randint(0, C, (n,), generator=gen).to(torch.uint8).cuda()
    uni_q = torch.randint(0, 256, (n,), generator=gen).to(torch.uint8).cuda()
    one_k = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    one_q = torch.full((n,), 255, dtype=torch.uint8, device="cuda")

    def labels(k):
        alter = (torch.rand(k.shape, generator=gen) < 0.2).to(k.device)
        return torch.where(alter, (k + 1) % C, k).contiguous()
    inputs = (("uniform", uni_k, uni_q), ("one bin", one_k, one_q), ("real frame", real_k.reshape(-1).contiguous(), real_q.reshape(-1).contiguous()))
    hist = torch.zeros((2, C, 256), dtype=torch.int64, device="cuda")
    graphs, names = [], []
    for label, k, q in inputs:
        g = labels(k)
        graphs.append(captured(lambda k=k, q=q: K.confidence_hist(k, q, C, hist=hist), a.launches))
        graphs.append(captured(lambda k=k, q=q, g=g: K.confidence_hist(k, q, C, gt=g, hist=hist), a.launches))
        names += [(label, "no labels", 2), (label, "uint8 labels", 3)]
    rows, med, rng = alternate(graphs, a)
    print("(b) fs_confidence_hist, %d pixels, C = %d; %d launches per graph, %d replays per block" % (n, C, a.launches, a.replays))
    print("input        labels          us (min..max)            GB/s")
    for (label, lab, per_px), m, r in zip(names, med, rng):
        print("%-11s  %-12s  %8.2f (%.2f..%.2f)   %7.1f" % (label, lab, m, r[0], r[1], per_px * n / m / 1e3))
        result["hist"]["%s, %s" % (label, lab)] = dict(us=m, min_us=r[0], max_us=r[1], gbps=per_px * n / m / 1e3)
    print("one bin / uniform: x%.3f without labels, x%.3f with labels; real frame / uniform: x%.3f, x%.3f; real frame: %d occupied bins" % (
        med[2] / med[0], med[3] / med[1], med[4] / med[0], med[5] / med[1],
        int((K.confidence_hist(inputs[2][1], inputs[2][2], C)[0] > 0).sum())))
    result["hist"]["one_bin_over_uniform"] = [med[2] / med[0], med[3] / med[1]]
    result["hist"]["blocks"] = rows

    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
