"""The student's inference frame in the engine's three arithmetics: fp32, bf16 and fp16.

    python tools/engine_dtype_timing.py [--alternations 6] [--frames 300] [--warmup 30] [--out FILE]

One MI355X, one process.  Student (arch_1, eval build, seeded weights) at 1 x 3 x 1024 x 2048, default engine settings (every engine
tunes its own plan), graph replay with the input already in engine.input.  Engines: fp32 / bf16 / fp16 with output="logits" and bf16 /
fp16 with output="classes".

The two 16-bit engines alternate in blocks of --frames replays (bf16, fp16, bf16, fp16, ...), each block between two device events after
a synchronise, so the spread of the bf16 blocks is the run-to-run spread fp16 is judged against; the fp32 engine is timed once per
alternation beside them.  Printed: ms per frame and frames/s per block, the per-launch table of profile_in_frame() for the bf16 and
fp16 logits engines side by side (launches matched by position where the two plans issue the same entry point, else listed apart), and
every engine's error against the fp32 engine on a seeded input (max |diff|, relative to max |logit|, arg-max agreement; class maps:
share of pixels that differ)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from fasterseg_amd.devtime import block_ms  # noqa: E402

NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


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
        sys.exit("engine_dtype_timing: no GPU - nothing is measured on a CPU")
    from fasterseg_amd import archs, engine
    H, W = a.height, a.width
    shape = (1, 3, H, W)
    net = archs.build_derived(1, training=False)
    archs.init_weight(net, seed=12345)
    net = net.cuda().eval()
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11)).cuda()
    engines = {}
    with torch.no_grad():
        for output, dtypes in (("logits", (torch.float32, torch.bfloat16, torch.float16)), ("classes", (torch.bfloat16, torch.float16))):
            for dt in dtypes:
                e = engines[(output, NAMES[dt])] = engine.InferenceEngine(net, shape, dtype=dt, output=output)
                e.input.copy_(x)
    outs = {}
    for key, e in engines.items():
        for _ in range(a.warmup):
            e.run()
        torch.cuda.synchronize()
        outs[key] = e.output.clone()
    print("student arch_1 at 1 x 3 x %d x %d, graph replay, %d frames per block" % (H, W, a.frames))
    rows = {k: [] for k in engines}
    for output in ("logits", "classes"):
        print("output=%s" % output)
        print("block   bf16 ms/frame (frames/s)   fp16 ms/frame (frames/s)   fp16 / bf16" + ("   fp32 ms/frame (frames/s)" if output == "logits" else ""))
        for k in range(a.alternations):
            mb = block_ms(engines[(output, "bf16")].run, a.frames)
            mh = block_ms(engines[(output, "fp16")].run, a.frames)
            rows[(output, "bf16")].append(mb)
            rows[(output, "fp16")].append(mh)
            line = "%5d   %12.4f (%8.1f)   %12.4f (%8.1f)   %11.4f" % (k, mb, 1e3 / mb, mh, 1e3 / mh, mh / mb)
            if output == "logits":
                mf = block_ms(engines[(output, "fp32")].run, max(1, a.frames // 4))
                rows[(output, "fp32")].append(mf)
                line += "   %12.4f (%8.1f)" % (mf, 1e3 / mf)
            print(line)
        b, h = rows[(output, "bf16")], rows[(output, "fp16")]
        med = lambda v: sorted(v)[len(v) // 2]
        print("bf16 blocks: min %.4f median %.4f max %.4f ms (spread %.2f %%); fp16 blocks: min %.4f median %.4f max %.4f ms; "
              "median fp16 / median bf16 %.4f" % (min(b), med(b), max(b), 100.0 * (max(b) - min(b)) / med(b), min(h), med(h), max(h), med(h) / med(b)))
    profiles = {}
    for name in ("bf16", "fp16"):
        eng = engines[("logits", name)]
        profiles[name] = [dict(r, fn=c["fn"]) for r, c in zip(eng.profile_in_frame(), eng.calls)]
    pb, ph = profiles["bf16"], profiles["fp16"]
    print("per launch, in frame (logits engines): us bf16 | us fp16 | fp16 - bf16 | label")
    if [r["fn"] for r in pb] == [r["fn"] for r in ph]:
        for rb, rh in zip(pb, ph):
            print("%9.2f | %9.2f | %+8.2f | %-22s %s%s" % (rb["ms"] * 1e3, rh["ms"] * 1e3, (rh["ms"] - rb["ms"]) * 1e3, rb["fn"], rh["label"],
                                                        "" if rb["label"] == rh["label"] else "   (bf16 plan: %s)" % rb["label"]))
    else:
        for name, prof in (("bf16", pb), ("fp16", ph)):
            print("the two plans issue different launches; %s plan:" % name)
            for r in prof:
                print("%9.2f | %-22s %s" % (r["ms"] * 1e3, r["fn"], r["label"]))
    print("sum of the frame's launches: bf16 %.1f us, fp16 %.1f us" % (sum(r["ms"] for r in pb) * 1e3, sum(r["ms"] for r in ph) * 1e3))
    ref = outs[("logits", "fp32")].float()
    errors = {}
    for name in ("bf16", "fp16"):
        got = outs[("logits", name)].float()
        err = float((got - ref).abs().max())
        errors[name] = dict(max_abs=err, rel=err / float(ref.abs().max()), argmax_agree=float((got.argmax(1) == ref.argmax(1)).float().mean()),
                            classes_differ=float((outs[("classes", name)].long() != ref.argmax(1)).float().mean()))
        print("%s against the fp32 engine: max |diff| %.4e (%.3e of max |logit|), arg-max agreement %.6f; class-map engine: %.6f of the "
              "pixels differ from the fp32 arg-max" % (name, err, errors[name]["rel"], errors[name]["argmax_agree"], errors[name]["classes_differ"]))
    print("max |fp16 - fp32| / max |bf16 - fp32| = %.4f" % (errors["fp16"]["max_abs"] / errors["bf16"]["max_abs"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(shape=list(shape), frames=a.frames, blocks={"%s.%s" % k: v for k, v in rows.items()}, errors=errors,
                           launches={n: [dict(fn=r["fn"], label=r["label"], us=r["ms"] * 1e3) for r in p] for n, p in profiles.items()}), f)


if __name__ == "__main__":
    main()
