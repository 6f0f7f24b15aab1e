"""Per-launch table of the C2 inference plan (searched arch_1, 1x3x1024x2048) from engine.profile_in_frame(), with the tuner's logs.

    python tools/plan_table.py OUT.json [bf16|fp32]

Writes {"frame_ms", "rows": [{label, family, fn, us}], "autotuned", "cells", "folds", "heads", "capture_log"}; prints one line per launch."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from fasterseg_amd import archs, engine
    out = sys.argv[1]
    dtype = torch.float32 if (len(sys.argv) > 2 and sys.argv[2] == "fp32") else torch.bfloat16
    shape = (1, 3, 1024, 2048)
    net = archs.build_derived(1, training=False)
    archs.init_weight(net, seed=12345)
    net = net.cuda().eval()
    eng = engine.InferenceEngine(net, shape, dtype=dtype, logits_dtype=torch.float32)
    with torch.no_grad():
        eng(torch.randn(shape, generator=torch.Generator().manual_seed(0)).cuda())
    torch.cuda.synchronize()
    rows = eng.profile_in_frame()
    table = [dict(i=i, label=r["label"], family=r["family"], fn=c["fn"], us=round(r["ms"] * 1e3, 2)) for i, (r, c) in enumerate(zip(rows, eng.calls))]
    for t in table:
        print("%3d %8.2f us  %-22s %s" % (t["i"], t["us"], t["fn"], t["label"]))
    print("serial sum %.1f us, %d launches" % (sum(t["us"] for t in table), len(table)))
    with open(out, "w") as f:
        json.dump(dict(serial_us=round(sum(t["us"] for t in table), 1), rows=table, autotuned=eng.autotuned, cells=eng.cell_log,
                       folds=getattr(eng, "fold_log", []), heads=getattr(eng, "head_log", []), capture_log=getattr(eng, "capture_log", [])), f, indent=1)


if __name__ == "__main__":
    main()
