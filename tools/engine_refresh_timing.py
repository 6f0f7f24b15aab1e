"""What following a weight change costs a built InferenceEngine, one MI355X, one process: the student at 1 x 3 x 1024 x 2048, bf16.

(a) engine construction - the only way to follow a weight change before load_weights existed: seconds for a build that tunes (per-layer
    candidates, zoom-cell and fold variants, `_tune_cells`, the captures) and seconds for a build that replays the plan file the first
    one wrote (FS_ENGINE_PLAN).
(b) reload - `load_weights()` on the net the engine was built from: host clock around each call, ending in a synchronise, `--calls` calls
    after `--warmup`; the launches of one call and the refresh kernel's own device time from one census-level-2 call; the algorithmic
    bytes of the engine's refresh table (every source element read once, every destination written once).  And `load_weights(net)` with
    another module of the same architecture (adds the host-only trace and the table upload).
(c) frame - milliseconds per frame over `--frames` frames before and after a reload (device events around the loop).
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[1, 3, 1024, 2048])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from fasterseg_amd import archs, census
    from fasterseg_amd.devtime import block_ms
    from fasterseg_amd.engine import InferenceEngine
    shape = tuple(args.shape)
    nets = [archs.init_weight(archs.build_derived(1, training=False, lasts=[2, 1]), seed).cuda().eval() for seed in (12345, 999)]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).cuda()
    row = {"shape": list(shape), "dtype": "bf16", "calls": args.calls, "warmup": args.warmup, "frames": args.frames}

    # (a) construction: tuned, then replayed from the plan file the tuned build wrote
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["FS_ENGINE_PLAN"] = os.path.join(tmp, "plan.json")
        try:
            with torch.no_grad():
                for key in ("build_tuned_s", "build_plan_replay_s"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    eng = InferenceEngine(nets[0], shape, dtype=torch.bfloat16)
                    torch.cuda.synchronize()
                    row[key] = round(time.perf_counter() - t0, 3)
                assert eng._plan_in is not None, "the second build did not replay the plan"
        finally:
            del os.environ["FS_ENGINE_PLAN"]
    eng.input.copy_(x)

    # (c) frame time before the reload
    row["frame_ms_before"] = round(block_ms(eng.run, args.frames, warm=20), 4)

    # (b) reload
    t0 = time.perf_counter()
    eng.load_weights()                                  # the first call also builds the device tables
    torch.cuda.synchronize()
    row["first_reload_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    ms = host_ms(eng.load_weights, args.calls, args.warmup)
    row.update(reload_ms_median=round(statistics.median(ms), 4), reload_ms_min=round(min(ms), 4), reload_ms_max=round(max(ms), 4))
    flip = [0]

    def rebind():
        flip[0] ^= 1
        eng.load_weights(nets[flip[0]])
    ms = host_ms(rebind, args.calls, args.warmup + (args.warmup & 1))       # an even warm-up: the timed calls end on nets[0]
    if flip[0]:
        rebind()
    row.update(rebind_ms_median=round(statistics.median(ms), 4), rebind_ms_min=round(min(ms), 4))
    with census.recording(level=2) as rec:
        eng.load_weights()
    row["reload_launches"] = sum(v[0] for v in rec.kernels.values())
    row["reload_kernels"] = {k: {"launches": v[0], "us": round(v[1] * 1e3, 2)} for k, v in rec.kernels.items()}
    tab = eng._refresh_tab
    kernel_ms = sum(v[1] for k, v in rec.kernels.items() if k.startswith("refresh_weights"))
    row.update(refresh_entries=len(eng._refresh), refresh_blocks=tab["n_chunks"], refresh_MB=round(tab["bytes"] / 1e6, 3),
               refresh_kernel_us=round(kernel_ms * 1e3, 2), refresh_GB_per_s=round(tab["bytes"] / 1e9 / (kernel_ms / 1e3), 1) if kernel_ms else None)

    # (c) frame time after the reload
    row["frame_ms_after"] = round(block_ms(eng.run, args.frames, warm=20), 4)
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
