"""bench.py — headline benchmark of the FasterSeg hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dtype bf16|fp32] [--dump-outputs DIR]
    python bench.py --full [--train-dtype fp32|bf16] [--workloads c2,c3,c4,c5] ...

ONE JSON line on rank 0.  Top level = BASELINE.json configs[1] (C2): searched student (arch_1) inference at 1x3x1024x2048,
frames/s, input resident in HBM, the whole forward replayed from one hipGraph (fasterseg_amd.engine).  A plain run does only
that: it builds the engine, warms up, times exactly K steps (`ms_per_step` = one step), writes the last step's logits (a fixed
seeded sample of pixels) with --dump-outputs and prints the line.  Everything else runs with --full:

With --full, before anything is timed the engine's logits are checked against the CPU oracle on the same weights and input (bf16:
relative error <= 5e-2 and arg-max agreement >= 97 %; fp32: <= 1e-3) — a frame rate of a wrong answer is never printed — and
`workloads` carries every BASELINE configuration with its own ms_per_step, images/s, `roofline` and `cpu_baseline`:
  C2_student_infer      the top-level numbers again
  C3_supernet_pretrain  `_loss(pretrain=True)`: max / min / random / random width passes, backward, clip, SGD; 3 x 3x256x512
  C4_student_train      teacher eval forward + student train forward/backward (3 heads, OHEM-CE + KL), SGD; 12 x 3x512x1024
  C5_supernet_search    Architect.step (arch0, arch1 Gumbel, max, min + latency loss, Adam) + weight step; 2 x 3x224x448,
                        latency table = the shipped MI355X table rebuilt from HIP-kernel timings
The train steps are restated in fasterseg_amd/train_step.py from search/train_search.py:215-251 and train/train.py:219-271.
With N > 1 (one rank per GPU, RCCL) inference runs as independent replicas (it does not shard: no data-path collective,
"weak") and the three train steps run data-parallel with the flat-gradient all-reduce, so every --gpus N run exercises the
collective path; launched without torchrun, `--gpus N` starts itself under torch.distributed.run as a child process.

Every train workload is gated like C2: the loss of the FIRST step of the stepper that is about to be timed is compared with the CPU
oracle on the same weights / batch / RNG seeds (`parity` inside each workload; a miss aborts).  A train workload's `value` / `dtype` are
the fp32 step's (fp32 storage + exact-fp32 MFMA: the reference trains in fp32, and only this step's gradients are the reference's
within its own fp32-vs-fp64 gap); the all-bf16 step is timed beside it as a labelled throughput mode (`value_bf16`, `ms_per_step_bf16`).
roofline: one more frame / step issued eagerly with every kernel launch timed by its own start/stop HIP event pair on the launch
stream (hipExtLaunchKernelGGL; fasterseg_amd/census.py, csrc/census.hip): achieved = algorithmic FLOPs of ALL launches of the dominant
kernel family / the sum of their measured durations - the figures tools/roofline_from_profile.py recomputes from the rocprofv3
tables under profiles/.  cpu_baseline: the CPU oracle (oracle/, fixture-pinned port of the
reference modules on torch-CPU kernels) on a bounded sample of the same workload, on this host's cores.
Without an explicit --steps, a step count whose timed region would be shorter than --min-seconds is raised (reported as `steps`;
`steps_requested` keeps the flag); an explicit --steps K is timed as exactly K steps.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}      # dense MFMA peaks, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0
# arithmetic of the committed PMC traffic tables (profiles/r06_<workload>_pmc.json; tools/prof_round.sh): `roofline.traffic` of a train
# step is quoted only for the leg that matches (the fp32 pass of C4 crashed rocprofv3 itself: its table is the bf16 step's, as in round 5)
PMC_TABLE_DTYPE = {"c3": "fp32", "c5": "fp32", "c4": "bf16"}
PUBLISHED_STUDENT_FPS = 163.9                        # BASELINE.md §1 (GTX 1080Ti + TensorRT fp32, latency/ variant)
METRIC = "supernet train-step images/sec @1024x2048 (1/2/4/8 GPU) + student fps"
PRECISION = {"bf16": "bf16 activations + bf16 MFMA, fp32 accumulate / BN statistics / master weights / parameter gradients",
             "fp32": "fp32 storage, exact-fp32 MFMA"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed C2 frames (default 2000); train workloads time 10 steps")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default 100 frames / 3 train steps)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="C2 (the headline): BASELINE configs[1] names bf16")
    ap.add_argument("--train-dtype", default="fp32", choices=["bf16", "fp32"],
                    help="precision of each train workload's `value` (C3/C4/C5): fp32 = the reference's arithmetic (default); the other "
                         "precision is timed as a labelled extra")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: the CPU-oracle parity gates, the train workloads (C3/C4/C5), roofline censuses, "
                         "the other-precision legs, the class-map engine, CPU baselines, device clocks.  Without it a run builds the C2 "
                         "engine, warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last C2 step computed to DIR/*.npy (float32; a fixed seeded sample of "
                         "the logits' pixels, all classes)")
    ap.add_argument("--workloads", default=None, help="comma list of c2,c3,c4,c5 (c2 is always the headline; default c2, with --full all four)")
    ap.add_argument("--train-steps", type=int, default=None, help="timed steps of every train workload (default 10; with an explicit --steps K: K bounded to 10..50)")
    ap.add_argument("--train-warmup", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5, help="minimum length of every timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-fp32-leg", "--no-other-leg", dest="no_fp32_leg", action="store_true",
                    help="skip the other-precision re-run of every train workload (and the fp32 engine of C2)")
    ap.add_argument("--no-class-map", action="store_true", help="skip the class-map (evaluator) variant of the C2 engine")
    ap.add_argument("--cpu-seconds", type=float, default=25.0, help="CPU budget of each cpu_baseline sample")
    ap.add_argument("--dump-plan", default=None, help="write the per-launch table of the C2 plan (json) here")
    ap.add_argument("--detail", default=None,
                    help="everything that is not in the (small) JSON line goes here: autotune logs, per-kernel tables, clocks, method strings "
                         "(default with --full: bench_detail.json; otherwise only written when given)")
    ap.add_argument("--regions", type=int, default=1, help="with an explicit --steps: timed regions of EXACTLY that many steps; the median is reported")
    args = ap.parse_args()
    if args.workloads is None:
        args.workloads = "c2,c3,c4,c5" if args.full else "c2"
    if args.detail is None and args.full:
        args.detail = os.path.join(ROOT, "bench_detail.json")
    args.steps_requested = args.steps
    args.exact = args.steps is not None                # an explicit --steps K is timed as exactly K steps (never raised)
    if args.steps is None:
        args.steps = 2000
    if args.warmup is None:
        args.warmup = 100
    if args.train_steps is None:                       # the train workloads follow --steps too, bounded so a huge K stays minutes
        args.train_steps = max(10, min(args.steps, 50)) if args.exact else 10
    args.workloads = [w.strip().lower() for w in args.workloads.split(",") if w.strip()]
    if not args.full and any(w != "c2" for w in args.workloads):
        raise SystemExit("bench.py: the train workloads (c3, c4, c5) run with --full")
    return args


# ---- distributed plumbing ----------------------------------------------------------------------------------------------
def dist_setup(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1 and args.gpus > 1:
        # not under torchrun: start one rank per GPU ourselves (the driver's own launch line, contract in the task statement)
        have = torch.cuda.device_count()
        if have < args.gpus and os.environ.get("FS_DIST_BACKEND", "nccl") == "nccl":
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible (RCCL needs one device per rank)" % (args.gpus, have))
        import socket
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr",
               "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        # a child process, not exec: this process has already initialised the GPU (device_count above), and replacing a process
        # that holds the device open is not safe
        import subprocess
        rc = subprocess.run(cmd).returncode
        raise SystemExit(rc if rc >= 0 else 128 - rc)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py: WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    backend = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        torch.cuda.set_device(local % torch.cuda.device_count())
        # backend "nccl" is RCCL on ROCm; FS_DIST_BACKEND=gloo exists only to exercise this path with several ranks on
        # a single-GPU box (RCCL refuses two ranks on one device)
        dist.init_process_group(os.environ.get("FS_DIST_BACKEND", "nccl"), rank=rank, world_size=world)
        backend = dist.get_backend()
    else:
        torch.cuda.set_device(0)
    return world, rank, backend


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        t = torch.zeros(1, device="cuda")
        dist.all_reduce(t)
    torch.cuda.synchronize()


def max_over_ranks(value, world):
    if world == 1:
        return value
    import torch.distributed as dist
    t = torch.tensor([value], dtype=torch.float64, device="cuda")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def timed_region(run, steps, warmup, world, min_seconds, exact=False, regions=1):
    """warm-up, then EXACTLY `steps` calls of run() between barrier+synchronize pairs; max over ranks.  Without an explicit --steps
    (`exact` False) `steps` is first raised (from the warm-up's own rate) until the region is at least min_seconds long.  With
    `exact`, `regions` such regions of exactly `steps` calls are timed and the median region is returned."""
    barrier(world)
    t0 = time.perf_counter()
    for _ in range(max(warmup, 1)):
        run()
    barrier(world)
    per = max_over_ranks((time.perf_counter() - t0) / max(warmup, 1), world)
    if not exact:
        steps = max(steps, int(math.ceil(min_seconds / max(per, 1e-7))))
        regions = 1
    times = []
    for _ in range(max(regions, 1)):
        barrier(world)
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        barrier(world)
        times.append(max_over_ranks(time.perf_counter() - t0, world))
    times.sort()
    return times[len(times) // 2], steps


def parallelism(world, backend, what):
    if world == 1:
        return "single GPU"
    return "dp%d, %s, torch.distributed backend '%s'%s" % (world, what, backend, " (= RCCL)" if backend == "nccl" else " (functional test only)")


# ---- measured HBM traffic (rocprofv3 --pmc passes of earlier runs, committed under profiles/) ----------------------------------------
def frame_traffic(family, dtype):
    """HBM bytes per launch of a kernel family of the C2 frame: profiles/r03_c2_pmc_frame.json (tools/pmc_frame.py: FETCH_SIZE / WRITE_SIZE
    passes over plan-order frames, conv3x3 and conv1x1 separately), else the round-2 table; None when there is no measurement."""
    for name, get in (("r06_c2_pmc_frame.json", lambda d: d.get(family, {}).get("hbm_bytes_per_launch")),
                      ("r05_c2_pmc_frame.json", lambda d: d.get(family, {}).get("hbm_bytes_per_launch")),
                      ("r04_c2_pmc_frame.json", lambda d: d.get(family, {}).get("hbm_bytes_per_launch")),
                      ("r03_c2_pmc_frame.json", lambda d: d.get(family, {}).get("hbm_bytes_per_launch")),
                      ("pmc_traffic.json", lambda d: d.get(dtype, {}).get(family))):
        path = os.path.join(ROOT, "profiles", name)
        if dtype == "bf16" and os.path.exists(path):
            try:
                with open(path) as f:
                    v = get(json.load(f))
                if v:
                    return int(v)
            except Exception:
                pass
    return None


def step_traffic(workload, kernels, launched=None):
    """HBM bytes per launch of the given kernels of a train step from profiles/r0N_<workload>_pmc.json (tools/pmc_table.py: separate
    FETCH_SIZE / WRITE_SIZE passes), or None - also when the committed PMC table does not cover the kernels the step launches NOW
    (`launched`: name -> {"launches"} of the census step; a table taken with an older kernel would be a stale figure)."""
    for rnd in ("r06", "r05", "r04", "r03"):
        path = os.path.join(ROOT, "profiles", "%s_%s_pmc.json" % (rnd, workload))
        if os.path.exists(path):
            break
    else:
        return None
    try:
        with open(path) as f:
            d = json.load(f)
        if launched:
            ran = sum(v["launches"] for k, v in launched.items() if k in kernels)
            covered = sum(v["launches"] for k, v in launched.items() if k in kernels and k in d)
            if ran and covered < 0.9 * ran:
                return None
        per = lambda k: d[k].get("hbm_read_bytes_per_launch", 0) + d[k].get("hbm_write_bytes_per_launch", 0)
        if launched:      # the table's per-launch bytes of every kernel, weighted by what THIS step launches (the PMC pass is an all-eager
            n = sum(v["launches"] for k, v in launched.items() if k in kernels and k in d)      # step: more grouped launches than a timed one)
            b = sum(v["launches"] * per(k) for k, v in launched.items() if k in kernels and k in d)
        else:
            n = sum(d[k]["launches"] for k in kernels if k in d)
            b = sum(d[k]["launches"] * per(k) for k in kernels if k in d)
        return int(b / n) if n else None
    except Exception:
        return None


STEP_FAMILY_KERNELS = {"conv_igemm (fwd + dgrad)": ("conv_igemm_kernel", "conv_igemm2_kernel", "conv_igemm2_group_kernel", "splitk_reduce_kernel"),
                       "conv_wgrad": ("wgrad_kernel", "wgrad_group_kernel"),
                       "conv3x3_halo": ("conv3x3_halo_kernel",)}


# ---- C2: student inference ---------------------------------------------------------------------------------------------
def roofline_from_profile(rows, dtype):
    fam = {}
    for r in rows:
        f = fam.setdefault(r["family"], dict(ms=0.0, flops=0.0, bytes=0.0, n=0))
        f["ms"] += r["ms"]; f["flops"] += r["flops"]; f["bytes"] += r["bytes"]; f["n"] += 1
    total_ms = sum(f["ms"] for f in fam.values())
    name, dom = max(fam.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = dom["ms"] / dom["n"]
    out = {"kernel": name, "launches_per_step": dom["n"], "avg_launch_us": round(avg_ms * 1e3, 3),
           "share_of_kernel_time": round(dom["ms"] / total_ms, 4), "traffic": None}
    if dom["flops"] > 0:
        ach = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
        out.update(bound="mfma", achieved=round(ach, 2), peak=PEAK_TFLOPS[dtype], unit="TFLOP/s", frac=round(ach / PEAK_TFLOPS[dtype], 4),
                   alg_flops_per_launch=dom["flops"] / dom["n"], alg_bytes_per_launch=dom["bytes"] / dom["n"],
                   achieved_GBps=round(dom["bytes"] / (dom["ms"] * 1e-3) / 1e9, 1))
    else:
        ach = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9
        out.update(bound="hbm", achieved=round(ach, 1), peak=PEAK_HBM_GBS, unit="GB/s", frac=round(ach / PEAK_HBM_GBS, 4),
                   alg_bytes_per_launch=dom["bytes"] / dom["n"])
    out["traffic"] = frame_traffic(name, dtype)
    families = {k: {"ms": round(v["ms"], 4), "launches": v["n"], "TFLOPs": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["flops"] else 0.0,
                    "GBps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1)} for k, v in fam.items()}
    return out, families, total_ms


DUMP_SEED = 20240601
DUMP_PIXEL_FRACTION = 4                              # one pixel in four: 19 classes x 524288 pixels x 4 B = 40 MB of the 159 MB logits


def dump_outputs(directory, logits):
    """What the timed C2 step hands its caller - the fp32 logits (N, C, H, W) - as DIR/logits_sample.npy: every class at a fixed,
    seeded set of pixels (ascending flat index; the same set on every run), shape (N, C, pixels), float32.  Called after the timed
    region, which ends with a device synchronize."""
    import numpy as np
    n, c, h, w = logits.shape
    g = torch.Generator().manual_seed(DUMP_SEED)
    idx = torch.randperm(h * w, generator=g)[:h * w // DUMP_PIXEL_FRACTION].sort().values
    sample = logits.reshape(n, c, h * w).index_select(2, idx.to(logits.device)).float().cpu().numpy()
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "logits_sample.npy"), sample)


def run_student_infer(args, world, rank, backend):
    from fasterseg_amd import archs, engine
    from oracle import ref_ops
    from oracle.seeded import resolve_aliases
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    shape = (1, 3, 1024, 2048)
    net = archs.build_derived(1, training=False)          # eval build, branches chosen by objective_acc_lat -> [2, 1]
    archs.init_weight(net, seed=12345)
    if args.full:
        with open(os.path.join(ROOT, "tests", "golden", "arch_1.json")) as f:
            meta = json.load(f)["eval_21"]                # decoded structure of arch_1 (test fixture): only the oracle reads it
        params = resolve_aliases({k: v.detach().clone() for k, v in net.state_dict().items()}, meta)
    net = net.cuda().eval()
    eng = engine.InferenceEngine(net, shape, dtype=dtype, logits_dtype=torch.float32)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(rank))
    parity = None
    if args.full:
        # ---- parity gate: the engine that is about to be timed vs the CPU oracle, same weights, same frame
        cores = torch.get_num_threads()
        with torch.no_grad():
            t0 = time.perf_counter()
            want = ref_ops.derived_forward(params, meta, x)
            oracle_s = time.perf_counter() - t0
            got = eng(x.cuda()).float().cpu()
        err = float((got - want).abs().max())
        rel = err / float(want.abs().max())
        agree = float((got.argmax(1) == want.argmax(1)).float().mean())
        ok = (err <= 1e-3) if args.dtype == "fp32" else (rel <= 5e-2 and agree >= 0.97)
        parity = {"vs": "oracle.ref_ops.derived_forward (CPU fp32), same weights and frame", "max_abs_err": err, "rel_to_max_logit": rel,
                  "argmax_agreement": agree, "bar": "fp32: max_abs_err <= 1e-3; bf16: rel <= 5e-2 and argmax >= 0.97", "pass": bool(ok)}
        if not ok:
            raise SystemExit("bench.py: engine logits do not match the CPU oracle: %s" % json.dumps(parity))
    else:
        with torch.no_grad():
            eng(x.cuda())                                 # the frame every timed step replays
    elapsed, steps = timed_region(eng.run, args.steps, args.warmup, world, args.min_seconds, args.exact, args.regions)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, eng.output)
    fps = world * steps / elapsed
    line = {
        "value": round(fps, 2), "unit": "frames/s", "steps": steps, "warmup": args.warmup, "ms_per_step": round(elapsed / steps * 1e3, 4),
        "dtype": args.dtype, "precision": PRECISION[args.dtype] + "; fp32 logits",
        "config": {"workload": "C2 student fps (BASELINE configs[1]): searched arch_1 (eval build, branches 1/32+1/16) inference 1x3x1024x2048, "
                               "19 classes, fp32 logits at input resolution",
                   "weights": "random kaiming init, seed 12345",
                   "parallelism": "replicas x%d (inference does not shard: no collective)" % world,
                   "engine": "static plan of %d launches in one hipGraph (%d stream lanes; %d zoomed / 2x cells as one fused launch each of "
                             "%d candidates; %d duplicate resamples shared, %d folded into 1x1 convs; instantiations timed at build, "
                             "ms/frame: %s)" % (len(eng.calls), getattr(eng, "graph_lanes", 1),
                                                sum(1 for c in eng.calls if c["fn"] == "fs_zoom_cell_fwd"), eng.fused_cells,
                                                eng.shared_resizes, eng.fused_resizes, getattr(eng, "capture_log", [])),
                   "conv_autotune": "3x3 s1 layers [label, pixels, cin, cout, chosen, candidates us]: %s" % (eng.autotuned,),
                   "cells": "[label, choice, fused us, split us (alone, cache-warm), frame ms with the choice flipped]: %s" % (eng.cell_log,)},
        "parity": parity,
        "alg_gflop_per_frame": round(eng.total_flops / 1e9, 3), "alg_mb_per_frame": round(eng.total_bytes / 1e6, 1),
        "vs_baseline": round(fps / world / PUBLISHED_STUDENT_FPS, 3),
        "vs_baseline_note": "per-GPU fps / 163.9 FPS published on GTX 1080Ti + TensorRT fp32 (nearest-resample latency/ variant of "
                            "the network); this run is the bilinear train/ network",
    }
    if rank == 0 and args.full and not args.no_roofline:
        # in-frame: every launch of the plan timed by its own HIP event pair while whole frames are issued in plan order (what
        # rocprofv3's kernel trace of a frame shows); isolated: each launch replayed 20x alone, cache-warm (the round-1/2 figure)
        rows = eng.profile_in_frame()
        roof, families, total_ms = roofline_from_profile(rows, args.dtype)
        iso_roof, iso_fam, iso_ms = roofline_from_profile(eng.profile(), args.dtype)
        roof["method"] = ("in-frame: 20 frames issued launch by launch in plan order on one stream, every kernel timed by its own start/stop "
                          "HIP event pair (hipExtLaunchKernelGGL); achieved = sum alg FLOPs / sum durations of the family's launches")
        roof["isolated"] = {"achieved": iso_fam[roof["kernel"]]["TFLOPs"], "frac": round(iso_fam[roof["kernel"]]["TFLOPs"] / PEAK_TFLOPS[args.dtype], 4),
                            "note": "each launch replayed 20x back to back from its own hipGraph (operands L2-warm): upper bound, not the in-frame rate"}
        line["roofline"] = roof
        line["kernel_families"] = families
        line["kernel_families_isolated"] = iso_fam
        line["sum_kernel_ms"] = round(total_ms, 4)
        flops_roof = eng.total_flops / (PEAK_TFLOPS[args.dtype] * 1e12)
        bytes_roof = eng.total_bytes / (PEAK_HBM_GBS * 1e9)
        line["frame_roofline"] = {"ideal_ms": round(max(flops_roof, bytes_roof) * 1e3, 4), "frac": round(max(flops_roof, bytes_roof) / (elapsed / steps), 4),
                                  "note": "max(alg FLOPs / MFMA peak, alg bytes / 8 TB/s) / measured frame time"}
        if args.dump_plan:
            with open(args.dump_plan, "w") as f:
                json.dump(rows, f, indent=1)
    if rank == 0 and args.full and args.dtype == "bf16" and not args.no_fp32_leg:
        # north_star's bar in ONE record: ">= 163 fps with logits within 1e-3 of the reference" is an fp32 statement (the published
        # 163.9 FPS is TensorRT fp32, latency/run_latency.py:81) - the same engine in fp32 storage + exact-fp32 MFMA, gated and timed
        torch.cuda.empty_cache()
        eng32 = engine.InferenceEngine(net, shape, dtype=torch.float32, logits_dtype=torch.float32)
        with torch.no_grad():
            got32 = eng32(x.cuda()).float().cpu()
        err32 = float((got32 - want).abs().max())
        if not err32 <= 1e-3:
            raise SystemExit("bench.py: fp32 engine logits differ from the CPU oracle by %.3e (> 1e-3)" % err32)
        el32, steps32 = timed_region(eng32.run, args.steps, args.warmup, 1, args.min_seconds, args.exact, args.regions)
        line["fp32"] = {"value": round(steps32 / el32, 2), "unit": "frames/s", "ms_per_step": round(el32 / steps32 * 1e3, 4), "steps": steps32,
                        "max_abs_err": err32, "argmax_agreement": float((got32.argmax(1) == want.argmax(1)).float().mean()),
                        "vs_baseline": round(steps32 / el32 / PUBLISHED_STUDENT_FPS, 3), "launches": len(eng32.calls),
                        "note": PRECISION["fp32"] + "; logits vs oracle.ref_ops.derived_forward on the same weights and frame, bar 1e-3"}
        del eng32, got32
        torch.cuda.empty_cache()
    if rank == 0 and args.full and not args.no_class_map:
        # the evaluator path: same network, class map (uint8) instead of fp32 logits as the output
        eng_c = engine.InferenceEngine(net, shape, dtype=dtype, output="classes")
        cls = eng_c(x.cuda())
        same = float((cls.cpu() == got.argmax(1).to(torch.uint8)).float().mean())
        el_c, steps_c = timed_region(eng_c.run, args.steps, args.warmup, 1, args.min_seconds, args.exact, args.regions)
        line["class_map"] = {"value": round(steps_c / el_c, 2), "unit": "frames/s", "ms_per_step": round(el_c / steps_c * 1e3, 4), "steps": steps_c,
                             "launches": len(eng_c.calls), "agreement_with_argmax_of_logits": same,
                             "note": "validation frames: the x8 up-sample and the evaluator's arg-max (tools/engine/evaluator.py:223) in one "
                                     "launch, 2 MB uint8 out instead of 159 MB fp32 logits"}
        del eng_c
    if rank == 0 and args.full and world == 1 and not args.no_cpu_baseline:
        def cpu_frame():
            with torch.no_grad():
                ref_ops.derived_forward(params, meta, x)
        line["cpu_baseline"] = _time_cpu(cpu_frame, 1, args.cpu_seconds,
                                         "frames of 1x3x1024x2048 fp32 through oracle/ref_ops.derived_forward (port of train/model_seg.py on "
                                         "torch-CPU kernels, fixture-pinned); first (cold, %d threads) frame %.2f s" % (cores, oracle_s),
                                         unit="frames/s")
    return line


# ---- train workloads ---------------------------------------------------------------------------------------------------
def _train_line(args, world, backend, name, batch, elapsed, steps, warmup, extra):
    ips = world * batch * steps / elapsed
    line = {"value": round(ips, 4), "unit": "images/s", "steps": steps, "warmup": warmup, "ms_per_step": round(elapsed / steps * 1e3, 3),
            "dtype": args.dtype, "precision": PRECISION[args.dtype], "per_gpu_batch": batch, "global_batch": world * batch,
            "config": {"workload": name, "parallelism": parallelism(world, backend, "flat fp32 gradient buckets all-reduced before clip / SGD")},
            "gradient_fidelity": GRADIENT_FIDELITY[args.dtype]}
    line.update(extra)
    return line


# what tests/test_train_parity_gpu.py measures for the step objects below against the reference's fp64 run (fixtures at the
# benchmarked depth / map size; tiny-batch BatchNorm amplifies a rounding of 1e-7 to 1e-2 in deep-layer gradients)
GRADIENT_FIDELITY = {
    "fp32": "loss exact to 7 digits; per-tensor gradient relative L2 <= 2e-2 vs the reference's fp64 run (= the reference's own fp32-vs-fp64 gap)",
    "bf16": "loss within 1e-3 of the reference's fp64 run, same parameters receive gradients; gradients next to the heads cosine >= 0.99, deep "
            "layers 0.5-0.9 (bf16 storage rounding x the ~1e5 amplification of tiny-batch BatchNorm): throughput mode - the fp32 leg "
            "(ms_per_step_fp32) is the reference's arithmetic"}
PARITY_BARS = {"bf16": 1e-2, "fp32": 2e-3}      # relative error of the first step's loss vs the CPU oracle (tests/test_train_parity_gpu.py)


def _parity(what, got, want, dtype_name, extra=None):
    rel = abs(got - want) / max(abs(want), 1e-12)
    out = {"vs": what, "loss": got, "oracle_loss": want, "rel_err": rel, "bar": "rel_err <= %g (%s)" % (PARITY_BARS[dtype_name], dtype_name),
           "pass": bool(rel <= PARITY_BARS[dtype_name])}
    if extra:
        out.update(extra)
    if not out["pass"]:
        raise SystemExit("bench.py: train-step loss does not match the CPU oracle: %s" % json.dumps(out))
    return out


def _timed_census(args, world, rank, step_fn, extra_entries=(), workload=None):
    """ONE more step, issued eagerly with every kernel launch timed by its own HIP event pair (census level 2).  Every rank runs it
    (the step contains the gradient all-reduce), rank 0 reports."""
    from fasterseg_amd import census
    with census.recording(level=2) as rec:
        step_fn()
        torch.cuda.synchronize()
    if rank != 0:
        return None
    roof, families, kernels = census.roofline_timed(rec, args.dtype, PEAK_TFLOPS[args.dtype], PEAK_HBM_GBS, extra_entries)
    if roof is not None and workload and args.dtype == PMC_TABLE_DTYPE.get(workload, "bf16"):
        roof["traffic"] = step_traffic(workload, STEP_FAMILY_KERNELS.get(roof["kernel"], ()), kernels)
    if roof is not None and roof.get("bound") == "mfma" and args.dtype == "fp32":
        # (detail file only) what `peak` is: the fp32 MFMA's dense peak.  Since round 6 the fp32 convolutions contract on the bf16 matrix
        # cores with exactly split operands - 8 bf16 MFMAs per 16 values of K, i.e. a ceiling of 2500 / 8 = 312.5 TFLOP/s of fp32 work
        roof["peak_note"] = "157.3 = dense fp32 MFMA peak; the split form's ceiling is 2500 / 8 = 312.5 TFLOP/s: frac %.4f of that" % (
            roof["achieved"] / 312.5)
    out = {"roofline": roof, "kernel_families": families, "kernels_in_step": kernels}
    if roof is not None and roof.get("step_ideal_ms"):
        # the whole step against the roofs (the analogue of C2's frame_roofline): every family at its own roof - convolutions at the dense
        # MFMA peak of the step's dtype, BatchNorm / resample / weighted-sum passes at 8 TB/s - over the measured step; `frac` is filled in by
        # the caller, who knows ms_per_step of the timed region
        out["step_roofline"] = {"ideal_ms": roof["step_ideal_ms"], "launches": sum(k["launches"] for k in kernels.values()),
                                "kernel_ms": round(sum(k["ms_per_step"] for k in kernels.values()), 3)}
    return out


def _close_step_roofline(line):
    sr = line.get("step_roofline")
    if sr and line.get("ms_per_step"):
        sr["frac"] = round(sr["ideal_ms"] / line["ms_per_step"], 5)
        sr["note"] = "sum over families of algorithmic work / roof (convs: dense MFMA peak of the dtype; BN, resample, weighted sums: 8 TB/s) / ms_per_step"


def _other_leg(args, world, make_stepper, run_of, batch):
    """The same step in the OTHER precision.  Round 6: a train workload's `value` is the fp32 step - fp32 storage,
    exact-fp32 MFMA: the reference's arithmetic (search/train_search.py:215-251, train/train.py:219-271), gradients within the
    reference's own fp32-vs-fp64 gap - and the all-bf16 step is this labelled extra (`*_bf16`: loss right to 1e-3, deep-layer
    gradients cosine 0.4-0.6, a throughput mode).  With --train-dtype bf16 the roles swap (`*_fp32`), as rounds 2-5 printed them."""
    if args.no_fp32_leg:
        return {}
    other = "bf16" if args.dtype == "fp32" else "fp32"
    torch.cuda.empty_cache()
    stepper = make_stepper(torch.float32 if other == "fp32" else torch.bfloat16)
    run = run_of(stepper)
    elapsed, steps = timed_region(run, max(10, args.train_steps), 2, world, args.min_seconds, args.exact, min(args.regions, 3))
    del stepper
    torch.cuda.empty_cache()
    note = (PRECISION["fp32"] + " - the reference trains in fp32 (search/train_search.py:215-251, train/train.py:219-271)") if other == "fp32" else \
           (PRECISION["bf16"] + " - throughput mode, NOT the reference's computation: " + GRADIENT_FIDELITY["bf16"])
    return {"ms_per_step_" + other: round(elapsed / steps * 1e3, 3), "value_" + other: round(world * batch * steps / elapsed, 4),
            other + "_steps": steps, other + "_note": note}


def run_student_train(args, world, rank, backend):
    from fasterseg_amd import train_step
    from oracle import ref_loss, ref_ops
    from oracle.seeded import resolve_aliases
    batch, H, W = 12, 512, 1024
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    make = lambda d: train_step.StudentDistillStep(batch, H, W, teacher_engine_dtype=d, compute_dtype=d)
    stepper = make(dt)
    imgs, target = train_step.synthetic_batch(batch, H, W, rank, "cuda")
    with open(os.path.join(ROOT, "tests", "golden", "arch_1.json")) as f:      # decoded structures (test fixtures): only the oracle reads them
        meta_s = json.load(f)["train_21"]
    with open(os.path.join(ROOT, "tests", "golden", "arch_0.json")) as f:
        meta_t = json.load(f)["train_21"]
    snap = lambda net, meta: resolve_aliases({k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, meta)
    ps, pt = snap(stepper.student, meta_s), snap(stepper.teacher, meta_t)          # the weights the first step sees
    # ---- parity gate: the FIRST step's loss (the stepper that is about to be timed, teacher engine included) vs the CPU oracle on a
    # slice of the same batch with the same weights.  OHEM's min_kept is per batch (train/train.py:62), so the device side evaluates
    # the same slice through the same modules and criteria (eager teacher) - and the full-batch first step must agree with it too.
    # (loss_only BEFORE the first step: the oracle gets the weights of step 0, and one SGD step of lr 0.01 already moves this loss by
    # 0.5 % - within the bf16 bar of rounds 3-5, five times the fp32 bar the gate has had since round 6)
    nb = 2
    got = stepper.loss_only(imgs[:nb], target[:nb]) if rank == 0 else None
    first = float(stepper.step(imgs, target))
    parity = None
    if rank == 0:
        xi, ti = imgs[:nb], target[:nb]
        with torch.no_grad():
            t_logits = ref_ops.derived_forward(pt, meta_t, xi.cpu(), training=False)
            p8, p16, p32 = ref_ops.derived_forward(dict(ps), meta_s, xi.cpu(), training=True)
            want = float(ref_loss.student_step_loss(p8, p16, p32, t_logits, ti.cpu(), min_kept=nb * H * W // 16))
        parity = _parity("oracle.ref_ops.derived_forward (teacher eval + student train mode) + oracle.ref_loss.student_step_loss on %d images of the "
                         "batch, weights of step 0" % nb, got, want, args.dtype, {"first_step_loss_full_batch": first})
    loss = [None]

    def run():
        loss[0] = stepper.step(imgs, target)
    elapsed, steps = timed_region(run, args.train_steps, args.train_warmup, world, args.min_seconds, args.exact, min(args.regions, 3))
    name = ("C4 student KL-distillation train step (BASELINE configs[3]): %d x 3x%dx%d per GPU, teacher arch_0 eval (engine) + student arch_1 "
            "train (3 heads), OHEM-CE + KLDiv, SGD" % (batch, H, W))
    line = _train_line(args, world, backend, name, batch, elapsed, steps, args.train_warmup, {"final_loss": float(loss[0]), "parity": parity})
    if not args.no_roofline:
        extra = []
        if rank == 0 and stepper.teacher_engine is not None:
            extra = stepper.teacher_engine.census_entries(stepper.teacher_engine.profile_in_frame(frames=3, warm=1))
        timed = _timed_census(args, world, rank, lambda: stepper.step(imgs, target), extra, workload="c4")
        if timed:
            line.update(timed)
            _close_step_roofline(line)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # the same step on the CPU oracle, on a 2-image sample (teacher eval forward + student train forward/backward)
        nb = 2
        for k, v in ps.items():
            if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
        xi, ti = imgs[:nb].cpu(), target[:nb].cpu()

        def cpu_step():
            with torch.no_grad():
                t_logits = ref_ops.derived_forward(pt, meta_t, xi, training=False)
            p8, p16, p32 = ref_ops.derived_forward(ps, meta_s, xi, training=True)
            ref_loss.student_step_loss(p8, p16, p32, t_logits, ti, min_kept=nb * H * W // 16).backward()
        line["cpu_baseline"] = _time_cpu(cpu_step, nb, args.cpu_seconds,
                                         "%d images of 3x%dx%d: teacher eval forward + student train forward/backward through oracle/ref_ops, "
                                         "OHEM-CE + KLDiv through oracle/ref_loss" % (nb, H, W))
    del stepper
    line.update(_other_leg(args, world, make, lambda st: (lambda: st.step(imgs, target)), batch))
    return line


CPU_THREAD_SWEEP = (16, 32, 8, 64)              # tried in this order until the sample's budget is spent


def _time_cpu(fn, images, budget_s, what, threads=None, unit="images/s"):
    """cpu_baseline of one workload: `fn` = one pass of the CPU oracle over `images` units.  The oracle's maps are small (45 convs on a
    frame, a few thousand pixels in the supernet): with one torch thread per core of a 128-core host the CPU kernels spend their time in
    fork/join (0.8 fps on 128 threads, 4.4 fps on 8).  So the thread count is SWEPT - one pass per candidate after a
    warm-up - and the rest of the budget is spent at the fastest one; `cores` states it, `sample` lists the sweep."""
    all_threads = torch.get_num_threads()
    cands = []
    for t in (threads or CPU_THREAD_SWEEP):
        if min(t, all_threads) not in cands:
            cands.append(min(t, all_threads))
    sweep = {}
    try:
        torch.set_num_threads(cands[0])
        t0 = time.perf_counter()
        fn()                                               # warm-up (allocator, oneDNN primitive caches)
        first = time.perf_counter() - t0
        spent = first
        for t in cands:
            if sweep and spent + min(sweep.values()) > budget_s:       # out of budget: the candidates not reached are left out
                break
            torch.set_num_threads(t)
            t0 = time.perf_counter()
            fn()
            sweep[t] = time.perf_counter() - t0
            spent += sweep[t]
        best = min(sweep, key=sweep.get)
        torch.set_num_threads(best)
        n, el = 1, sweep[best]
        if spent + el < budget_s:
            n, t0 = 0, time.perf_counter()
            while True:
                fn()
                n += 1
                el = time.perf_counter() - t0
                if spent + el >= budget_s or n >= 20:
                    break
    finally:
        torch.set_num_threads(all_threads)
    return {"value": round(images * n / el, 4), "unit": unit, "cores": best, "kind": "port",
            "sample": "%s; threads swept %s s/pass (host has %d), %d timed pass(es) at %d threads, %.1f s" %
                      (what, {t: round(v, 2) for t, v in sweep.items()}, all_threads, n, best, el)}


def run_supernet(args, world, rank, backend, pretrain):
    import numpy as np
    from fasterseg_amd import latency_lookup_table, train_step
    from oracle import ref_supernet
    batch = 3 if pretrain else 2
    H, W = (256, 512) if pretrain else (224, 448)
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    lut = None if pretrain else latency_lookup_table.load_shipped("bf16")
    make = lambda d: train_step.SupernetStep(pretrain=pretrain, lut=lut, compute_dtype=d)
    stepper = make(dt)
    g = torch.Generator().manual_seed(2000 + rank)

    def make_batch():
        imgs = torch.randn(batch, 3, H, W, generator=g).cuda()
        tgt = torch.randint(0, 19, (batch, H // 8, W // 8), generator=g)
        tgt[torch.rand(batch, H // 8, W // 8, generator=g) < 0.05] = 255
        return imgs, tgt.cuda()
    imgs, target = make_batch()
    imgs_s, target_s = make_batch()
    cfg = dict(layers=train_step.SearchConfig.layers, width_mult_list=train_step.SearchConfig.width_mult_list,
               prun_modes=train_step.SearchConfig.prun_modes, stem_head_width=train_step.SearchConfig.stem_head_width)
    params = {k: v.detach().cpu().clone() for k, v in stepper.model.state_dict().items()}       # the weights the first step sees
    # ---- parity gate: the FIRST step of the stepper that is about to be timed (graph capture, programs, pair batching and all) vs the
    # CPU oracle's `_loss` on the same batch, same weights, same host-RNG seeds (np.random widths / torch.rand Gumbel noise).  Pretrain:
    # the weight step's loss.  Search: the architecture step's `_loss` on the search batch (it runs first, on the initial weights and
    # architecture parameters; the latency penalty is reported separately).
    SEED = 4242
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    first_w, first_a = stepper.step(imgs, target, imgs_s, target_s)
    parity = None
    if rank == 0:
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        threads = torch.get_num_threads()
        torch.set_num_threads(min(32, threads))
        try:
            with torch.no_grad():
                xi, ti = (imgs, target) if pretrain else (imgs_s, target_s)
                want = float(ref_supernet.loss(params, cfg, xi.cpu(), ti.cpu(), pretrain))
        finally:
            torch.set_num_threads(threads)
        got = float(first_w) if pretrain else float(stepper.last_arch_ce)
        parity = _parity("oracle.ref_supernet.loss (`_loss` of search/model_search.py:478-505, 4 passes) on the full batch, weights and RNG "
                         "seeds of step 0%s" % ("" if pretrain else "; architecture step's loss without the latency penalty"), got, want, args.dtype)
    np.random.seed(SEED + 1)
    torch.manual_seed(SEED + 1)
    out = [None, None]

    def run():
        out[0], out[1] = stepper.step(imgs, target, imgs_s, target_s)
    elapsed, steps = timed_region(run, args.train_steps, args.train_warmup, world, args.min_seconds, args.exact, min(args.regions, 3))
    if pretrain:
        name = "C3 supernet pretrain step (BASELINE configs[2]): %d x 3x%dx%d per GPU, F12.L16, widths {4,6,8,10,12}/12, all 5 primitives per MixedOp, " \
               "4 width passes fwd+bwd, clip 5, SGD" % (batch, H, W)
    else:
        name = "C5 architecture-search step (BASELINE configs[4]): arch update (Architect.step, Adam) + weight update, %d x 3x%dx%d per GPU for " \
               "each, F12.L16; latency table = shipped MI355X table (667 hipEvent-timed entries, fasterseg_amd/latency_lookup_table.py)" % (batch, H, W)
    line = _train_line(args, world, backend, name, batch, elapsed, steps, args.train_warmup,
                       {"final_loss": float(out[0]), "arch_loss": None if out[1] is None else float(out[1]), "parity": parity,
                        "eager_passes_per_phase": sum(1 for s_ in stepper._specs() if not stepper._is_static(s_)),
                        "execution": stepper.describe()})
    # ---- after the timed region (a capture-path fault that appears "from the 5th replay on" would pass a step-0 gate):
    # the state the replayed steps left behind must be finite, and the NEXT step issued eagerly (no graph replay, same kernels) must land
    # next to the last replayed one - consecutive steps on one batch differ by the width draws and one small SGD step, not by 25 %
    graphed_loss = float(out[0])
    eager_next = [None]

    def eager_step():
        eager_next[0] = stepper.step(imgs, target, imgs_s, target_s, force_eager=True)
    if not args.no_roofline:
        timed = _timed_census(args, world, rank, eager_step, workload="c3" if pretrain else "c5")
        if timed:
            line.update(timed)
            _close_step_roofline(line)
    else:
        eager_step()
    eager_loss = float(eager_next[0][0])
    flat = stepper.sync.flat
    check = {"last_replayed_loss": graphed_loss, "next_eager_loss": eager_loss,
             "rel_change": abs(eager_loss - graphed_loss) / max(abs(graphed_loss), 1e-12), "steps_before": steps + args.train_warmup + 1,
             "grads_finite": bool(torch.isfinite(flat).all()), "weights_finite": all(bool(torch.isfinite(p).all()) for p in stepper.weights),
             "bar": "finite state after the timed region; |eager next loss - last replayed loss| <= 25 %"}
    check["pass"] = bool(check["grads_finite"] and check["weights_finite"] and math.isfinite(eager_loss) and check["rel_change"] <= 0.25)
    line["post_timed_check"] = check
    if not check["pass"]:
        raise SystemExit("bench.py: the supernet step's state after the timed region is not sane: %s" % json.dumps(check))
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        for k, v in params.items():
            if v.is_floating_point() and not k.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
        # the WHOLE per-GPU batch (one image normalises its BatchNorms over a third / half of the pixels the step does)
        xi, ti = imgs.cpu(), target.cpu()

        def cpu_step():
            if not pretrain:                               # the architecture step's `_loss` on the search batch, then the weight step's
                ref_supernet.loss(params, cfg, xi, ti, False).backward()
            ref_supernet.loss(params, cfg, xi, ti, pretrain).backward()
        line["cpu_baseline"] = _time_cpu(cpu_step, batch, args.cpu_seconds,
                                         "the step's batch, %d images" % batch + " of 3x%dx%d: %s through oracle/ref_supernet (port of search/model_search.py on torch-CPU "
                                         "kernels, fixture-pinned)" % (H, W, "`_loss(pretrain)` forward+backward" if pretrain else
                                                                       "`_loss` forward+backward of the arch step and of the weight step"),
                                         threads=(16, 32, 8))
    del stepper
    line.update(_other_leg(args, world, make, lambda st: (lambda: st.step(imgs, target, imgs_s, target_s)), batch))
    return line


# ---- the printed line ------------------------------------------------------------------------------------------------------
LINE_LIMIT = 4096                                    # bytes; the driver could not parse round 3's 24 KB line
_ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "launches_per_step", "avg_launch_us")
_CPU_KEYS = ("value", "unit", "cores", "kind")


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def _sig(x, digits=5):
    """floats of the printed line to `digits` significant digits (recursively)"""
    if isinstance(x, float):
        return float("%.*g" % (digits, x)) if math.isfinite(x) else None
    if isinstance(x, dict):
        return {k: _sig(v, digits) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_sig(v, digits) for v in x]
    return x


def _short(text, n):
    text = str(text)
    return text if len(text) <= n else text[:n - 3] + "..."


def compact_workload(w):
    """The per-workload object of the printed line: numbers only, no method strings, no per-kernel tables."""
    out = _pick(w, ("value", "unit", "ms_per_step", "steps", "dtype", "ms_per_step_fp32", "value_fp32", "fp32_steps", "ms_per_step_bf16", "value_bf16",
                    "bf16_steps", "per_gpu_batch"))
    par = w.get("parity") or {}
    out["parity"] = _pick(par, ("pass", "rel_err", "max_abs_err", "rel_to_max_logit", "argmax_agreement"))
    if w.get("post_timed_check"):
        out["parity"]["after_timed"] = bool(w["post_timed_check"].get("pass"))
    if w.get("roofline"):
        out["roofline"] = _pick(w["roofline"], _ROOF_KEYS)
    if w.get("step_roofline"):
        out["step_roofline"] = _pick(w["step_roofline"], ("ideal_ms", "frac", "launches"))
    if w.get("cpu_baseline"):
        out["cpu_baseline"] = _pick(w["cpu_baseline"], _CPU_KEYS)
    return out


def build_line(c2, train, world, steps_requested, dtype, detail_path):
    """(printed line, detail) from the full result dictionaries.  The line carries the contract's scalars, `config` (workload +
    parallelism), `parity`, `roofline` of the dominant kernel family, `cpu_baseline` and one small object per workload; everything
    else (autotune logs, per-kernel tables, method strings, clocks) is `detail`, written to `detail_path`."""
    line = {"metric": METRIC, "value": c2["value"], "unit": c2["unit"], "n_gpus": world, "steps": c2["steps"], "warmup": c2["warmup"],
            "ms_per_step": c2["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": c2.get("vs_baseline"),
            "dtype": dtype, "data": "synthetic",
            "config": {"workload": _short(c2["config"]["workload"], 220), "parallelism": _short(c2["config"]["parallelism"], 100)}}
    if steps_requested is not None and steps_requested != c2["steps"]:
        line["steps_requested"] = steps_requested
    if c2.get("parity"):
        line["parity"] = compact_workload(c2)["parity"]
    for k in ("alg_gflop_per_frame", "alg_mb_per_frame"):
        if k in c2:
            line[k] = c2[k]
    if c2.get("roofline"):
        line["roofline"] = _pick(c2["roofline"], _ROOF_KEYS)
    if c2.get("frame_roofline"):
        line["frame_roofline"] = _pick(c2["frame_roofline"], ("ideal_ms", "frac"))
    if c2.get("cpu_baseline"):
        line["cpu_baseline"] = dict(_pick(c2["cpu_baseline"], _CPU_KEYS), sample=_short(c2["cpu_baseline"].get("sample", ""), 110))
    if c2.get("fp32"):               # the same engine in the reference's arithmetic: north_star's ">= 163 fps, logits within 1e-3" in one record
        line["fp32"] = _pick(c2["fp32"], ("value", "unit", "ms_per_step", "max_abs_err", "vs_baseline"))
    if c2.get("class_map"):
        line["class_map"] = _pick(c2["class_map"], ("value", "unit", "ms_per_step"))
    workloads = {"C2_student_infer": _pick(c2, ("value", "unit", "ms_per_step", "steps", "dtype"))}    # its objects are the top-level ones
    for name, w in train.items():
        workloads[name] = compact_workload(w)
    line["workloads"] = workloads
    line["detail"] = os.path.relpath(detail_path, ROOT) if detail_path else None
    line = _sig(line)
    detail = {"C2_student_infer": c2}
    detail.update(train)
    return fit_line(line), detail


def fit_line(line, limit=LINE_LIMIT):
    """Never let the printed line outgrow what the driver parses (round 3 lost its whole result to a 24 KB line), and never lose the
    result to the limit either: optional objects are dropped widest first, then the per-workload objects are thinned, then
    strings are cut, and as a last resort only the contract's scalars remain with a pointer to the detail file."""
    size = lambda: len(json.dumps(line))
    for k in ("class_map", "frame_roofline", "alg_mb_per_frame", "alg_gflop_per_frame", "steps_requested"):
        if size() < limit:
            return line
        line.pop(k, None)
    for drop in (("step_roofline",), ("cpu_baseline",), ("parity",), ("roofline",), ("fp32_steps", "bf16_steps", "per_gpu_batch", "steps", "unit")):
        for w in (line.get("workloads") or {}).values():
            if size() < limit:
                return line
            for k in drop:
                w.pop(k, None)
    if size() >= limit and isinstance(line.get("cpu_baseline"), dict):
        line["cpu_baseline"].pop("sample", None)
    if size() >= limit:
        for k in ("workload", "parallelism"):
            line["config"][k] = _short(line["config"].get(k, ""), 60)
    if size() >= limit:
        line.pop("workloads", None)
    if size() >= limit:
        keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "detail")
        for k in [k for k in line if k not in keep]:
            line.pop(k)
        line["metric"] = _short(line["metric"], 100)
    return line


def device_clocks():
    """sclk / mclk / power of GPU 0 as rocm-smi reports them right now (explain box-to-box spread)."""
    import subprocess
    try:
        r = subprocess.run(["rocm-smi", "-d", "0", "--showclocks", "--showpower", "--showtemp", "--json"], capture_output=True, text=True, timeout=20)
        d = json.loads(r.stdout)
        card = d.get("card0", d)
        keep = {k: v for k, v in card.items() if any(t in k.lower() for t in ("sclk", "mclk", "fclk", "power", "temperature (sensor junction)"))}
        return keep or card
    except Exception as e:                              # rocm-smi missing / busy: the bench result does not depend on it
        return {"error": repr(e)[:120]}


def host_info():
    info = {"logical_cpus": os.cpu_count(), "torch_threads": torch.get_num_threads()}
    try:
        with open("/proc/cpuinfo") as f:
            models = [l.split(":", 1)[1].strip() for l in f if l.startswith("model name")]
        info["cpu_model"] = models[0] if models else None
        mhz = [float(l.split(":", 1)[1]) for l in open("/proc/cpuinfo") if l.startswith("cpu MHz")]
        if mhz:
            info["cpu_mhz_max_now"] = max(mhz)
        info["loadavg"] = open("/proc/loadavg").read().split()[:3]
    except Exception as e:
        info["error"] = repr(e)[:80]
    return info


def main():
    args = parse()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the measured path)")
    world, rank, backend = dist_setup(args)
    import copy
    targs = copy.copy(args)                    # the train workloads' own precision (default fp32: the reference's arithmetic); C2 keeps --dtype
    targs.dtype = args.train_dtype
    runners = {"c3": ("C3_supernet_pretrain", lambda: run_supernet(targs, world, rank, backend, True)),
               "c4": ("C4_student_train", lambda: run_student_train(targs, world, rank, backend)),
               "c5": ("C5_supernet_search", lambda: run_supernet(targs, world, rank, backend, False))}
    train = {}
    clocks = {}
    # The supernet steps are HOST-bound: run them before the student train step, whose teardown leaves the
    # process ~15 % slower at issuing launches (measured on one box: C3 83.9 ms first / 87.3 ms after C2 / 101.6 ms after C2 + C4 with its
    # CPU-oracle and fp32 legs; profiles/r05_bench_order.txt).  C4 itself is device-bound and does not care.  FS_BENCH_ORDER overrides.
    order = os.environ.get("FS_BENCH_ORDER", "c2,c3,c5,c4").split(",")
    c2 = None

    def clocked(name, fn):
        if rank == 0 and args.full:
            clocks[name] = {"before": device_clocks()}
        out = fn()
        if rank == 0 and args.full:
            clocks[name]["after"] = device_clocks()
        return out
    for key in order:
        if key == "c2":
            torch.cuda.empty_cache()
            c2 = clocked("C2_student_infer", lambda: run_student_infer(args, world, rank, backend))
        elif key in args.workloads and key in runners:
            name, fn = runners[key]
            torch.cuda.empty_cache()
            train[name] = clocked(name, fn)
    if c2 is None:
        c2 = clocked("C2_student_infer", lambda: run_student_infer(args, world, rank, backend))
    if rank == 0:
        line, detail = build_line(c2, train, world, args.steps_requested, args.dtype, args.detail)
        detail["argv"] = sys.argv[1:]
        detail["order"] = order
        if args.full:
            detail["clocks"] = clocks
            detail["host"] = host_info()      # the supernet steps are host-bound: the box's CPU is part of the result
        if args.detail:
            try:
                with open(args.detail, "w") as f:
                    json.dump(detail, f, indent=1, default=str)
            except OSError as e:
                line["detail"] = "not written: %r" % (e,)
        text = json.dumps(fit_line(line))
        sys.stdout.flush()
        print(text, flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
