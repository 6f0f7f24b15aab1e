"""fs_ohem_select against the torch chain of losses._OhemCE.forward (the sort through to the loss), one MI355X.

One seeded true_prob / nll / target of P = 12 x 512 x 1024 pixels with 5 % ignored labels, thresh 0.7, min_kept = P / 16 (the student
step's setting, train/train.py:62), weight=None.  Both sides are timed with device events around `--calls` consecutive calls after
`--warmup` calls, `--rounds` times alternating the two in one process; the median round is reported, with the minimum.  The bytes of a
select call are the kernels' own count (FS_NOTE_BYTES, read back through one census-level-2 call), the per-kernel times come from the
same call.  The two sides are checked against each other first (threshold bit-equal, same kept set).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IGNORE = 255


def vectors(P, seed=1):
    g = torch.Generator().manual_seed(seed)
    tp = torch.rand(P, generator=g) ** 2                    # most pixels hard, a tail of easy ones
    tgt = torch.randint(0, 19, (P,), generator=g)
    tgt[torch.rand(P, generator=g) < 0.05] = IGNORE
    nll = -torch.log(tp.clamp_min(1e-30))
    tp[tgt == IGNORE] = 1.0
    nll[tgt == IGNORE] = 0.0
    return tp.cuda(), nll.cuda(), tgt.cuda()


def torch_chain(true_prob, nll, tgt, thresh, min_kept):
    """losses._OhemCE.forward between its two kernels, verbatim."""
    P = true_prob.numel()
    valid = tgt.ne(IGNORE)
    num_valid = valid.sum()
    kept = valid
    if min_kept > 0:
        threshold = torch.full((), float(thresh), dtype=torch.float32, device=true_prob.device)
        kth = torch.sort(true_prob).values[min(P, min_kept) - 1]
        threshold = torch.maximum(threshold, kth)
        apply = (num_valid >= min_kept) & (num_valid > 0)
        kept = valid & (true_prob.le(threshold) | ~apply)
    count = kept.sum()
    loss = (nll * kept).sum() / count
    return loss, kept.to(torch.uint8), count, threshold


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=12 * 512 * 1024)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from fasterseg_amd import _lib, census
    from fasterseg_amd.devtime import block_ms
    from fasterseg_amd.losses import ohem_select
    P = args.pixels
    thresh, min_kept = 0.7, P // 16
    tp, nll, tgt = vectors(P)
    ws = torch.empty((int(_lib.lib().fs_ohem_select_workspace_bytes(P)) + 7) // 8, dtype=torch.long, device="cuda")
    select = lambda: ohem_select(tp, nll, tgt, 19, IGNORE, thresh, min_kept, weight=None, workspace=ws)
    chain = lambda: torch_chain(tp, nll, tgt, thresh, min_kept)
    coef, result, counts = select()
    loss, kept, count, threshold = chain()
    torch.cuda.synchronize()
    assert result[2:3].view(torch.int32).item() == threshold.reshape(1).view(torch.int32).item(), "thresholds differ"
    assert torch.equal(coef.ne(0), kept.bool()) and int(counts[1]) == int(count), "kept sets differ"
    assert abs(float(result[0]) - float(loss)) <= 1e-5 * abs(float(loss)), (float(result[0]), float(loss))
    sel_ms, chain_ms = [], []
    for _ in range(args.rounds):
        sel_ms.append(block_ms(select, args.calls, warm=args.warmup))
        chain_ms.append(block_ms(chain, args.calls, warm=args.warmup))
    with census.recording(level=2) as rec:
        select()
    kernels = {k: {"launches": v[0], "us": round(v[1] * 1e3, 2), "bytes": rec.kernel_bytes.get(k, 0.0)}
               for k, v in rec.kernels.items() if k.startswith("ohem_select")}
    nbytes = sum(v["bytes"] for v in kernels.values())
    s, c = statistics.median(sel_ms), statistics.median(chain_ms)
    row = {"pixels": P, "min_kept": min_kept, "thresh": thresh, "calls": args.calls, "warmup": args.warmup, "rounds": args.rounds,
           "select_ms_median": round(s, 4), "select_ms_min": round(min(sel_ms), 4), "torch_chain_ms_median": round(c, 4),
           "torch_chain_ms_min": round(min(chain_ms), 4), "chain_over_select": round(c / s, 2), "select_launches": sum(v["launches"] for v in kernels.values()),
           "select_MB_per_call": round(nbytes / 1e6, 2), "select_GB_per_s": round(nbytes / 1e9 / (s / 1e3), 1), "kernels": kernels,
           "loss": float(result[0]), "kept": int(counts[1]), "valid": int(counts[0])}
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
