"""Regenerates tests/golden/loss_weighted.npz from the UNMODIFIED reference (build container only, CPU).

    python tools/make_loss_weighted_golden.py

The reference's ProbOhemCrossEntropy2d (tools/seg_opr/loss_opr.py:43-93) is imported through oracle.ref_loader.reference("train") with
the scratch copy's tools/ directory on sys.path, as oracle/make_golden.py does for the unweighted fixture, and built with
use_weight=True.  Its constructor moves the weight table to a GPU (`.cuda()`, loss_opr.py:52-55); for the duration of the construction
this tool makes torch.Tensor.cuda return the tensor itself, so the criterion lives on the CPU.  No reference file is edited.

Only data is written: the reference's 19 class weights (read back from the criterion it built), four cases of seeded logits, labels,
(thresh, min_kept), the loss and the gradient the reference returned, and for the three cases with min_kept > 0 the k-th smallest
true-class probability (the reference's own expressions, loss_opr.py:70-83) and the number of pixels the reference kept (counted on the
target it hands to its CrossEntropyLoss).  Shapes and settings are those of tests/test_losses_gpu.py's first parametrisation, with 19
classes in the last case too: the reference's table has 19 entries.  Logits are rounded to fp16 values so that they store in half
the bytes and read back exactly."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = (dict(shape=(2, 19, 32, 48), thresh=0.7, min_kept=2 * 32 * 48 // 16, ignore_frac=0.05),
         dict(shape=(3, 19, 17, 23), thresh=0.05, min_kept=400, ignore_frac=0.1),
         dict(shape=(1, 19, 16, 16), thresh=0.7, min_kept=10 ** 6, ignore_frac=0.0),
         dict(shape=(2, 19, 20, 20), thresh=0.9, min_kept=0, ignore_frac=0.5))


def inputs(i, case):
    g = torch.Generator().manual_seed(70 + i)
    B, C, H, W = case["shape"]
    pred = (torch.randn(B, C, H, W, generator=g) * 2.0).half().float()
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < case["ignore_frac"]] = 255
    return pred, target


def run_reference():
    from oracle import ref_loader
    store = {}
    with ref_loader.reference("train") as wd:
        sys.path.insert(0, os.path.join(os.path.dirname(wd), "tools"))
        for m in [k for k in sys.modules if k.split(".")[0] in ("seg_opr", "engine")]:
            sys.modules.pop(m)
        from seg_opr.loss_opr import ProbOhemCrossEntropy2d
        for i, case in enumerate(CASES):
            pred, target = inputs(i, case)
            pred.requires_grad_(True)
            real_cuda = torch.Tensor.cuda
            torch.Tensor.cuda = lambda self, *a, **k: self          # loss_opr.py:55, for the construction only
            try:
                crit = ProbOhemCrossEntropy2d(ignore_label=255, thresh=case["thresh"], min_kept=case["min_kept"], use_weight=True)
            finally:
                torch.Tensor.cuda = real_cuda
            seen = {}
            inner = crit.criterion.forward

            def record(p, t, inner=inner, seen=seen):               # the masked target the reference reduces over
                seen["kept"] = int(t.ne(255).sum())
                return inner(p, t)
            crit.criterion.forward = record
            loss = crit(pred, target.clone())
            loss.backward()
            store["weight"] = crit.criterion.weight.detach().numpy().astype(np.float32)
            store["ohem%d/pred" % i] = pred.detach().numpy().astype(np.float16)
            store["ohem%d/target" % i] = target.numpy().astype(np.uint8)
            store["ohem%d/cfg" % i] = np.array([case["thresh"], case["min_kept"]])
            store["ohem%d/loss" % i] = np.array([float(loss.detach())])
            store["ohem%d/grad" % i] = pred.grad.numpy().astype(np.float32)
            if case["min_kept"] > 0:
                with torch.no_grad():                               # loss_opr.py:65-83
                    flat = target.view(-1)
                    valid = flat.ne(255)
                    prob = F.softmax(pred, dim=1).transpose(0, 1).reshape(pred.shape[1], -1).masked_fill_(~valid, 1)
                    mask_prob = prob[flat * valid.long(), torch.arange(len(flat), dtype=torch.long)]
                    index = mask_prob.argsort()
                    kth = mask_prob[index[min(len(index), case["min_kept"]) - 1]]
                store["ohem%d/kth" % i] = np.array([float(kth)], dtype=np.float32)
                store["ohem%d/kept" % i] = np.array([seen["kept"]], dtype=np.int64)
    return store


def main():
    store = run_reference()
    path = os.path.join(GOLD, "loss_weighted.npz")
    np.savez_compressed(path, **store)
    print("wrote loss_weighted.npz: %d arrays, %d bytes; losses" % (len(store), os.path.getsize(path)),
          [float(store["ohem%d/loss" % i][0]) for i in range(len(CASES))])


if __name__ == "__main__":
    main()
