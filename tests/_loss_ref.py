"""Plain fp64 references of the loss heads and class maps (no product code): what the *_up_* kernels of csrc/loss_up.hip, the
full-resolution kernels of csrc/loss.hip and the class-map kernels of csrc/eval.hip / eval_heads.hip compute, restated with torch
ops on CPU doubles.  Logits come in already rounded to their storage dtype; everything after that is double (or, where `dtype`
says so, the same chain in fp32, which the tests use to size their tolerances)."""
import torch
import torch.nn.functional as F


def upsample(x, size, dtype=torch.float64):
    """(N, C, h, w) -> (N, C, H, W), bilinear with align_corners=True (train/model_seg.py:357-362)."""
    return F.interpolate(x.to(dtype), size=tuple(size), mode="bilinear", align_corners=True)


def valid_mask(target, C, ignore):
    return target.ne(ignore) & target.ge(0) & target.lt(C)


def ohem_vectors(logits, target, ignore=255):
    """logits (N, C, H, W), target (N, H, W) int64 -> flat per-pixel (true_prob, nll, lse, valid), p = (n * H + y) * W + x.
    nll = lse - x[target] (0 when not valid), true_prob = exp(-nll) (1 when not valid), valid = target != ignore and 0 <= target < C."""
    C = logits.shape[1]
    valid = valid_mask(target, C, ignore)
    lse = torch.logsumexp(logits, dim=1)
    logp = F.log_softmax(logits, dim=1)
    safe = torch.where(valid, target, torch.zeros_like(target))
    picked = logp.gather(1, safe.unsqueeze(1)).squeeze(1)
    nll = torch.where(valid, -picked, torch.zeros_like(picked))
    true_prob = torch.where(valid, torch.exp(picked), torch.ones_like(picked))
    return true_prob.reshape(-1), nll.reshape(-1), lse.reshape(-1), valid.reshape(-1)


def kl_vectors(student, teacher):
    """(N, C, H, W) logits -> flat per-pixel (kl, lse_s, lse_t); kl = sum_c p_t (log p_t - log p_s), 0 log 0 = 0 (xlogy)."""
    lps, lpt = F.log_softmax(student, dim=1), F.log_softmax(teacher, dim=1)
    pt = torch.exp(lpt)
    term = torch.where(pt > 0, pt * (lpt - lps), torch.zeros_like(pt))
    return term.sum(1).reshape(-1), torch.logsumexp(student, dim=1).reshape(-1), torch.logsumexp(teacher, dim=1).reshape(-1)


def ohem_grad(lo, size, target, coef, scale, ignore=255, dtype=torch.float64):
    """d / d lo of scale * sum_p coef[p] * nll[p]; size None: `lo` is the full-resolution map itself."""
    x = lo.to(dtype).clone().requires_grad_(True)
    full = x if size is None else upsample(x, size, dtype)
    nll = ohem_vectors(full, target, ignore)[1]
    (float(scale) * (coef.reshape(-1).to(dtype) * nll).sum()).backward()
    return x.grad


def kl_grad(s_lo, t_lo, size, scale, dtype=torch.float64):
    """d / d s_lo of scale * sum_p kl[p]; size None: both maps are at full resolution already."""
    x = s_lo.to(dtype).clone().requires_grad_(True)
    s = x if size is None else upsample(x, size, dtype)
    t = t_lo.to(dtype) if size is None else upsample(t_lo, size, dtype)
    (float(scale) * kl_vectors(s, t)[0].sum()).backward()
    return x.grad


def ohem_criterion(logits, target, thresh, min_kept, ignore=255, weight=None):
    """ProbOhemCrossEntropy2d (tools/seg_opr/loss_opr.py:63-93) on double logits with labels outside [0, C) ignored: the loss and the
    per-pixel coefficient (class weight of a kept pixel, 0 otherwise) such that loss = sum coef * nll / sum coef."""
    C = logits.shape[1]
    true_prob, nll, _, valid = ohem_vectors(logits, target, ignore)
    kept = valid.clone()
    num_valid = int(valid.sum())
    if min_kept > 0 and num_valid >= min_kept and num_valid > 0:
        kth = torch.sort(true_prob).values[min(true_prob.numel(), min_kept) - 1]
        kept = valid & true_prob.le(max(float(thresh), float(kth)))
    w = torch.ones(C, dtype=logits.dtype) if weight is None else torch.as_tensor(weight, dtype=logits.dtype)
    flat = target.reshape(-1)
    safe = torch.where(valid, flat, torch.zeros_like(flat))
    coef = torch.where(kept, w[safe], torch.zeros_like(nll))
    return (coef * nll).sum() / coef.sum(), coef


def class_map(lo, size):
    """fp64 up-sample of the storage-rounded logits -> (up, arg-max (first maximum wins), gap between the two largest values;
    +inf with a single class)."""
    up = upsample(lo, size)
    arg = up.argmax(1)
    if up.shape[1] == 1:
        return up, arg, torch.full(arg.shape, float("inf"), dtype=torch.float64)
    top = up.topk(2, dim=1).values
    return up, arg, top[:, 0] - top[:, 1]


def check_class_map(got, up, arg, gap, clear_gap=1e-4):
    """Every pixel is checked: on a clear pixel (gap > clear_gap) the class is the fp64 arg-max, on any other a class whose fp64
    value is within clear_gap of the maximum.  Returns the share of clear pixels."""
    got = got.long().cpu()
    clear = gap > clear_gap
    assert torch.equal(got[clear], arg[clear]), "%d clear pixels differ from the fp64 arg-max" % int((got[clear] != arg[clear]).sum())
    val = up.gather(1, got.unsqueeze(1)).squeeze(1)
    assert bool((val >= up.max(1).values - clear_gap).all()), "a near-tie pixel took a class more than the gap below the maximum"
    return float(clear.double().mean())


def hist_info(n_cl, pred, gt):
    """tools/seg_opr/metric.py:7-17 on numpy arrays."""
    import numpy as np
    k = (gt >= 0) & (gt < n_cl)
    hist = np.bincount(n_cl * gt[k].astype(np.int64) + pred[k].astype(np.int64), minlength=n_cl ** 2).reshape(n_cl, n_cl)
    return hist, int(k.sum()), int((pred[k] == gt[k]).sum())
