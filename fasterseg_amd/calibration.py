"""From a confidence histogram to per-class thresholds (class-balanced self-training), on the host, in exact integer arithmetic.

`ConfidenceHistogram` accumulates fs_confidence_hist over a run on the device and is read back once: an int64 (2, C, 256) array,
hist[0][k][q] the pixels predicted as class k with confidence byte q (those that were RIGHT when labels were given), hist[1][k][q]
those that were wrong (all zero without labels).  The functions below turn it into the uint8 (C,) bytes the per-class kernels compare
with (kernels.class_threshold_table; a pixel of class k is kept iff q >= t_k):

  class_balanced_thresholds   class k keeps at least a chosen share of the pixels predicted as k
  precision_thresholds        class k keeps pixels down to the lowest byte at which the kept ones still reach a chosen precision
  reliability                 kept share, precision and calibration error as arrays, for a caller to print or plot

A share or precision given as a float is replaced by the exact rational fractions.Fraction(value).limit_denominator(10 ** 6) - 0.9 is
9/10, not the double next to it - and every comparison that decides a byte is between Python / int64 integers."""
import fractions

import numpy as np
import torch

from . import kernels as K


class ConfidenceHistogram:
    """Device accumulator of (predicted class, confidence byte[, right / wrong]) counts, in the style of metric.HistAccumulator."""

    def __init__(self, class_num, device="cuda"):
        self.class_num = int(class_num)
        self.hist = torch.zeros((2, self.class_num, 256), dtype=torch.int64, device=device)

    def add(self, classes, conf, gt=None):
        """One fs_confidence_hist launch: uint8 maps of one shape, optionally with uint8 / int32 / int64 labels of that shape."""
        assert classes.is_cuda and conf.is_cuda and (gt is None or gt.is_cuda)
        K.confidence_hist(classes, conf, self.class_num, gt=gt, hist=self.hist)

    def result(self):
        """int64 (2, C, 256) numpy - one device-to-host read for the whole run."""
        return self.hist.cpu().numpy()


def _rational(value, what, low_open):
    """value -> (num, den) of its exact rational; ValueError outside (0, 1] (low_open) or [0, 1]"""
    try:
        f = fractions.Fraction(value).limit_denominator(10 ** 6)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s must be a number in %s0, 1], got %r" % (what, "(" if low_open else "[", value))
    if not (0 < f if low_open else 0 <= f) or f > 1:
        raise ValueError("%s must be in %s0, 1], got %r" % (what, "(" if low_open else "[", value))
    return f.numerator, f.denominator


def _hist(hist):
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[0] != 2 or h.shape[2] != 256 or not np.issubdtype(h.dtype, np.integer):
        raise ValueError("hist must be an integer array of shape (2, C, 256), got %s %s" % (h.dtype, h.shape))
    return h.astype(np.int64)


def _tails(h):
    """tail[..., t] = sum of h[..., t:]"""
    return np.cumsum(h[..., ::-1], axis=-1)[..., ::-1]


def class_balanced_thresholds(hist, portion, floor=0.0, cap=1.0):
    """uint8 (C,): with h = hist[0] + hist[1] and n_k the pixels predicted as class k, t_k is the LARGEST byte t whose kept count
    h[k][t:].sum() is at least need_k = ceil(portion * n_k): class k keeps at least `portion` of its pixels and one byte higher would
    keep fewer than that.  need_k = (num * n_k + den - 1) // den with num / den = Fraction(portion).limit_denominator(10 ** 6), in
    integers.  A class with no pixel gets the cap byte.  Then t_k = min(max(t_k, confidence_threshold(floor)), confidence_threshold(cap)).
    portion outside (0, 1]: ValueError."""
    num, den = _rational(portion, "portion", low_open=True)
    lo, hi = K.confidence_threshold(floor), K.confidence_threshold(cap)
    h = _hist(hist).sum(axis=0)
    tails = _tails(h)                                          # non-increasing in t; tails[:, 0] = n_k
    out = np.empty(h.shape[0], dtype=np.int64)
    for k in range(h.shape[0]):
        n = int(tails[k, 0])
        if n == 0:
            out[k] = hi
            continue
        need = (num * n + den - 1) // den                      # >= 1 since portion > 0, <= n since portion <= 1: t = 0 always qualifies
        out[k] = int(np.flatnonzero(tails[k] >= need)[-1])
    return np.minimum(np.maximum(out, lo), hi).astype(np.uint8)


def precision_thresholds(hist, precision, cap=1.0):
    """uint8 (C,) from a labelled histogram: with right(t) = hist[0][k][t:].sum() and wrong(t) = hist[1][k][t:].sum(), t_k is the
    SMALLEST byte t at which something is kept, right(t) + wrong(t) > 0, and the kept pixels reach the precision,
    right(t) * den >= num * (right(t) + wrong(t)), num / den = Fraction(precision).limit_denominator(10 ** 6).  A class that never
    reaches it (or has no pixel) gets the cap byte, and no class exceeds it.  precision outside [0, 1]: ValueError."""
    num, den = _rational(precision, "precision", low_open=False)
    hi = K.confidence_threshold(cap)
    h = _hist(hist)
    right, wrong = _tails(h[0]), _tails(h[1])
    out = np.empty(h.shape[1], dtype=np.int64)
    for k in range(h.shape[1]):
        r = [int(v) for v in right[k]]                         # Python integers: right * den cannot overflow
        w = [int(v) for v in wrong[k]]
        out[k] = next((t for t in range(256) if r[t] + w[t] > 0 and r[t] * den >= num * (r[t] + w[t])), hi)
    return np.minimum(out, hi).astype(np.uint8)


def reliability(hist):
    """Curves of a histogram, per class (rows 0..C-1) and overall (row C), as a dict of numpy arrays:
      "count"      int64 (C + 1, 256): pixels per confidence byte (both planes)
      "right"      int64 (C + 1, 256): those of plane 0
      "kept"       float64 (C + 1, 256): the share of the row's pixels with byte >= t (NaN for an empty row)
      "precision"  float64 (C + 1, 256): right / all among the pixels with byte >= t (NaN where nothing is kept); labelled histograms
      "ece"        float64 (C + 1,): expected calibration error over the 256 bins, sum_q count_q / n * |right_q / count_q - q / 255|
    The float arrays are for printing and plotting; nothing here decides a threshold."""
    h = _hist(hist)
    count = h.sum(axis=0)
    count = np.concatenate([count, count.sum(axis=0, keepdims=True)])
    right = np.concatenate([h[0], h[0].sum(axis=0, keepdims=True)])
    n = count.sum(axis=1, keepdims=True).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        kept = _tails(count) / n
        precision = _tails(right) / _tails(count).astype(np.float64)
        acc = right / count.astype(np.float64)
        gap = np.where(count > 0, np.abs(acc - np.arange(256) / 255.0), 0.0)
        ece = (count * gap).sum(axis=1) / n[:, 0]
    return {"count": count, "right": right, "kept": kept, "precision": precision, "ece": ece}
