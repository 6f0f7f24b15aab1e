"""Host references of the per-class threshold tests: the (class, confidence byte, right / wrong) histogram with np.add.at, and threshold
pickers that work on the PIXELS (each class's bytes sorted; a Fraction comparison per candidate byte), not on a histogram, so they share
no code path with fasterseg_amd/calibration.py.  Everything is exact: integers and fractions.Fraction."""
import fractions
import math

import numpy as np


def exact(value):
    """the rational the product documents for a share or precision given as a float"""
    return fractions.Fraction(value).limit_denominator(10 ** 6)


def hist_numpy(classes, conf, C, gt=None):
    """int64 (2, C, 256) of fs_confidence_hist's contract"""
    k = np.asarray(classes).reshape(-1).astype(np.int64)
    q = np.asarray(conf).reshape(-1).astype(np.int64)
    hist = np.zeros((2, C, 256), dtype=np.int64)
    use = k < C
    if gt is None:
        np.add.at(hist, (np.zeros(int(use.sum()), dtype=np.int64), k[use], q[use]), 1)
        return hist
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    use &= (g >= 0) & (g < C)
    np.add.at(hist, ((k[use] != g[use]).astype(np.int64), k[use], q[use]), 1)
    return hist


def byte_of(t):
    """kernels.confidence_threshold, restated: the smallest byte q with q / 255 >= t"""
    return int(math.ceil(255.0 * float(t)))


def balanced_brute(classes, conf, C, portion, floor=0.0, cap=1.0):
    """class k: its bytes sorted downwards, need = ceil(portion n_k) of them must be kept, so the threshold is the need-th largest byte"""
    k = np.asarray(classes).reshape(-1)
    q = np.asarray(conf).reshape(-1)
    p = exact(portion)
    out = np.zeros(C, dtype=np.uint8)
    for c in range(C):
        b = np.sort(q[k == c])[::-1]
        if b.size == 0:
            t = byte_of(cap)
        else:
            need = math.ceil(p * int(b.size))
            t = int(b[need - 1])
        out[c] = min(max(t, byte_of(floor)), byte_of(cap))
    return out


def precision_brute(classes, conf, gt, C, precision, cap=1.0):
    """class k: the smallest byte t at which the labelled pixels predicted k with q >= t exist and are right at least `precision` of the time"""
    k = np.asarray(classes).reshape(-1).astype(np.int64)
    q = np.asarray(conf).reshape(-1).astype(np.int64)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    p = exact(precision)
    labelled = (g >= 0) & (g < C)
    out = np.zeros(C, dtype=np.uint8)
    for c in range(C):
        mine = labelled & (k == c)
        qc, right = q[mine], g[mine] == c
        t_k = byte_of(cap)
        for t in range(256):
            kept = qc >= t
            total = int(kept.sum())
            if total > 0 and fractions.Fraction(int(right[kept].sum()), total) >= p:
                t_k = t
                break
        out[c] = min(t_k, byte_of(cap))
    return out


def masked(classes, conf, thresholds, ignore_label=255):
    """where(conf >= thresholds[class], class, ignore_label) in numpy; classes < len(thresholds) everywhere"""
    classes, conf = np.asarray(classes), np.asarray(conf)
    t = np.asarray(thresholds, dtype=np.uint8)
    return np.where(conf >= t[classes], classes, np.uint8(ignore_label)).astype(np.uint8)


def skewed_maps(n=50000, C=19, seed=0, absent=(5, 11), single=7):
    """(classes, conf, gt) uint8 arrays of n pixels, skewed as a street scene is: three classes hold most pixels, most bytes are near
    255, classes `absent` never occur and class `single` has exactly one pixel; gt agrees with the class at about 80 % of the pixels, more
    often at high confidence, and holds 255 at some"""
    rng = np.random.default_rng(seed)
    w = 1.0 / (1.0 + np.arange(C)) ** 1.5
    w[list(absent)] = 0.0
    w[single] = 0.0
    k = rng.choice(C, size=n, p=w / w.sum()).astype(np.uint8)
    k[n // 2] = single
    q = (255 - np.minimum(rng.geometric(0.03, size=n) - 1, 255)).astype(np.uint8)
    right = rng.random(n) < 0.5 + 0.5 * (q / 255.0) ** 2
    g = np.where(right, k, (k + 1 + rng.integers(0, C - 1, size=n)) % C).astype(np.uint8)
    g[rng.random(n) < 0.05] = 255
    return k, q, g
