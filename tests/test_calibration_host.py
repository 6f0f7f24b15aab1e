"""fasterseg_amd.calibration on the host: the threshold functions against the brute-force pickers of tests/_class_threshold_ref.py, which
work on the pixels themselves.  About 50 000 skewed pixels, 19 classes, two of them absent and one with a single pixel.  Every
comparison of a threshold or a count is exact; the float curves of reliability() - arrays for plotting that decide nothing - are
multiplied back to the integers they came from."""
import fractions
import math

import numpy as np
import pytest

from tests import _class_threshold_ref as TR

C = 19
ABSENT, SINGLE = (5, 11), 7
_cache = {}


def _maps():
    if "maps" not in _cache:
        k, q, g = TR.skewed_maps(50000, C, seed=3, absent=ABSENT, single=SINGLE)
        _cache["maps"] = (k, q, g, TR.hist_numpy(k, q, C), TR.hist_numpy(k, q, C, g))
    return _cache["maps"]


def test_the_maps_are_what_the_tests_need():
    k, q, g, h, hl = _maps()
    n = np.bincount(k, minlength=C)
    assert all(n[c] == 0 for c in ABSENT) and n[SINGLE] == 1 and (n > 0).sum() == C - len(ABSENT)
    assert h[1].sum() == 0 and h[0].sum() == k.size
    assert hl.sum() == int((g < C).sum()) and hl[0].sum() > hl[1].sum() > 0
    assert n.max() > 20 * np.sort(n[n > 1])[0] and len(np.unique(q)) > 100          # skewed classes, many bytes


@pytest.mark.parametrize("portion", [0.05, 0.2, 0.5, 1.0])
@pytest.mark.parametrize("labelled", [False, True], ids=["plane0", "both-planes"])
def test_class_balanced_thresholds(portion, labelled):
    from fasterseg_amd import calibration as CAL
    k, q, g, h, hl = _maps()
    if labelled:                                        # h = hist[0] + hist[1]: the split by right / wrong must not matter
        use = g < C
        k, q, hist = k[use], q[use], hl
    else:
        hist = h
    t = CAL.class_balanced_thresholds(hist, portion)
    assert t.dtype == np.uint8 and t.shape == (C,)
    assert (t == TR.balanced_brute(k, q, C, portion)).all()
    p = TR.exact(portion)
    for c in range(C):
        mine = q[k == c]
        if mine.size == 0:
            assert t[c] == 255
            continue
        need = math.ceil(p * int(mine.size))
        assert int((mine >= t[c]).sum()) >= need
        assert int((mine >= int(t[c]) + 1).sum()) < need        # one byte higher keeps fewer than the share
    if portion == 1.0:
        assert all(t[c] == q[k == c].min() for c in range(C) if (k == c).any())


def test_floor_and_cap_clamp():
    from fasterseg_amd import calibration as CAL
    from fasterseg_amd import kernels as K
    k, q, g, h, _ = _maps()
    free = CAL.class_balanced_thresholds(h, 0.5)
    lo, hi = 0.92, 0.97
    blo, bhi = K.confidence_threshold(lo), K.confidence_threshold(hi)
    t = CAL.class_balanced_thresholds(h, 0.5, floor=lo, cap=hi)
    assert (t == np.clip(free, blo, bhi)).all() and (t == TR.balanced_brute(k, q, C, 0.5, lo, hi)).all()
    assert (free < blo).any() and (free > bhi).any(), "the clamp is not exercised on both sides"
    assert all(t[c] == bhi for c in ABSENT) and all(free[c] == 255 for c in ABSENT)
    assert (CAL.class_balanced_thresholds(np.zeros_like(h), 0.3, cap=0.5) == 128).all()      # nothing seen: the cap everywhere
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), None, "half"):
        with pytest.raises(ValueError, match="portion"):
            CAL.class_balanced_thresholds(h, bad)
    for bad in (np.zeros((C, 256), dtype=np.int64), np.zeros((2, C, 255), dtype=np.int64), np.zeros((2, C, 256))):
        with pytest.raises(ValueError, match="hist"):
            CAL.class_balanced_thresholds(bad, 0.5)


def test_the_share_is_an_exact_rational():
    """0.1 as a double is above 1/10: ceil(0.1 * 10) in floats of the double's exact value would be 2.  With n_k = 10 distinct bytes and
    portion 0.1 the class keeps exactly one pixel."""
    from fasterseg_amd import calibration as CAL
    h = np.zeros((2, 1, 256), dtype=np.int64)
    h[0, 0, 100:110] = 1
    assert fractions.Fraction(0.1) > fractions.Fraction(1, 10)
    assert CAL.class_balanced_thresholds(h, 0.1)[0] == 109
    assert CAL.class_balanced_thresholds(h, 0.3)[0] == 107
    assert CAL.class_balanced_thresholds(h, 1 / 3)[0] == 106         # ceil(10 / 3) = 4
    # counts beyond 2^53: the integers stay exact
    big = np.zeros((2, 1, 256), dtype=np.int64)
    big[0, 0, 200], big[0, 0, 100] = 2 ** 60 + 1, 2 ** 60
    assert CAL.class_balanced_thresholds(big, 0.5)[0] == 200          # need = 2^60 + 1 of 2^61 + 1; a double product cannot tell it from 2^60
    big[0, 0, 200] -= 1
    assert CAL.class_balanced_thresholds(big, 0.5)[0] == 200          # need = 2^60 of 2^61
    big[0, 0, 200] -= 1
    big[0, 0, 100] += 2
    assert CAL.class_balanced_thresholds(big, 0.5)[0] == 100          # 2^60 - 1 at the top: one short


@pytest.mark.parametrize("precision", [0.5, 0.8, 0.9, 0.97, 1.0])
def test_precision_thresholds(precision):
    from fasterseg_amd import calibration as CAL
    k, q, g, _, hl = _maps()
    t = CAL.precision_thresholds(hl, precision)
    want = TR.precision_brute(k, q, g, C, precision)
    assert t.dtype == np.uint8 and (t == want).all(), (t, want)
    assert all(t[c] == 255 for c in ABSENT)
    p = TR.exact(precision)
    for c in range(C):
        right, wrong = int(hl[0, c, t[c]:].sum()), int(hl[1, c, t[c]:].sum())
        if right + wrong and fractions.Fraction(right, right + wrong) >= p:
            for lower in range(int(t[c])):              # no smaller byte qualifies
                r, w = int(hl[0, c, lower:].sum()), int(hl[1, c, lower:].sum())
                assert fractions.Fraction(r, r + w) < p


def test_precision_never_reached_and_cap():
    from fasterseg_amd import calibration as CAL
    h = np.zeros((2, 3, 256), dtype=np.int64)
    h[0, 0, 255], h[1, 0, 255] = 8, 2                   # class 0: 80 % right even at the top byte
    h[0, 1, 250], h[1, 1, 10] = 9, 1                    # class 1: 90 % from byte 0, 100 % from byte 11
    t = CAL.precision_thresholds(h, 0.9)
    assert list(t) == [255, 0, 255]                     # never reached: the cap; reached at once; no pixel: the cap
    assert list(CAL.precision_thresholds(h, 0.95)) == [255, 11, 255]
    assert list(CAL.precision_thresholds(h, 0.8)) == [0, 0, 255]
    assert list(CAL.precision_thresholds(h, 0.95, cap=200 / 255)) == [200, 11, 200]
    assert list(CAL.precision_thresholds(h, 0.0)) == [0, 0, 255]
    for bad in (-0.1, 1.5, float("nan"), None):
        with pytest.raises(ValueError, match="precision"):
            CAL.precision_thresholds(h, bad)


def test_reliability_sums_back_to_the_histogram():
    from fasterseg_amd import calibration as CAL
    _, _, _, _, hl = _maps()
    r = CAL.reliability(hl)
    assert r["count"].shape == (C + 1, 256) and r["count"].dtype == np.int64
    assert (r["count"][:C] == hl[0] + hl[1]).all() and (r["count"][C] == hl.sum(axis=(0, 1))).all()
    assert (r["right"][:C] == hl[0]).all() and (r["right"][C] == hl[0].sum(axis=0)).all()
    n = r["count"].sum(axis=1)
    present = n > 0
    assert (r["kept"][present, 0] == 1.0).all() and np.isnan(r["kept"][~present]).all()
    # kept and precision are the tail sums over the row totals: multiplied back they are the integers
    tails = np.cumsum(r["count"][:, ::-1], axis=1)[:, ::-1]
    assert (np.rint(r["kept"][present] * n[present, None]) == tails[present]).all()
    rt = np.cumsum(r["right"][:, ::-1], axis=1)[:, ::-1]
    some = tails > 0
    assert (np.rint(r["precision"][some] * tails[some]) == rt[some]).all() and np.isnan(r["precision"][~some]).all()
    assert (np.diff(r["kept"][present], axis=1) <= 0).all()
    # the calibration error, restated bin by bin
    for row in (0, 2, C):
        cnt, rgt = r["count"][row].astype(np.float64), r["right"][row].astype(np.float64)
        ece = sum(cnt[b] / cnt.sum() * abs(rgt[b] / cnt[b] - b / 255.0) for b in range(256) if cnt[b])
        assert abs(r["ece"][row] - ece) < 1e-12 and 0.0 < r["ece"][row] < 1.0
