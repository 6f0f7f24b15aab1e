"""fs_confidence_hist against the numpy histogram of tests/_class_threshold_ref.hist_numpy, exactly: sizes below, at and past one lane's
run of 16 pixels and one block's share, 1 / 19 / 32 classes (32 with labels claims a block's whole 64 KB of LDS), no labels and uint8 /
int32 / int64 labels with their ignore values, class bytes >= C (skipped), maps that start at byte offsets 0, 1 and 3 - each map at its
own - and a 2^20-pixel map with every pixel in one bin.  `hist` sits between guard words; plane 1 is pre-filled with a sentinel and must
keep it when no labels are given; a second call without zeroing accumulates."""
import numpy as np
import pytest
import torch

from tests import _class_threshold_ref as TR

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = 0x5A5A5A5A5A5A5A5A
OFFSETS = ((0, 0), (1, 3), (3, 1))          # byte offsets of (classes, conf) inside their buffers
ONE_BIN = 1 << 20


def _maps(n, C, one_bin):
    rng = np.random.default_rng(n * 64 + C)
    if one_bin:
        k = np.full(n, min(2, C - 1), dtype=np.uint8)
        q = np.full(n, 255, dtype=np.uint8)
        g = k.astype(np.int64)
    else:
        # runs of equal keys next to isolated ones, as a class map has; some class bytes are C itself and 255 (masked pixels)
        k = np.repeat(rng.integers(0, C, size=n), rng.integers(1, 6, size=n))[:n].astype(np.uint8)
        q = np.where(rng.random(n) < 0.6, 255, rng.integers(0, 256, size=n)).astype(np.uint8)
        k[rng.random(n) < 0.05] = 255
        k[rng.random(n) < 0.05] = C
        g = np.where(rng.random(n) < 0.7, k.astype(np.int64), rng.integers(0, C, size=n))
        g[g >= C] = rng.integers(0, C, size=int((g >= C).sum()))
    return k, q, g, rng


def _labels(kind, g, C, rng):
    """(device labels, numpy labels as int64) with the kind's own ignore values sprinkled in"""
    n = g.size
    drop = rng.random(n) < 0.1
    if kind == "uint8":
        lab = np.where(drop, 255, g).astype(np.uint8)
    elif kind == "int32":
        lab = np.where(drop, -1, g).astype(np.int32)
    else:
        lab = np.where(drop, rng.choice([C, C + 1, 255, 1 << 40, -1, -(1 << 40)], size=n), g).astype(np.int64)
    return torch.from_numpy(lab).cuda(), lab.astype(np.int64)


def _guarded_hist(C, plane1=0):
    buf = torch.full((GUARD + 2 * C * 256 + GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    hist = buf[GUARD:GUARD + 2 * C * 256].view(2, C, 256)
    hist[0].zero_()
    hist[1].fill_(plane1)

    def intact():
        return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + 2 * C * 256:] == SENTINEL).all())
    return hist, intact


def _at(a, offset):
    """the array on the device, starting `offset` bytes into its allocation"""
    buf = torch.zeros(a.size + 16, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == offset and view.is_contiguous()
    return view


@pytest.mark.parametrize("C", [1, 19, 32])
@pytest.mark.parametrize("n", [1, 255, 4099, 3 * 4096 + 5, ONE_BIN], ids=["1", "255", "4099", "12293", "one-bin-2^20"])
def test_confidence_hist(n, C):
    from fasterseg_amd import kernels as K
    k, q, g, rng = _maps(n, C, n == ONE_BIN)
    want = TR.hist_numpy(k, q, C)
    assert want[1].sum() == 0 and want.sum() == int((k < C).sum())
    if n == ONE_BIN:
        assert (want > 0).sum() == 1 and want.max() == n
    views = [(_at(k, oc), _at(q, oq)) for oc, oq in OFFSETS]
    # without labels: plane 0 only, plane 1 keeps whatever it held
    for kd, qd in views:
        hist, intact = _guarded_hist(C, plane1=SENTINEL)
        assert K.confidence_hist(kd, qd, C, hist=hist) is hist
        torch.cuda.synchronize()
        assert intact(), "a write outside hist"
        assert (hist[1] == SENTINEL).all(), "plane 1 was touched without labels"
        got = hist[0].cpu().numpy()
        assert (got == want[0]).all(), (int((got != want[0]).sum()), int(got.sum()), int(want[0].sum()))
    # a second call without zeroing accumulates; a fresh accumulator is created zeroed
    K.confidence_hist(views[1][0], views[1][1], C, hist=hist)
    assert (hist[0].cpu().numpy() == 2 * want[0]).all() and (hist[1] == SENTINEL).all() and intact()
    assert (K.confidence_hist(views[0][0], views[0][1], C).cpu().numpy() == want).all()
    # with labels of each type
    for kind in ("uint8", "int32", "int64"):
        lab, lab_np = _labels(kind, g, C, rng)
        want_l = TR.hist_numpy(k, q, C, lab_np)
        assert want_l.sum() == int(((k < C) & (lab_np >= 0) & (lab_np < C)).sum())
        if n >= 255 and C > 1 and n != ONE_BIN:
            assert want_l[0].sum() > 0 and want_l[1].sum() > 0 and want_l.sum() < want.sum()
        for kd, qd in views:
            hist, intact = _guarded_hist(C)
            K.confidence_hist(kd, qd, C, gt=lab, hist=hist)
            torch.cuda.synchronize()
            assert intact(), "a write outside hist"
            got = hist.cpu().numpy()
            assert (got == want_l).all(), (kind, int((got != want_l).sum()), int(got.sum()), int(want_l.sum()))
        K.confidence_hist(views[2][0], views[2][1], C, gt=lab, hist=hist)
        assert (hist.cpu().numpy() == 2 * want_l).all() and intact()


def test_confidence_histogram_accumulator():
    """calibration.ConfidenceHistogram over three maps of different sizes equals the histogram of their concatenation; 2-D maps"""
    from fasterseg_amd import calibration as CAL
    C = 19
    acc = CAL.ConfidenceHistogram(C, "cuda")
    acc_l = CAL.ConfidenceHistogram(C, "cuda")
    ks, qs, gs = [], [], []
    for shape in ((7, 33), (64, 96), (1, 5)):
        n = shape[0] * shape[1]
        k, q, g, _ = _maps(n, C, False)
        g = g.astype(np.uint8)
        ks.append(k), qs.append(q), gs.append(g)
        kd, qd, gd = (torch.from_numpy(a.reshape(shape)).cuda() for a in (k, q, g))
        acc.add(kd, qd)
        acc_l.add(kd, qd, gd)
    k, q, g = (np.concatenate(a) for a in (ks, qs, gs))
    got = acc.result()
    assert got.dtype == np.int64 and got.shape == (2, C, 256) and (got == TR.hist_numpy(k, q, C)).all()
    assert (acc_l.result() == TR.hist_numpy(k, q, C, g)).all()
    with pytest.raises(TypeError, match="uint8, int32 or int64"):
        acc.add(kd, qd, gd.to(torch.int16))
