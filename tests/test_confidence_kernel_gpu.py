"""fs_bilinear_argmax_conf and fs_score_confidence against the host reference of tests/_confidence_ref.py (fp64, per-pixel bound derived
there), for the three storage types on the x8 strip path and the generic path: the confidence byte at every pixel, the class map bit for
bit fs_bilinear_argmax's when nothing is masked, the mask exactly `q >= min_conf`, either output alone, pad lanes that hold junk larger
than any logit, logits that overflow exp without the max subtraction."""
import numpy as np
import pytest
import torch

from tests import _confidence_ref as CR

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16", "fp16")
GUARD = 64


def _view(buf, C, dtype):
    """NHWC logits view (N, C, Hi, Wi) over the whole padded buffer on the device"""
    t = torch.from_numpy(buf).to(CR.TORCH[dtype]).cuda()
    assert torch.equal(t.float().cpu(), torch.from_numpy(buf))            # the stored values are the reference's
    return t.permute(0, 3, 1, 2)[:, :C]


def _guarded(shape):
    """a uint8 map inside a sentinel-filled buffer: (map view, check that nothing outside it was written)"""
    n = int(np.prod(shape))
    pad = -n % 16
    buf = torch.full((GUARD + n + pad + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def intact():
        return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all())
    return buf[GUARD:GUARD + n].view(shape), intact


def _run(x, size, **kw):
    from fasterseg_amd import kernels as K
    N = x.shape[0]
    classes, c_ok = _guarded((N,) + tuple(size))
    conf, q_ok = _guarded((N,) + tuple(size))
    K.bilinear_argmax_conf(x, size, classes=classes, conf=conf, **kw)
    torch.cuda.synchronize()
    assert c_ok() and q_ok(), "a store outside the maps"
    return classes, conf


def _check_case(case, dtype, scale=2.0):
    from fasterseg_amd import kernels as K
    buf, C = CR.logits(case, dtype, scale=scale)
    size = CR.CASES[case][4]
    ref = CR.reference(buf, C, size)
    x = _view(buf, C, dtype)
    classes, conf = _run(x, size)
    q = conf.cpu().numpy()
    err = np.abs(q.astype(np.float64) - ref["t"])
    print("%s %s x%g: max |q - t| = %.4f (bound %.4f, 255 eps %.4f), M %.1f A %.1f, q in %d..%d" % (
        case, dtype, scale, err.max(), ref["tol"], 255 * ref["eps"], ref["M"], ref["A"], q.min(), q.max()))
    bad = CR.failures(q, ref)
    assert not bad.any(), "%d of %d confidence bytes outside the bound" % (bad.sum(), bad.size)
    want = K.bilinear_argmax(x, size)
    assert torch.equal(classes, want), "%d class-map pixels differ from fs_bilinear_argmax" % int((classes != want).sum())
    return x, size, classes.clone(), conf.clone(), q


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CR.CASES))
def test_confidence_and_classes(case, dtype):
    x, size, classes, conf, q = _check_case(case, dtype)
    C = CR.CASES[case][1]
    if C == 1:
        assert (q == 255).all() and int(classes.max()) == 0
    # the mask: exactly q >= min_conf, and the confidence map is unchanged by it
    for min_conf, ignore in ((128, 255), (230, 255), (128, 254)):
        masked, conf2 = _run(x, size, min_confidence=min_conf / 255, ignore_label=ignore)
        keep = conf >= min_conf
        assert torch.equal(masked, torch.where(keep, classes, torch.full_like(classes, ignore))), (min_conf, ignore)
        assert torch.equal(conf2, conf)
    # either output alone
    from fasterseg_amd import kernels as K
    only_c, none = K.bilinear_argmax_conf(x, size, min_confidence=128 / 255, conf=False)
    none2, only_q = K.bilinear_argmax_conf(x, size, min_confidence=128 / 255, classes=False)
    assert none is None and none2 is None
    assert torch.equal(only_c, torch.where(conf >= 128, classes, torch.full_like(classes, 255))) and torch.equal(only_q, conf)


@pytest.mark.parametrize("dtype", DTYPES)
def test_logits_that_overflow_exp(dtype):
    _, _, _, _, q = _check_case("x8-two-images", dtype, scale=30.0)
    assert q.max() == 255


@pytest.mark.parametrize("C,cs", [(19, 20), (19, 32), (3, 4)])
@pytest.mark.parametrize("pixels", [1, 255, 4096 + 3])
def test_score_confidence(pixels, C, cs):
    from fasterseg_amd import kernels as K
    rng = np.random.default_rng(pixels * 100 + cs)
    score = np.full((pixels, cs), 1e30, dtype=np.float32)
    score[:, :C] = np.exp(2.0 * rng.standard_normal((pixels, C))).astype(np.float32)
    if pixels > 4:
        score[1, :C] = 0.0                               # a row of zeros
        score[2, min(1, C - 1)] = np.inf                 # a row with an inf
        score[3, :C] = score[3, 0]                       # exact ties over the whole row: the lowest index wins
        score[4, C - 1] = score[4, :C].max()             # ... and a two-way tie of the maximum
    t, tol, cls = CR.score_reference(score, C)
    dev = torch.from_numpy(score).cuda()
    classes, c_ok = _guarded((pixels,))
    conf, q_ok = _guarded((pixels,))
    K.score_confidence(dev, C, classes=classes, conf=conf)
    torch.cuda.synchronize()
    assert c_ok() and q_ok()
    q = conf.cpu().numpy().astype(np.float64)
    bad = np.abs(q - t) > tol
    print("score %d x %d/%d: max |q - t| = %.4f" % (pixels, C, cs, np.abs(q - t).max()))
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8])
    assert torch.equal(classes.cpu(), torch.argmax(torch.from_numpy(score[:, :C]), dim=1).to(torch.uint8))
    assert (classes.cpu().numpy() == cls).all()
    if pixels > 4:
        assert q[1] == 0 and q[2] == 0 and int(classes[3]) == 0 and int(classes[2]) == min(1, C - 1)
    masked, conf2 = K.score_confidence(dev, C, min_confidence=128 / 255, ignore_label=254)
    assert torch.equal(conf2, conf) and torch.equal(masked, torch.where(conf >= 128, classes, torch.full_like(classes, 254)))
    only_c, _ = K.score_confidence(dev, C, min_confidence=128 / 255, ignore_label=254, conf=False)
    _, only_q = K.score_confidence(dev, C, classes=False)
    assert torch.equal(only_c, masked) and torch.equal(only_q, conf)
