"""The host reference of the confidence byte (tests/_confidence_ref.py) on its own, without a device: it accepts the contract evaluated
in numpy float32 at every pixel of every case, and it rejects the mistakes a kernel could make - a truncating quantiser, a scale of 256,
a softmax over bf16-rounded values, pad lanes in the sum, no max subtraction on logits that overflow exp."""
import numpy as np
import pytest

from tests import _confidence_ref as CR

DTYPES = ("fp32", "bf16", "fp16")


def _size(case):
    return CR.CASES[case][4]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CR.CASES))
def test_reference_accepts_the_fp32_contract(case, dtype):
    buf, C = CR.logits(case, dtype)
    ref = CR.reference(buf, C, _size(case))
    q = CR.fp32_bytes(buf, C, _size(case))
    bad = CR.failures(q, ref)
    assert not bad.any(), "%d of %d pixels outside the bound (255 eps = %.4f)" % (bad.sum(), bad.size, 255 * ref["eps"])
    assert 255 * ref["eps"] <= 0.03                    # the bound decides the byte except next to a half-integer
    if C == 1:
        assert (q == 255).all()
    elif C == 19 and q.size >= 4096:
        assert q.min() < 0.25 * 255 and q.max() > 0.75 * 255          # the confidences span the range


def test_reference_accepts_the_overflowing_case():
    buf, C = CR.logits("x8-two-images", "fp32", scale=30.0)
    ref = CR.reference(buf, C, _size("x8-two-images"))
    q = CR.fp32_bytes(buf, C, _size("x8-two-images"))
    assert not CR.failures(q, ref).any() and q.max() == 255 and 255 * ref["eps"] <= 0.03
    assert np.abs(buf[..., :C]).max() > 89.0           # exp overflows fp32 without the max subtraction


@pytest.mark.parametrize("mistake,kw,least,most", [
    ("truncation", dict(truncate=True), 0.35, 0.65),
    ("scale-256", dict(scale=256.0), 0.15, 0.5),
    ("bf16-softmax", dict(soft_dtype="bf16"), 0.03, 0.4),
    ("pads-in-the-sum", dict(with_pads=True), 0.9, 1.0),
])
def test_reference_rejects(mistake, kw, least, most):
    for case in ("x8-two-images", "generic-ratio"):
        if mistake == "pads-in-the-sum" and CR.CASES[case][1] == CR.CASES[case][2]:
            continue
        buf, C = CR.logits(case, "fp32")
        ref = CR.reference(buf, C, _size(case))
        share = CR.failures(CR.fp32_bytes(buf, C, _size(case), **kw), ref).mean()
        assert least <= share <= most, "%s on %s: %.3f of the pixels fail" % (mistake, case, share)


def test_reference_rejects_no_max_subtraction_where_exp_overflows():
    buf, C = CR.logits("x8-two-images", "fp32", scale=30.0)
    ref = CR.reference(buf, C, _size("x8-two-images"))
    bad = CR.failures(CR.fp32_bytes(buf, C, _size("x8-two-images"), subtract_max=False), ref)
    over = ref["vmax"] > 89.0                          # exp(v_max) is inf in fp32: inf / inf, whatever the true share
    assert over.any() and bad[over].all(), (int(over.sum()), int(bad[over].sum()))


def test_score_reference():
    score = np.array([[1.0, 3.0, 0.0, 1e30], [0.0, 0.0, 0.0, 1e30], [np.inf, 1.0, 2.0, 1e30], [2.0, 2.0, 1.0, 1e30]], dtype=np.float32)
    t, tol, cls = CR.score_reference(score, 3)
    assert np.allclose(t, [255 * 0.75, 0.0, 0.0, 255 * 0.4]) and list(cls) == [1, 0, 0, 0]
    assert (tol >= 0.5).all() and (tol < 0.5001).all()
