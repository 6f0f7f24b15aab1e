"""Self-test of tests/_loss_ref.py (the fp64 reference the GPU loss and class-map tests compare against): in double it reproduces the
CPU op chains of fasterseg_amd.losses, which tests/test_losses.py pins to the reference's fixtures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _loss_ref as R
from tests._util import load_npz


@pytest.mark.parametrize("i", range(4))
def test_ohem_reference_reproduces_cpu_criterion_on_fixture(i):
    from fasterseg_amd.losses import ProbOhemCrossEntropy2d
    store = load_npz("loss.npz")
    pred = torch.tensor(store["ohem%d/pred" % i]).double()
    target = torch.tensor(store["ohem%d/target" % i])
    thresh, min_kept = float(store["ohem%d/cfg" % i][0]), int(store["ohem%d/cfg" % i][1])
    x = pred.clone().requires_grad_(True)
    want = ProbOhemCrossEntropy2d(255, thresh=thresh, min_kept=min_kept)(x, target)          # CPU path, double
    want.backward()
    loss, coef = R.ohem_criterion(pred, target, thresh, min_kept)
    assert abs(float(loss) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert abs(float(loss) - float(store["ohem%d/loss" % i][0])) < 1e-5                      # and the reference's own fp32 value
    grad = R.ohem_grad(pred, None, target, coef, 1.0 / float(coef.sum()))
    assert float((grad - x.grad).abs().max()) <= 1e-12
    np.testing.assert_allclose(grad.numpy(), store["ohem%d/grad" % i], atol=2e-6)


def test_ohem_reference_vectors_and_label_rule():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 5, 3, 4, generator=g).double()
    t = torch.randint(0, 5, (2, 3, 4), generator=g)
    t[0, 0, 0], t[0, 0, 1], t[0, 0, 2], t[0, 0, 3], t[1, 0, 0] = 255, -1, 5, 254, 2 ** 32 + 3
    tp, nll, lse, valid = R.ohem_vectors(x, t)
    assert int(valid.sum()) == 24 - 5
    assert bool((tp[~valid] == 1).all()) and bool((nll[~valid] == 0).all())
    logp = torch.log_softmax(x, 1).permute(0, 2, 3, 1).reshape(-1, 5)
    idx = torch.nonzero(valid).squeeze(1)
    assert torch.allclose(nll[idx], -logp[idx, t.reshape(-1)[idx]], rtol=0, atol=1e-14)
    assert torch.allclose(tp, torch.exp(-nll), rtol=0, atol=1e-14) and torch.allclose(lse, torch.logsumexp(x, 1).reshape(-1))
    # the gradient of a not-valid pixel is zero whatever its coefficient
    grad = R.ohem_grad(x, None, t, torch.ones(24), 1.0)
    assert float(grad[0, :, 0, :].abs().max()) == 0 and float(grad[1, :, 0, 0].abs().max()) == 0 and float(grad[1, :, 1, 1].abs().max()) > 0


def test_kl_reference_reproduces_distill_kl():
    from fasterseg_amd.losses import distill_kl
    g = torch.Generator().manual_seed(2)
    s = (torch.randn(2, 7, 5, 6, generator=g) * 2).double()
    t = (torch.randn(2, 7, 5, 6, generator=g) * 3).double()
    x = s.clone().requires_grad_(True)
    want = distill_kl(x, t)
    want.backward()
    kl, ls, lt = R.kl_vectors(s, t)
    n = s.numel()
    assert abs(float(kl.sum() / n) - float(want)) <= 1e-14
    assert float((R.kl_grad(s, t, None, 1.0 / n) - x.grad).abs().max()) <= 1e-15
    # through the up-sample, and a teacher class at -inf: the xlogy convention keeps value and gradient finite
    lo = s[:, :, :2, :3]
    up = lambda v: F.interpolate(v, size=(5, 6), mode="bilinear", align_corners=True)
    tl = t[:, :, :2, :3]
    x2 = lo.clone().requires_grad_(True)
    distill_kl(up(x2), up(tl)).backward()
    assert float((R.kl_grad(lo, tl, (5, 6), 1.0 / n) - x2.grad).abs().max()) <= 1e-15
    t2 = t.clone()
    t2[:, 3, ::2, ::2] = float("-inf")
    kl2 = R.kl_vectors(s, t2)[0]
    assert bool(torch.isfinite(kl2).all()) and bool(torch.isfinite(R.kl_grad(s, t2, None, 1.0)).all())
    assert abs(float(kl2.sum() / n) - float(distill_kl(s, t2))) <= 1e-14


def test_class_map_reference():
    lo = torch.tensor([[[[0.0, 1.0]], [[1.0, 0.0]], [[0.5, 0.5]]]])          # (1, 3, 1, 2): classes cross in the middle
    up, arg, gap = R.class_map(lo, (1, 5))
    assert arg.tolist() == [[[1, 1, 0, 0, 0]]]                               # the three-way tie in the middle goes to class 0
    assert gap[0, 0, 2] == 0 and gap[0, 0, 0] == 0.5
    assert R.check_class_map(arg, up, arg, gap) == 0.8
    other = arg.clone()
    other[0, 0, 2] = 2                                                        # another member of the tie passes, a clear miss does not
    R.check_class_map(other, up, arg, gap)
    other[0, 0, 0] = 0
    with pytest.raises(AssertionError):
        R.check_class_map(other, up, arg, gap)
    hist, labeled, correct = R.hist_info(3, np.array([0, 1, 2, 1]), np.array([0, 1, 255, 2]))
    assert labeled == 3 and correct == 2 and hist[2, 1] == 1 and hist.sum() == 3
