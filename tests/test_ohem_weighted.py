"""Class-weighted OHEM criterion on the CPU: fasterseg_amd.losses.ProbOhemCrossEntropy2d(weight=...) against the values the
reference's own ProbOhemCrossEntropy2d(use_weight=True) produced (tests/golden/loss_weighted.npz, tools/make_loss_weighted_golden.py)."""
import numpy as np
import pytest
import torch

from fasterseg_amd.losses import ProbOhemCrossEntropy2d
from tests._util import load_npz


def test_weighted_ohem_matches_reference_fixture():
    """Bars of the unweighted fixture's GPU test (tests/test_losses_gpu.py): loss 1e-5, gradient 2e-6."""
    store = load_npz("loss_weighted.npz")
    weight = store["weight"]
    assert weight.shape == (19,)
    for i in range(4):
        pred = torch.tensor(store["ohem%d/pred" % i].astype(np.float32)).requires_grad_(True)
        target = torch.tensor(store["ohem%d/target" % i].astype(np.int64))
        thresh, min_kept = store["ohem%d/cfg" % i]
        crit = ProbOhemCrossEntropy2d(255, thresh=float(thresh), min_kept=int(min_kept), use_weight=True, weight=weight)
        loss = crit(pred, target)
        loss.backward()
        assert abs(float(loss.detach()) - float(store["ohem%d/loss" % i][0])) < 1e-5, i
        np.testing.assert_allclose(pred.grad.numpy(), store["ohem%d/grad" % i], atol=2e-6)


def test_use_weight_without_weight_names_the_argument():
    with pytest.raises(ValueError, match="weight"):
        ProbOhemCrossEntropy2d(255, use_weight=True)


@pytest.mark.parametrize("use_weight", [True, False], ids=["use_weight", "weight_only"])
def test_unit_weights_equal_the_unweighted_criterion(use_weight):
    g = torch.Generator().manual_seed(11)
    pred = (torch.randn(2, 19, 12, 20, generator=g) * 2.0)
    target = torch.randint(0, 19, (2, 12, 20), generator=g)
    target[torch.rand(2, 12, 20, generator=g) < 0.1] = 255
    a = pred.clone().requires_grad_(True)
    b = pred.clone().requires_grad_(True)
    plain = ProbOhemCrossEntropy2d(255, thresh=0.3, min_kept=40)(a, target)
    ones = ProbOhemCrossEntropy2d(255, thresh=0.3, min_kept=40, use_weight=use_weight, weight=torch.ones(19))(b, target)
    plain.backward()
    ones.backward()
    assert abs(float(plain.detach()) - float(ones.detach())) <= 1e-6
    assert float((a.grad - b.grad).abs().max()) <= 1e-6


def test_weight_changes_the_loss_and_a_sequence_is_accepted():
    """A weight given with use_weight=False is honoured: weighted mean = sum w nll / sum w over the kept pixels."""
    g = torch.Generator().manual_seed(12)
    pred = torch.randn(1, 5, 6, 7, generator=g) * 2.0
    target = torch.randint(0, 5, (1, 6, 7), generator=g)
    w = [0.5, 1.0, 1.5, 2.0, 0.25]
    got = ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=0, weight=w)(pred, target)
    nll = torch.nn.functional.cross_entropy(pred.double(), target, reduction="none").reshape(-1)
    wt = torch.tensor(w, dtype=torch.float64)[target.reshape(-1)]
    want = float((wt * nll).sum() / wt.sum())
    assert abs(float(got) - want) <= 1e-5 * abs(want)
    assert abs(float(got) - float(ProbOhemCrossEntropy2d(255, thresh=0.7, min_kept=0)(pred, target))) > 1e-3
