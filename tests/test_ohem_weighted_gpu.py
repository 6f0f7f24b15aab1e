"""Class-weighted OHEM criterion on the device (fs_ohem_ce[_up]_fwd + fs_ohem_select + fs_ohem_ce[_up]_bwd_coef) against the CPU op
chain of fasterseg_amd.losses.ProbOhemCrossEntropy2d(weight=...), itself pinned to the reference fixture in tests/test_ohem_weighted.py.
Cases and bars are those of tests/test_losses_gpu.py for the unweighted criterion."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _seeded_weight(C, seed=41):
    return torch.rand(C, generator=torch.Generator().manual_seed(seed)) + 0.5          # in [0.5, 1.5]


@pytest.mark.parametrize("case", [
    dict(shape=(2, 19, 32, 48), thresh=0.7, min_kept=2 * 32 * 48 // 16, ignore_frac=0.05),      # k-th value above thresh or not
    dict(shape=(3, 19, 17, 23), thresh=0.05, min_kept=400, ignore_frac=0.1),                    # k-th smallest decides
    dict(shape=(1, 19, 16, 16), thresh=0.7, min_kept=10 ** 6, ignore_frac=0.0),                 # fewer valid than min_kept: no OHEM
    dict(shape=(2, 7, 20, 20), thresh=0.9, min_kept=0, ignore_frac=0.5),                        # threshold only
], ids=["typical", "kth", "not_enough_valid", "thresh_only"])
def test_weighted_ohem_matches_torch_chain(case):
    from fasterseg_amd.losses import ProbOhemCrossEntropy2d
    g = torch.Generator().manual_seed(5)
    B, C, H, W = case["shape"]
    pred = (torch.randn(B, C, H, W, generator=g) * 2.0).requires_grad_(True)
    target = torch.randint(0, C, (B, H, W), generator=g)
    target[torch.rand(B, H, W, generator=g) < case["ignore_frac"]] = 255
    crit = ProbOhemCrossEntropy2d(ignore_label=255, thresh=case["thresh"], min_kept=case["min_kept"], use_weight=True, weight=_seeded_weight(C))
    ref = crit(pred, target)
    ref.backward()
    pred_d = pred.detach().cuda().requires_grad_(True)
    got = crit(pred_d, target.cuda())
    assert type(got.grad_fn).__name__ == "_OhemCEWBackward"
    got.backward()
    print("weighted loss", float(got), "cpu chain", float(ref))
    assert abs(float(got) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (float(got), float(ref))
    err = float((pred_d.grad.cpu() - pred.grad).abs().max())
    assert err <= 1e-6 + 1e-4 * float(pred.grad.abs().max()), err
    # scaled upstream gradient and a non-contiguous prediction
    pred_t = pred.detach().cuda().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    (crit(pred_t, target.cuda()) * 0.2).backward()
    assert float((pred_t.grad.cpu() - 0.2 * pred.grad).abs().max()) <= 1e-6 + 1e-4 * float(pred.grad.abs().max())
    # and the weight matters: the unweighted criterion gives another loss
    plain = ProbOhemCrossEntropy2d(ignore_label=255, thresh=case["thresh"], min_kept=case["min_kept"])(pred.detach().cuda(), target.cuda())
    assert abs(float(plain) - float(got)) > 1e-4 * abs(float(got))


def _lowres_logits(shape, dtype, seed, cs=32):
    """(N, C, h, w) NHWC view with channel stride cs like a Head's classifier output, plus its fp32 value on the CPU."""
    from fasterseg_amd import kernels as K
    N, C, h, w = shape
    g = torch.Generator().manual_seed(seed)
    val = (torch.randn(N, C, h, w, generator=g) * 2.0).to(dtype).float()
    buf = K.empty_nhwc(N, C, h, w, dtype, "cuda", cs=cs, zero=True)
    buf.copy_(val.cuda().to(dtype))
    return buf, val


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", [
    dict(lo=(2, 19, 8, 12), up=8, thresh=0.7, min_kept=2 * 64 * 96 // 16, ignore_frac=0.05),
    dict(lo=(1, 19, 4, 6), up=16, thresh=0.7, min_kept=64 * 96 // 16, ignore_frac=0.1),
    dict(lo=(2, 19, 2, 3), up=32, thresh=0.2, min_kept=300, ignore_frac=0.0),
    dict(lo=(1, 19, 5, 7), up=8, thresh=0.7, min_kept=10 ** 7, ignore_frac=0.02),             # not enough valid pixels: no OHEM
], ids=["x8", "x16", "x32", "no_ohem"])
def test_weighted_ohem_from_lowres_logits_matches_upsample_then_cpu_chain(case, dtype):
    import torch.nn.functional as F
    from fasterseg_amd.losses import ProbOhemCrossEntropy2d, ohem_ce_lowres
    N, C, h, w = case["lo"]
    H, W = h * case["up"], w * case["up"]
    buf, val = _lowres_logits(case["lo"], dtype, 21)
    g = torch.Generator().manual_seed(22)
    target = torch.randint(0, C, (N, H, W), generator=g)
    target[torch.rand(N, H, W, generator=g) < case["ignore_frac"]] = 255
    crit = ProbOhemCrossEntropy2d(255, thresh=case["thresh"], min_kept=case["min_kept"], use_weight=True, weight=_seeded_weight(C))
    ref_in = val.clone().requires_grad_(True)
    ref = crit(F.interpolate(ref_in, size=(H, W), mode="bilinear", align_corners=True), target)
    ref.backward()
    x = buf.detach().requires_grad_(True)
    got = ohem_ce_lowres(crit, x, target.cuda())
    assert type(got.grad_fn).__name__ == "_OhemCEUpWBackward"
    (got * 0.5).backward()
    print("weighted lowres loss", float(got), "cpu chain", float(ref))
    assert abs(float(got) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref))), (float(got), float(ref))
    gtol = (1e-6 + 2e-4 * float(ref_in.grad.abs().max())) if dtype == torch.float32 else 1e-2 * float(ref_in.grad.abs().max())
    err = float((x.grad.float().cpu() - 0.5 * ref_in.grad).abs().max())
    assert err <= gtol, (err, gtol)
    # pad channels of the low-resolution gradient are zero: the entry point itself, into a buffer that starts as NaN
    import ctypes
    from fasterseg_amd import kernels as K
    from fasterseg_amd import losses as L
    d = L._logits_desc(buf, (H, W))
    vec = torch.empty((3, N * H * W), dtype=torch.float32, device="cuda")
    tgt = target.cuda().reshape(-1)
    K.call("fs_ohem_ce_up_fwd", K._stream(), ctypes.byref(d), K._p(buf), K._p(tgt), 255, K._p(vec[0]), K._p(vec[1]), K._p(vec[2]))
    coef, _, _ = L.ohem_select(vec[0], vec[1], tgt, C, 255, case["thresh"], case["min_kept"], weight=_seeded_weight(C))
    dx = torch.full((N, h, w, 32), float("nan"), dtype=dtype, device="cuda")
    ws = L._up_workspace(d, "cuda")
    scale = torch.ones(1, device="cuda")
    K.call("fs_ohem_ce_up_bwd_coef", K._stream(), ctypes.byref(d), K._p(buf), K._p(tgt), K._p(vec[2]), K._p(coef), K._p(scale), K._p(dx),
           K._p(ws), ws.numel() * 4)
    assert float(dx[..., C:].float().abs().max()) == 0.0 and bool(torch.isfinite(dx[..., :C].float()).all())


def test_weighted_ohem_matches_reference_fixture():
    """The HIP criterion against the reference's own use_weight=True values (tests/golden/loss_weighted.npz)."""
    import numpy as np
    from fasterseg_amd.losses import ProbOhemCrossEntropy2d, ohem_select
    from fasterseg_amd import kernels as K
    from tests._util import load_npz
    store = load_npz("loss_weighted.npz")
    weight = store["weight"]
    for i in range(4):
        pred = torch.tensor(store["ohem%d/pred" % i].astype(np.float32)).cuda().requires_grad_(True)
        target = torch.tensor(store["ohem%d/target" % i].astype(np.int64)).cuda()
        thresh, min_kept = store["ohem%d/cfg" % i]
        loss = ProbOhemCrossEntropy2d(255, thresh=float(thresh), min_kept=int(min_kept), use_weight=True, weight=weight)(pred, target)
        assert type(loss.grad_fn).__name__ == "_OhemCEWBackward"
        loss.backward()
        assert abs(float(loss.detach()) - float(store["ohem%d/loss" % i][0])) < 1e-5, i
        np.testing.assert_allclose(pred.grad.cpu().numpy(), store["ohem%d/grad" % i], atol=2e-6)
        if "ohem%d/kth" % i in store:           # the selection itself: the reference's k-th value (to fp32 rounding of the softmax) and kept count
            B, C, H, W = pred.shape
            buf = torch.empty((3, B * H * W), dtype=torch.float32, device="cuda")
            logits = pred.detach().contiguous()
            K.call("fs_ohem_ce_fwd", K._stream(), K._p(logits), K._p(target), B, C, H * W, 255, K._p(buf[0]), K._p(buf[1]), K._p(buf[2]))
            _, result, counts = ohem_select(buf[0], buf[1], target.reshape(-1), C, 255, float(thresh), int(min_kept), weight=weight)
            kth = float(store["ohem%d/kth" % i][0])
            assert abs(float(result[2]) - max(float(thresh), kth)) <= 1e-6, (i, float(result[2]), kth)
            assert int(counts[1]) == int(store["ohem%d/kept" % i][0]), i


def test_student_step_with_class_weights_fused_equals_materialised():
    """StudentDistillStep(class_weight=w): loss heads fused into the up-sample vs the up-sampled tensors - same loss, same parameters
    afterwards (bars of test_student_step_fused_loss_equals_materialised_loss) - and the weights change the loss."""
    from fasterseg_amd import train_step
    w = _seeded_weight(19)
    losses, states = [], []
    for fused in (True, False):
        torch.manual_seed(0)
        st = train_step.StudentDistillStep(2, 128, 256, fused_loss=fused, class_weight=w)
        imgs, target = train_step.synthetic_batch(2, 128, 256, 0, "cuda")
        if fused:
            weighted_before = st.loss_only(imgs, target)
        losses.append(float(st.step(imgs, target)))
        states.append({k: v.detach().float().cpu().clone() for k, v in st.student.state_dict().items()})
    print("weighted step loss fused / materialised", losses)
    assert abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[1]), losses
    worst = max(float((states[0][k] - states[1][k]).abs().max()) for k in states[0])
    assert worst <= 1e-4, worst
    assert abs(weighted_before - losses[0]) <= 1e-4 * abs(losses[0])            # loss_only's criterion carries the weight too
    torch.manual_seed(0)
    plain = train_step.StudentDistillStep(2, 128, 256, fused_loss=True)
    imgs, target = train_step.synthetic_batch(2, 128, 256, 0, "cuda")
    unweighted = float(plain.step(imgs, target))
    assert abs(unweighted - losses[0]) > 1e-4 * abs(losses[0]), (unweighted, losses[0])
