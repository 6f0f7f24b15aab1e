"""Supernet validation on MI355X (fasterseg_amd.search_eval, search/train_search.py:141-212, 259-271): fs_heads_confusion against
fs_bilinear_argmax + fs_hist_info head by head, the supernet's low-resolution eval forward, SupernetEvaluator against the reference's
five sweeps restated with the module forward, torch arg-max and numpy hist_info, a validation between graphed train steps, and an
exported architecture through the training and inference paths."""
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.seeded import seeded_input, seeded_state

pytestmark = pytest.mark.gpu

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])       # config_search.py image_mean / image_std
WML = [4. / 12, 6. / 12, 8. / 12, 10. / 12, 1.]
CFG = dict(num_classes=19, layers=6, Fch=12, width_mult_list=WML, prun_modes=['max', 'arch_ratio'],
           stem_head_width=[(1, 1), (8. / 12, 8. / 12)])


def hist_info_np(n_cl, pred, gt):
    """tools/seg_opr/metric.py:7-17."""
    k = (gt >= 0) & (gt < n_cl)
    labeled = int(np.sum(k))
    correct = int(np.sum(pred[k] == gt[k]))
    return np.bincount(n_cl * gt[k].astype(int) + pred[k].astype(int), minlength=n_cl ** 2).reshape(n_cl, n_cl), labeled, correct


def normalize(img):
    """(u / 255 - mean) / std in fp32 (SegEvaluator.process_image, img_utils.py:178-184)."""
    x = img.astype(np.float32) / np.float32(255)
    return (x - MEAN.astype(np.float32)) / STD.astype(np.float32)


# ---- the kernel -------------------------------------------------------------------------------------------------------------
def _head(N, C, h, w, cs, dtype, gen):
    from fasterseg_amd import kernels as K
    buf = torch.full((N, h, w, cs), 1e4, dtype=dtype, device="cuda")        # pad lanes must never win
    t = buf.permute(0, 3, 1, 2)[:, :C]
    t.copy_(torch.randn((N, C, h, w), generator=gen).to(dtype))
    assert K.channel_stride(t) == cs
    return t


def _labels(N, H, W, C, kind, gen):
    g = torch.randint(0, C, (N, H, W), generator=gen)
    drop = torch.rand((N, H, W), generator=gen)
    if kind == "u8":
        g[drop < 0.1] = 255
        return g.to(torch.uint8).cuda()
    g[drop < 0.05] = 255
    g[(drop >= 0.05) & (drop < 0.1)] = -1
    return g.to(torch.int64 if kind == "i64" else torch.int32).cuda()


def _per_head(head, gt):
    """fs_bilinear_argmax + fs_hist_info: the class map and the counts of one head."""
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    from fasterseg_amd.metric import HistAccumulator
    N, C, h, w = head.shape
    H, W = gt.shape[-2:]
    d = _lib.ResizeDesc(N, h, w, H, W, C, K.channel_stride(head), 0, K.dtype_code(head.dtype), 0, 0)
    classes = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
    _lib.call("fs_bilinear_argmax", K._stream(), ctypes.byref(d), K._p(head), K._p(classes))
    acc = HistAccumulator(C)
    acc.add(classes, gt.reshape(N, H, W).contiguous())
    return acc.hist, acc.counts


CASES = [   # K, N, (h, w), (H, W), C, channel strides, labels
    (1, 2, (9, 13), (72, 104), 19, [32], "u8"),                            # x8 strip kernel, odd low-resolution sizes
    (2, 1, (7, 11), (29, 44), 19, [32, 20], "i64"),                        # generic kernel, odd output height
    (3, 2, (9, 13), (72, 104), 7, [8, 12, 8], "i64"),                      # x8, few classes (CQ = 2)
    (4, 1, (7, 11), (29, 44), 19, [24, 32, 20, 28], "u8"),
    (5, 2, (9, 13), (72, 104), 19, [32, 20, 24, 32, 28], "u8"),            # the five supernet heads
    (5, 1, (8, 16), (64, 128), 19, [32] * 5, "i32"),
    (2, 1, (8, 16), (64, 128), 25, [28, 32], "u8"),                       # x8 geometry, C > 20: the generic kernel
    (3, 2, (9, 13), (72, 104), 32, [32, 32, 32], "i64"),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES)
def test_heads_confusion_equals_argmax_plus_hist_info(case, dtype):
    from fasterseg_amd import kernels as K
    Kh, N, (h, w), (H, W), C, cs, kind = case
    gen = torch.Generator().manual_seed(7 + Kh)
    heads = [_head(N, C, h, w, c, dtype, gen) for c in cs]
    gt = _labels(N, H, W, C, kind, gen)
    hist = torch.zeros(Kh * C * C, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2 * Kh, dtype=torch.int64, device="cuda")
    K.heads_confusion(heads, gt, hist, counts)
    K.heads_confusion(heads, gt, hist, counts)        # accumulates
    for k, head in enumerate(heads):
        want_h, want_c = _per_head(head, gt)
        assert torch.equal(hist[k * C * C:(k + 1) * C * C], 2 * want_h), k
        assert torch.equal(counts[2 * k:2 * k + 2], 2 * want_c), k
    assert int(counts[0]) > 0


def test_heads_confusion_against_torch_interpolate():
    """Sanity against torch: F.interpolate(align_corners=True).argmax(1) + numpy hist_info agree on >= 99.99 % of the pixels (rounding
    near ties may differ: not a bit-exact check)."""
    from fasterseg_amd import kernels as K
    gen = torch.Generator().manual_seed(3)
    N, C, h, w, H, W = 2, 19, 32, 64, 256, 512
    heads = [_head(N, C, h, w, 32, torch.float32, gen) for _ in range(5)]
    gt = _labels(N, H, W, C, "u8", gen)
    hist = torch.zeros(5 * C * C, dtype=torch.int64, device="cuda")
    counts = torch.zeros(10, dtype=torch.int64, device="cuda")
    K.heads_confusion(heads, gt, hist, counts)
    g = gt.cpu().numpy()
    for k, head in enumerate(heads):
        up = F.interpolate(head.float().contiguous(), size=(H, W), mode="bilinear", align_corners=True)
        pred = up.argmax(1).cpu().numpy()
        want, labeled, correct = hist_info_np(C, pred, g)
        got = hist[k * C * C:(k + 1) * C * C].cpu().numpy().reshape(C, C)
        assert int(counts[2 * k]) == labeled
        assert np.abs(got - want).sum() // 2 <= 1e-4 * labeled, k
        assert abs(int(counts[2 * k + 1]) - correct) <= 1e-4 * labeled, k


def test_heads_confusion_error_status():
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    gen = torch.Generator().manual_seed(1)
    head = _head(1, 19, 8, 16, 32, torch.float32, gen)
    gt = _labels(1, 64, 128, 19, "u8", gen)
    hist = torch.zeros(19 * 19, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    ptrs = (ctypes.c_void_p * 1)(head.data_ptr())

    def status(**kw):
        f = dict(K=1, N=1, h=8, w=16, C=19, H=64, W=128, dtype=_lib.FS_F32, cs=32)
        f.update(kw)
        d = _lib.HeadsDesc(f["K"], f["N"], f["h"], f["w"], f["C"], f["H"], f["W"], f["dtype"],
                           (ctypes.c_int * _lib.FS_MAX_HEADS)(*([f["cs"]] * _lib.FS_MAX_HEADS)))
        return _lib.lib().fs_heads_confusion(K._stream(), ctypes.byref(d), ptrs, K._p(gt), 1, K._p(hist), K._p(counts))

    assert status(K=9) == 2 and status(C=33) == 2 and status(K=0) == 2           # FS_ERR_UNSUPPORTED
    assert status(cs=18) == 1 and status(cs=16) == 1 and status(dtype=5) == 1    # FS_ERR_INVALID: stride, dtype
    assert _lib.lib().fs_heads_confusion(K._stream(), None, ptrs, K._p(gt), 1, K._p(hist), K._p(counts)) == 1
    with pytest.raises(_lib.FasterSegHipError, match="channel stride"):
        d = _lib.HeadsDesc(1, 1, 8, 16, 19, 64, 128, _lib.FS_F32, (ctypes.c_int * _lib.FS_MAX_HEADS)(*([19] * 8)))
        _lib.call("fs_heads_confusion", K._stream(), ctypes.byref(d), ptrs, K._p(gt), 1, K._p(hist), K._p(counts))
    # labels must cover every image: (N, H, W), or (H, W) only for N = 1 (here H == N, which a loose check would take)
    heads2 = [_head(2, 19, 1, 4, 32, torch.float32, gen)]
    with pytest.raises(AssertionError):
        K.heads_confusion(heads2, _labels(1, 2, 32, 19, "u8", gen)[0], hist, counts)
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0 and int(counts.sum()) == 0, "a refused call writes nothing"
    assert status() == 0


# ---- the supernet --------------------------------------------------------------------------------------------------------------
_NET = {}


def _supernet():
    if "net" not in _NET:
        from fasterseg_amd import model_search
        net = model_search.Network_Multi_Path(criterion=torch.nn.CrossEntropyLoss(ignore_index=255), **CFG)
        sd = seeded_state(net.state_dict(), 777)
        for k in list(sd):
            if k.split("_")[0] in ("alpha", "beta", "ratio"):
                sd[k] = sd[k] * 5.0
        net.load_state_dict(sd)
        _NET["net"] = net.cuda().eval()
    return _NET["net"]


@pytest.mark.parametrize("arch_idx", [0, 1])
def test_forward_lowres_then_x8_equals_forward(arch_idx):
    from fasterseg_amd import functional as FN
    from fasterseg_amd import kernels as K
    net = _supernet()
    net.arch_idx, net.prun_mode = arch_idx, None          # arch 1: Gumbel widths, drawn from the same seeds below
    x = seeded_input((1, 3, 64, 128), 5).cuda()
    with torch.no_grad(), K.deterministic():
        torch.manual_seed(4)
        np.random.seed(4)
        lo = net.forward_lowres(x)
        torch.manual_seed(4)
        np.random.seed(4)
        full = net(x)
    assert len(lo) == 5
    for p, want in zip(lo, full):
        assert p.shape == (1, 19, 8, 16) and K.channel_stride(p) % 4 == 0
        got = FN.interpolate(p, scale_factor=8, out_nchw=1)
        assert torch.equal(got, want)


def _source(n=2, H=128, W=256):
    from fasterseg_amd.dataloader import ArraySource
    rng = np.random.RandomState(11)
    imgs, lbls = [], []
    for _ in range(n):
        imgs.append(rng.randint(0, 256, (H, W, 3)).astype(np.uint8))
        lbl = rng.randint(0, 19, (H, W)).astype(np.uint8)
        lbl[rng.rand(H, W) < 0.1] = 255
        lbls.append(lbl)
    return ArraySource(imgs, lbls, down_sampling=2)


def _reference_sweeps(net, src, heads=(0, 1, 2, 3, 4)):
    """train_search.py:259-271 + evaluator.py:297-318 restated: one sweep per head, one module forward per image, arg-max of the
    up-sampled score, numpy hist_info, compute_score.  Returns [(hist, labeled, correct)] per head."""
    out = []
    for o in heads:
        hist, labeled, correct = np.zeros((19, 19), np.int64), 0, 0
        for i in range(len(src)):
            img, lbl = src.get(i)
            x = torch.from_numpy(np.ascontiguousarray(normalize(img.cpu().numpy()).transpose(2, 0, 1)[None])).cuda()
            with torch.no_grad():
                score = net(x)[o]
            pred = score[0].argmax(0).cpu().numpy()
            h, l, c = hist_info_np(19, pred, lbl.cpu().numpy())
            hist += h
            labeled += l
            correct += c
        out.append((hist, labeled, correct))
    return out


@pytest.mark.parametrize("mode,arch_idx,share", [("min", 0, True), ("min", 0, False), ("max", 0, True), ("max", 0, False),
                                                 ("random", 0, False), ("arch_ratio", 1, False)])
def test_supernet_evaluator_equals_the_reference_sweeps(mode, arch_idx, share):
    from fasterseg_amd import kernels as K
    from fasterseg_amd.metric import compute_score
    from fasterseg_amd.search_eval import SupernetEvaluator
    net = _supernet()
    src = _source()
    ev = SupernetEvaluator(net, 19, MEAN, STD, src, share_forward=share)
    with K.deterministic():
        net.arch_idx, net.prun_mode = arch_idx, mode
        np.random.seed(8)
        torch.manual_seed(8)
        mious = ev.run()
        metrics = ev.compute_metric()
        net.arch_idx, net.prun_mode = arch_idx, mode
        np.random.seed(8)
        torch.manual_seed(8)
        want = _reference_sweeps(net, src)
    assert len(mious) == 5 and len(metrics) == 5
    for m, miou, (hist, labeled, correct) in zip(metrics, mious, want):
        assert np.array_equal(m["hist"], hist) and m["labeled"] == labeled and m["correct"] == correct
        iu, mean_IU, _, acc = compute_score(hist, correct, labeled)
        assert miou == m["mean_IU"] == mean_IU and m["mean_pixel_acc"] == acc
    assert metrics[0]["labeled"] > 0


def test_search_mode_validation_exports_loadable_architectures(tmp_path):
    """validate_epoch's search branch (pretrain = the path of the pretrained weights): prun_mode None, one (mIoUs, fps0, fps1) per
    architecture index with the latencies from the table (the reference's 1080Ti fixture), the model back in train mode; its results
    through arch_states, save_arch, a plain torch.load and build_derived."""
    import json
    import os
    from fasterseg_amd import archs, model_search, operations, search_eval
    from fasterseg_amd import kernels as K
    net = model_search.Network_Multi_Path(criterion=torch.nn.CrossEntropyLoss(ignore_index=255), **CFG)
    net.load_state_dict(_supernet().state_dict())
    net = net.cuda()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latency_lut_1080ti.json")) as f:
        lut = json.load(f)
    saved = dict(operations.latency_lookup_table)
    operations.latency_lookup_table.clear()
    operations.latency_lookup_table.update(lut)
    try:
        ev = search_eval.SupernetEvaluator(net, 19, MEAN, STD, _source(1))
        torch.manual_seed(6)
        with K.deterministic():
            res = search_eval.validate_epoch(net, ev, "pretrained/weights.pt")
        assert net.training and net.prun_mode is None and net.arch_idx == len(net._arch_names) - 1
        assert len(res) == 2
        for idx, (mious, fps0, fps1) in enumerate(res):
            assert len(mious) == 5 and all(0.0 <= m <= 1.0 for m in mious)
            net.arch_idx = idx
            assert (fps0, fps1) == search_eval.arch_fps(net)
        search_eval.save_arch(str(tmp_path), search_eval.arch_states(net, res, "pretrained/weights.pt"), 0)
    finally:
        operations.latency_lookup_table.clear()
        operations.latency_lookup_table.update(saved)
    for idx in (0, 1):
        state = torch.load(str(tmp_path / ("arch_%d.pt" % idx)))          # torch.load's default: weights only
        assert state["mIoU02"] == float(res[-1][0][3]) and state["latency12"] == 1000. / res[-1][2]
        d = archs.build_derived(idx, training=True, layers=CFG["layers"], state=state)
        assert d.lasts in ([2, 0], [2, 1])


# ---- no side effects on training ---------------------------------------------------------------------------------------------
class SmallSearch:
    lr = 2e-2
    momentum = 0.9
    weight_decay = 5e-4
    grad_clip = 5
    arch_learning_rate = 3e-4
    layers = 5
    Fch = 12
    width_mult_list = WML
    prun_modes = ['max', 'arch_ratio']
    stem_head_width = [(1, 1), (8. / 12, 8. / 12)]
    latency_weight = [0, 1e-2]


def _train(validate):
    from fasterseg_amd import kernels as K
    from fasterseg_amd import search_eval
    from fasterseg_amd.train_step import SupernetStep
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(2, 3, 128, 256, generator=g).cuda()
    tgt = torch.randint(0, 19, (2, 16, 32), generator=g)
    tgt[torch.rand(2, 16, 32, generator=g) < 0.05] = 255
    tgt = tgt.cuda()
    with K.deterministic():
        st = SupernetStep(pretrain=True, cfg=SmallSearch, seed=11, use_graphs=True)
        np.random.seed(21)
        losses = [float(st.step(imgs, tgt)[0]) for _ in range(2)]
        if validate:
            ev = search_eval.SupernetEvaluator(st.model, 19, MEAN, STD, _source(1))
            rng = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state_all())
            sel = (st.model.arch_idx, st.model.prun_mode)
            res = search_eval.validate_epoch(st.model, ev, True)
            assert set(res) == {"min", "max", "random"} and all(len(v) == 5 for v in res.values())
            assert st.model.training and st.model.prun_mode == "random"
            random.setstate(rng[0])
            np.random.set_state(rng[1])
            torch.set_rng_state(rng[2])
            torch.cuda.set_rng_state_all(rng[3])
            st.model.arch_idx, st.model.prun_mode = sel
        losses += [float(st.step(imgs, tgt)[0]) for _ in range(2)]
        torch.cuda.synchronize()
    return losses, {k: v.detach().cpu().clone() for k, v in st.model.state_dict().items()}


def test_validation_between_graphed_steps_changes_nothing():
    """validate_epoch between graphed pretrain steps (bit-reproducible mode), with the host RNGs and the model's selection put back
    as the reference's seeds would have them: losses, weights, BatchNorm statistics identical to a run without it."""
    a_losses, a_sd = _train(False)
    b_losses, b_sd = _train(True)
    assert a_losses == b_losses, (a_losses, b_losses)
    assert list(a_sd) == list(b_sd)
    for k in a_sd:
        assert torch.equal(a_sd[k], b_sd[k]), k


# ---- an exported architecture through training and inference -----------------------------------------------------------------
def test_exported_architecture_trains_and_infers(tmp_path):
    from fasterseg_amd import archs, engine, model_search, search_eval, train_step
    net = model_search.Network_Multi_Path(19, 16, None, 12, WML, ['max', 'arch_ratio'], [(1, 1), (8. / 12, 8. / 12)])
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for idx in (0, 1):
            for k, v in archs.load_arch(idx).items():
                if torch.is_tensor(v):
                    getattr(net, k).copy_(v + 0.05 * torch.randn(v.shape, generator=g))
    results = [([0.3, 0.3, 0.3, 0.31, 0.30], 150.0, 140.0), ([0.2, 0.2, 0.2, 0.22, 0.21], 180.0, 170.0)]
    search_eval.save_arch(str(tmp_path), search_eval.arch_states(net, results, "w.pt"), 0)
    states = [torch.load(str(tmp_path / ("arch_%d.pt" % i))) for i in (0, 1)]
    student = archs.init_weight(archs.build_derived(1, state=states[1])).cuda().eval()
    eng = engine.InferenceEngine(student, (1, 3, 128, 256), dtype=torch.float32)
    x = seeded_input((1, 3, 128, 256), 9).cuda()
    with torch.no_grad():
        out = eng(x).clone()
        want = student(x)
    torch.cuda.synchronize()
    assert out.shape == (1, 19, 128, 256) and bool(torch.isfinite(out).all())
    assert float((out - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))
    st = train_step.StudentDistillStep(2, 128, 256, arch_states=states)
    imgs, target = train_step.synthetic_batch(2, 128, 256, 0, "cuda")
    loss = st.step(imgs, target)
    assert bool(torch.isfinite(loss).all())
