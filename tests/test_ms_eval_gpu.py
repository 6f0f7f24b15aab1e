"""GPU: multi-scale / sliding-window / flip evaluation (fs_eval_window_input, fs_eval_score_accumulate, fs_eval_rescale_accumulate
and SegEvaluator's sliding_eval / whole_eval(output_size, input_size) / is_flip) against restatements of the reference in this file:
cv2's 8-bit INTER_LINEAR (fixed point, INTER_RESIZE_COEF_BITS = 11) and float INTER_LINEAR in numpy, tools/engine/evaluator.py's
whole_eval / sliding_eval / scale_process / val_func_process in float64 numpy around the oracle's forward (oracle.ref_ops).

The 8-bit resize restates the formula OpenCV 4 uses for uint8 INTER_LINEAR; it has not been checked against a cv2 build."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])       # config_train.py:44-45
SCALES = [0.5, 0.6, 0.75, 1.0, 1.25]


# ---- restatement of the reference's host-side arithmetic ----------------------------------------------------------------------
def cv_round(v):
    return int(np.rint(v))


def u8_taps(src, dst, s):
    """cv2 resize.cpp, INTER_LINEAR on 8-bit data: fx = (float)((d + 0.5) * (1 / s) - 0.5), sx = floor, clamp, cvRound coefficients."""
    fx = ((np.arange(dst) + 0.5) * (1.0 / s) - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    fx[sx < 0] = 0
    sx[sx < 0] = 0
    fx[sx >= src - 1] = 0
    sx[sx >= src - 1] = src - 1
    c0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    return sx, np.minimum(sx + 1, src - 1), c0, c1


def resize_u8(img, s):
    """cv2.resize(img, None, fx=s, fy=s, interpolation=cv2.INTER_LINEAR) for uint8 HWC."""
    H, W, _ = img.shape
    rows, cols = cv_round(H * s), cv_round(W * s)
    y0, y1, b0, b1 = u8_taps(H, rows, s)
    x0, x1, a0, a1 = u8_taps(W, cols, s)
    S = img.astype(np.int64)
    D = S[:, x0] * a0[None, :, None] + S[:, x1] * a1[None, :, None]            # horizontal pass, int32 range
    out = (((b0[:, None, None] * (D[y0] >> 4)) >> 16) + ((b1[:, None, None] * (D[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def normalize(img):
    """(u / 255 - mean) / std in fp32, the expression of SegEvaluator.process_image."""
    x = img.astype(np.float32) / np.float32(255)
    return (x - MEAN.astype(np.float32)) / STD.astype(np.float32)


def pad_margins(rows, cols, shape):
    ph, pw = max(shape[0] - rows, 0), max(shape[1] - cols, 0)
    return ph // 2, ph // 2 + ph % 2, pw // 2, pw // 2 + pw % 2


def pad(img, shape, value=0):
    t, b, l, r = pad_margins(img.shape[0], img.shape[1], shape)
    return np.pad(img, ((t, b), (l, r), (0, 0)), constant_values=value), (t, b, l, r)


def resize_float(score, H, W):
    """cv2.resize(score (h, w, C) float, (W, H), INTER_LINEAR): half-pixel centres, edge clamp, float64 here."""
    h, w = score.shape[:2]

    def taps(src, dst):
        # cv2 resize.cpp: scale = 1 / (dsize / ssize) in double, the source position rounded to float: (float)((d + 0.5) * scale - 0.5)
        f = ((np.arange(dst) + 0.5) * (1.0 / (dst / src)) - 0.5).astype(np.float32)
        i = np.floor(f).astype(np.int64)
        f = (f - i.astype(np.float32)).astype(np.float64)
        f[i < 0] = 0
        i[i < 0] = 0
        f[i >= src - 1] = 0
        i[i >= src - 1] = src - 1
        return i, np.minimum(i + 1, src - 1), f
    y0, y1, fy = taps(h, H)
    x0, x1, fx = taps(w, W)
    s = score.astype(np.float64)
    d = s[:, x0] * (1 - fx)[None, :, None] + s[:, x1] * fx[None, :, None]
    return d[y0] * (1 - fy)[:, None, None] + d[y1] * fy[:, None, None]


class RefEvaluator:
    """tools/engine/evaluator.py whole_eval / sliding_eval / scale_process / val_func_process with the oracle as val_func."""

    def __init__(self, forward, is_flip):
        self.forward, self.is_flip = forward, is_flip

    def val_func_batch(self, xs):
        """[(crop, crop, 3) normalised] -> [(19, crop, crop) exp-score] (evaluator.py:297-318), batched for speed."""
        x = torch.tensor(np.stack([a.transpose(2, 0, 1) for a in xs]).astype(np.float32))
        if self.is_flip:
            x = torch.cat([x, x.flip(-1)])
        with torch.no_grad():
            logits = self.forward(x)
        n = len(xs)
        score = logits[:n]
        if self.is_flip:
            score = score + logits[n:].flip(-1)
        return [np.exp(score[i].numpy()).astype(np.float64) for i in range(n)], [score[i].numpy() for i in range(n)]

    def scale_process(self, img, ori_shape, crop):
        new_rows, new_cols, _ = img.shape
        if max(new_rows, new_cols) <= crop:
            x, m = pad(normalize(img), (crop, crop))
            score = self.val_func_batch([x])[0][0][:, m[0]:crop - m[1], m[2]:crop - m[3]]
        else:
            stride = int(np.ceil(crop * self.stride_rate))
            img_pad, m = pad(img, (crop, crop))
            pad_rows, pad_cols = img_pad.shape[:2]
            r_grid = int(np.ceil((pad_rows - crop) / stride)) + 1
            c_grid = int(np.ceil((pad_cols - crop) / stride)) + 1
            data_scale = np.zeros((19, pad_rows, pad_cols))
            wins = []
            for gy in range(r_grid):
                for gx in range(c_grid):
                    e_x, e_y = min(gx * stride + crop, pad_cols), min(gy * stride + crop, pad_rows)
                    wins.append((e_y - crop, e_x - crop))
            scores = self.val_func_batch([normalize(img_pad[sy:sy + crop, sx:sx + crop]) for sy, sx in wins])[0]
            for (sy, sx), sc in zip(wins, scores):
                data_scale[:, sy:sy + crop, sx:sx + crop] += sc
            score = data_scale[:, m[0]:pad_rows - m[1], m[2]:pad_cols - m[3]]
        return resize_float(score.transpose(1, 2, 0), ori_shape[0], ori_shape[1])

    def sliding_eval(self, img, scales, crop, stride_rate):
        self.stride_rate = stride_rate
        H, W = img.shape[:2]
        total = np.zeros((H, W, 19))
        for s in scales:
            total += self.scale_process(resize_u8(img, s), (H, W), crop)
        return total.argmax(2), total

    def whole_eval(self, img, output_size=None, input_size=None):
        """Returns (class map, the score the arg-max is taken of)."""
        x = normalize(img)
        m = (0, 0, 0, 0)
        if input_size is not None:
            x, m = pad(x, input_size)
        exp_score, logit = self.val_func_batch([x])
        Hp, Wp = x.shape[:2]
        score = exp_score[0][:, m[0]:Hp - m[1], m[2]:Wp - m[3]].transpose(1, 2, 0)
        logit = logit[0][:, m[0]:Hp - m[1], m[2]:Wp - m[3]].transpose(1, 2, 0)
        if output_size is not None:
            score = resize_float(score, output_size[0], output_size[1])
            return score.argmax(2), score
        return logit.argmax(2), logit


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
_NET = {}


def student():
    """arch_1 student with seeded weights (as tests/test_eval_path.py) and the oracle forward on its parameters."""
    if not _NET:
        from fasterseg_amd import archs
        from oracle import ref_ops
        from oracle.seeded import resolve_aliases, seeded_state
        with open(os.path.join(ROOT, "tests", "golden", "arch_1.json")) as f:
            meta = json.load(f)["eval_21"]
        net = archs.build_derived(1, training=False, lasts=[2, 1])
        state = seeded_state(net.state_dict(), 12345)
        net.load_state_dict(state)
        params = resolve_aliases({k: v.clone() for k, v in state.items()}, meta)
        _NET["net"] = net.cuda().eval()
        _NET["forward"] = lambda x: ref_ops.derived_forward(params, meta, x, training=False)
    return _NET["net"], _NET["forward"]


def images(H, W, n=2, seed=7):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        # smooth structure plus noise, so that the network's classes form regions (a pure-noise image gives near-ties everywhere)
        base = rng.randint(0, 256, size=(H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
        up = np.kron(base, np.ones((16, 16, 1)))[:H, :W]
        out.append(np.clip(up + rng.randint(-40, 41, size=(H, W, 3)), 0, 255).astype(np.uint8))
    return out


def labels(H, W, seed):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, 19, size=(H, W)).astype(np.uint8)
    lab[rng.rand(H, W) < 0.05] = 255
    return lab


def clear_mask(score, rel):
    top2 = np.sort(score, axis=2)[..., -2:]
    return (top2[..., 1] - top2[..., 0]) > rel * np.abs(top2[..., 1])


# ---- 1. fs_eval_window_input ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("s", [0.5, 0.6, 0.75, 1.0, 1.25, 1.75])
def test_window_input_bit_exact(s):
    from fasterseg_amd import eval_plan as EP
    from fasterseg_amd import kernels as K
    H, W, crop = 200, 328, 128
    img = np.random.RandomState(int(s * 100)).randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    rs = resize_u8(img, s)
    rows, cols = rs.shape[:2]
    (plan,) = EP.scale_plan(H, W, [s], crop, 5 / 6)
    ytab = torch.from_numpy(EP.pack_taps(plan.y_index, plan.y_coef)).cuda()
    xtab = torch.from_numpy(EP.pack_taps(plan.x_index, plan.x_coef)).cuda()
    dimg = torch.from_numpy(img).cuda()
    u8_canvas, m = pad(rs, (crop, crop))                         # pad mode 0: uint8 0, normalised afterwards
    norm_canvas, m2 = pad(normalize(rs), (crop, crop))           # pad mode 1: 0 after normalisation
    assert m == m2 and (m[0], m[2]) == (plan.top, plan.left)
    origins = plan.windows + [(0, 0), (u8_canvas.shape[0] - crop, u8_canvas.shape[1] - crop)]
    sentinel = 1234.5
    for pad_mode in (0, 1):
        for flip in (0, 1):
            for oy, ox in origins:
                buf = torch.full((4 * 3 * crop * crop + 64,), sentinel, dtype=torch.float32, device="cuda")
                out = buf[32:32 + 3 * 3 * crop * crop].view(3, 3, crop, crop)       # slot 2 (and slot 1 without flip) must stay
                d = K.eval_window_desc(H, W, rows, cols, plan.top, plan.left, oy, ox, crop, crop, pad_mode, flip, MEAN, STD)
                K.eval_window_input(d, dimg, ytab, xtab, out)
                got = buf.cpu().numpy()
                if pad_mode == 0:
                    want = normalize(u8_canvas[oy:oy + crop, ox:ox + crop])
                else:
                    want = norm_canvas[oy:oy + crop, ox:ox + crop]
                want = want.transpose(2, 0, 1).astype(np.float32)
                win = got[32:32 + 3 * 3 * crop * crop].reshape(3, 3, crop, crop)
                assert np.array_equal(win[0].view(np.uint32), want.view(np.uint32)), \
                    "s=%g pad_mode=%d origin=%s: %d values differ" % (s, pad_mode, (oy, ox), int((win[0] != want).sum()))
                if flip:
                    assert np.array_equal(win[1].view(np.uint32), want[:, :, ::-1].copy().view(np.uint32))
                else:
                    assert (win[1] == sentinel).all()
                assert (win[2] == sentinel).all() and (got[:32] == sentinel).all() and (got[32 + 3 * 3 * crop * crop:] == sentinel).all()


# ---- 2. fs_eval_score_accumulate -----------------------------------------------------------------------------------------------
def _lowres_logits(dtype, N=2, C=19, h=16, w=24, cs=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    full = (torch.randn(N, h, w, cs, generator=g) * 2).to(dtype)        # pad channels hold garbage: they must not matter
    return full, full.cuda().permute(0, 3, 1, 2)[:, :C]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("flip", [0, 1])
def test_score_accumulate(dtype, flip):
    from fasterseg_amd import kernels as K
    C, h, w = 19, 16, 24
    Hw, Ww = 8 * h, 8 * w
    full, logits = _lowres_logits(dtype, C=C, h=h, w=w)
    up = F.interpolate(full.float().permute(0, 3, 1, 2)[:, :C], size=(Hw, Ww), mode="bilinear", align_corners=True)
    l = up[0] + (up[1].flip(-1) if flip else 0)
    e = torch.exp(l).permute(1, 2, 0)                                  # (Hw, Ww, C)
    y0, x0, rows, cols, cy, cx = 5, 7, 100, 150, 3, 9
    g = torch.Generator().manual_seed(1)
    pre = torch.rand(120, 170, 20, generator=g)
    for store in (False, True):
        canvas = pre.clone().cuda()
        K.eval_score_accumulate(logits, (Hw, Ww), flip, (y0, x0, rows, cols), canvas=canvas, at=(cy, cx), store=store)
        got = canvas.cpu()
        want = pre.clone()
        region = e[y0:y0 + rows, x0:x0 + cols]
        want[cy:cy + rows, cx:cx + cols, :C] = region if store else want[cy:cy + rows, cx:cx + cols, :C] + region
        if store:
            want[cy:cy + rows, cx:cx + cols, C:] = 0
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
        outside = torch.ones(120, 170, dtype=torch.bool)
        outside[cy:cy + rows, cx:cx + cols] = False
        assert torch.equal(got[outside], pre[outside]), "canvas pixels outside the rectangle changed"
        if not store:
            assert torch.equal(got[..., C:], pre[..., C:]), "the pad channel changed"
    # arg-max mode: the class map of l0 (+ l1 mirrored) over the same rectangle, the canvas untouched
    classes = torch.full((rows * cols + 8,), 77, dtype=torch.uint8, device="cuda")
    K.eval_score_accumulate(logits, (Hw, Ww), flip, (y0, x0, rows, cols), classes=classes[:rows * cols])
    got = classes[:rows * cols].view(rows, cols).cpu().numpy()
    assert (classes[rows * cols:].cpu() == 77).all()
    lw = l[:, y0:y0 + rows, x0:x0 + cols].permute(1, 2, 0).numpy()
    top2 = np.sort(lw, axis=2)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-4
    assert clear.mean() > 0.99
    assert (got == lw.argmax(2))[clear].all()


# ---- 3. fs_eval_rescale_accumulate ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rect,out", [((2, 3, 37, 53), (64, 96)), ((0, 0, 80, 120), (50, 70)), ((4, 1, 61, 83), (61, 83))],
                         ids=["up", "down", "same"])
def test_rescale_accumulate(rect, out):
    from fasterseg_amd import kernels as K
    C = 19
    g = torch.Generator().manual_seed(3)
    canvas = torch.rand(90, 130, 20, generator=g) * 5
    pre = torch.rand(out[0], out[1], 20, generator=g)
    y0, x0, rows, cols = rect
    src = canvas[y0:y0 + rows, x0:x0 + cols].permute(2, 0, 1)[None]
    res = F.interpolate(src.double(), size=out, mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    res_cv = torch.from_numpy(resize_float(src[0].permute(1, 2, 0).numpy(), out[0], out[1]))
    for store in (False, True):
        total = pre.clone().cuda()
        classes = torch.empty(out, dtype=torch.uint8, device="cuda")
        K.eval_rescale_accumulate(canvas.cuda(), C, rect, total, store=store, classes=classes)
        got = total.cpu()[..., :C].double()
        # cv2 rounds each source position to float ((float)((d + 0.5) * scale - 0.5)), torch keeps it in double here: the weights
        # differ by up to a float ulp of the position, i.e. |error| <= ulp(position) * |neighbour difference|
        torch.testing.assert_close(got, (res + (0 if store else pre))[..., :C].double(), rtol=1e-5, atol=1e-5 * float(canvas.abs().max()))
        want = res_cv + (0 if store else pre)
        torch.testing.assert_close(got, want[..., :C].double(), rtol=1e-5, atol=1e-6)
        w = want[..., :C].numpy()
        clear = clear_mask(w, 1e-4)
        assert clear.mean() > 0.99
        assert (classes.cpu().numpy() == w.argmax(2))[clear].all()
    with pytest.raises(Exception):           # a rectangle outside the canvas is refused with a status, not run
        K.eval_rescale_accumulate(canvas.cuda(), C, (50, 0, 80, 120), total, store=True)


# ---- 4 / 5. end to end -------------------------------------------------------------------------------------------------------
_REF = {}


def _reference_sliding(img_idx, img):
    if img_idx not in _REF:
        _, forward = student()
        _REF[img_idx] = RefEvaluator(forward, True).sliding_eval(img, SCALES, 256, 5 / 6)
    return _REF[img_idx]


def _end_to_end(dtype):
    from fasterseg_amd.evaluator import SegEvaluator
    net, _ = student()
    ev = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), dtype=dtype, multi_scales=SCALES, is_flip=True, crop_size=256)
    assert ev.engine is None
    hist = np.zeros((19, 19), dtype=np.int64)
    labeled = correct = 0
    agree_all = []
    for i, img in enumerate(images(256, 512)):
        label = labels(256, 512, 10 + i)
        pred = ev.func_per_iteration({"data": img, "label": label}).cpu().numpy()
        ref_pred, ref_total = _reference_sliding(i, img)
        agree = pred == ref_pred
        agree_all.append(agree)
        if dtype == torch.float32:
            clear = clear_mask(ref_total, 5e-3)
            assert agree[clear].all(), "image %d: %d clear-cut pixels disagree" % (i, int((~agree[clear]).sum()))
        h, l, c = ref_eval.hist_info(19, pred, label.astype(np.int64))
        hist += h; labeled += int(l); correct += int(c)
    got = ev.compute_metric()
    assert (got["hist"] == hist).all() and got["labeled"] == labeled and got["correct"] == correct
    iu, miou, _, acc = ref_eval.compute_score(hist, correct, labeled)
    np.testing.assert_allclose(got["iu"], iu, rtol=1e-12)
    np.testing.assert_allclose(got["mean_IU"], miou, rtol=1e-12)
    assert abs(got["mean_pixel_acc"] - acc) < 1e-12
    assert set(ev._lowres) == {(2, 3, 256, 256)}                    # every pass of scale_process is crop x crop
    return float(np.mean(agree_all))


@pytest.mark.gpu
def test_sliding_eval_fp32_matches_reference():
    assert _end_to_end(torch.float32) >= 0.999


@pytest.mark.gpu
def test_sliding_eval_bf16_matches_reference():
    assert _end_to_end(torch.bfloat16) >= 0.97


# ---- 6. single-scale flip, padded / resized whole_eval -------------------------------------------------------------------------
@pytest.mark.gpu
def test_whole_eval_flip_and_sizes():
    from fasterseg_amd.evaluator import SegEvaluator
    net, forward = student()
    ev = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), dtype=torch.float32, is_flip=True)
    assert ev.engine is None
    img = images(256, 512, n=1, seed=3)[0]
    pred = ev.func_per_iteration({"data": img, "label": labels(256, 512, 1)}).cpu().numpy()   # one scale: whole_eval
    assert set(ev._lowres) == {(2, 3, 256, 512)}
    ref_pred, ref_logit = RefEvaluator(forward, True).whole_eval(img)
    top2 = np.sort(ref_logit, axis=2)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 4e-3
    agree = pred == ref_pred
    assert agree[clear].all() and agree.mean() >= 0.999
    # padded to input_size (odd pads: 2 / 3 rows, 5 / 6 columns) and resized to output_size, with and without the mirrored pass
    small = images(251, 501, n=1, seed=4)[0]
    for flip, e in ((True, ev), (False, SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), dtype=torch.float32))):
        for output_size in ((200, 400), None):
            got = e.whole_eval(small, output_size=output_size, input_size=(256, 512)).cpu().numpy()
            want, score = RefEvaluator(forward, flip).whole_eval(small, output_size=output_size, input_size=(256, 512))
            assert got.shape == want.shape
            if output_size is None:
                top2 = np.sort(score, axis=2)[..., -2:]
                clear = (top2[..., 1] - top2[..., 0]) > 4e-3
            else:
                clear = clear_mask(score, 5e-3)
            agree = got == want
            assert agree[clear].all() and agree.mean() >= 0.999, (flip, output_size, agree.mean())


# ---- 7. determinism and defaults -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sliding_eval_deterministic_and_defaults(monkeypatch):
    from fasterseg_amd.evaluator import SegEvaluator
    # one fixed plan for every engine: timing-based kernel / cell choices may differ between builds in the last bits
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    monkeypatch.setenv("FS_ENGINE_FUSE_CELLS", "1")
    net, _ = student()
    img = images(256, 512, n=1, seed=9)[0]
    ev = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), dtype=torch.bfloat16, multi_scales=[0.75, 1.0, 1.25], is_flip=True,
                      crop_size=256)
    a = ev.sliding_eval(img, 256, 5 / 6).clone()
    st = ev._states[(256, 512)]
    total_a = st.total.clone()
    canvas_ptr = st.canvas.data_ptr()
    b = ev.sliding_eval(img, 256, 5 / 6).clone()
    assert torch.equal(st.total.view(torch.int32), total_a.view(torch.int32)) and torch.equal(a, b)
    assert st.canvas.data_ptr() == canvas_ptr                        # buffers reused, not re-allocated per frame
    d0 = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), dtype=torch.float32)
    d1 = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), dtype=torch.float32, multi_scales=(1,), is_flip=False, crop_size=None,
                      stride_rate=5 / 6)
    for d in (d0, d1):
        assert d.engine is not None and d.engine.output_mode == "classes" and not d._lowres
    c0 = d0.func_per_iteration({"data": img, "label": labels(256, 512, 2)}).clone()
    c1 = d1.func_per_iteration({"data": img, "label": labels(256, 512, 2)}).clone()
    assert torch.equal(c0, c1) and not d0._lowres and not d0._states
