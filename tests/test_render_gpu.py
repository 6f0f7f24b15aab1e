"""GPU: fs_render_prediction, fasterseg_amd.visualize, SegTester / PredictionWriter and SegEvaluator's file outputs, every comparison
BIT-EXACT against the numpy restatement of tests/_render_ref.py (which tests/test_render.py ties to the reference's own outputs): the
kernel's arithmetic is fully specified - one rounded product, one fused multiply-add, round-half-even, saturate - so no tolerance
applies.  Composites are rendered into buffers with a guard band: bytes before and after the rows and in the pitch padding must
keep their sentinel."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _render_ref as R
from _util import GOLD, load_json, load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
SENTINEL = 0xA5


def tables():
    return load_json("cityscapes_labels.json")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def banded(nbytes, lead):
    """A sentinel-filled device buffer with `lead` guard bytes in front of and 64 behind `nbytes` payload bytes."""
    return torch.full((lead + nbytes + 64,), SENTINEL, dtype=torch.uint8, device="cuda")


def render_case(img, maps, palette, background, show255, weights, image_panel, gap, pad_pitch, lead=64, lut=None):
    """One launch through kernels.render_prediction into guard-banded buffers, compared byte for byte with the restatement."""
    from fasterseg_amd import kernels as K
    H, W = img.shape[:2]
    panels = len(weights)
    P = panels + int(image_panel)
    Wt = W * P + gap * (P - 1) if P else 0
    pitch = K.round_up(3 * Wt, 16) if pad_pitch else 3 * Wt
    comp_buf = comp = None
    if P:
        comp_buf = banded(H * pitch, lead)
        comp = comp_buf[lead:lead + H * pitch].view(H, pitch)[:, :3 * Wt].unflatten(1, (Wt, 3))
    ids_buf = ids = None
    if lut is not None:
        ids_buf = banded(H * W, lead)
        ids = ids_buf[lead:lead + H * W].view(H, W)
    K.render_prediction(dev(img) if P else None, [dev(m) for m in maps], dev(palette) if panels else None, comp, image_panel=image_panel,
                        gap=gap, background=background, show255=show255, weights=weights, lut=None if lut is None else dev(lut), ids=ids)
    what = (H, W, len(maps), image_panel, gap, pad_pitch, lead)
    if P:
        want = np.full(comp_buf.numel(), SENTINEL, dtype=np.uint8)
        rows = want[lead:lead + H * pitch].reshape(H, pitch)
        rows[:, :3 * Wt] = R.composite(palette, background, img, maps[:panels], show255, weights, image_panel, gap).reshape(H, 3 * Wt)
        got = comp_buf.cpu().numpy()
        assert np.array_equal(got, want), ("composite", what, np.flatnonzero(got != want)[:8])
    if lut is not None:
        want = np.full(ids_buf.numel(), SENTINEL, dtype=np.uint8)
        want[lead:lead + H * W] = R.label_ids(lut, maps[0]).reshape(-1)
        got = ids_buf.cpu().numpy()
        assert np.array_equal(got, want), ("ids", what, np.flatnonzero(got != want)[:8])


def class_map(rng, H, W):
    """Every class 0..18, values without a colour (19, 200) and the ignore label."""
    pool = np.array(list(range(19)) + [19, 200, 255], dtype=np.uint8)
    return pool[rng.randint(0, len(pool), size=(H, W))]


# ---- 1. the reference's own outputs ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_visualize_reproduces_the_reference_fixture():
    from fasterseg_amd import visualize as V
    g, t = load_npz("render.npz"), tables()
    colors, bg = t["colors"], t["background"]
    img, gt, p0, p1 = g["img"], g["gt"], g["pred0"], g["pred1"]
    assert np.array_equal(V.show_prediction(colors, bg, img, p0).cpu().numpy(), g["show_prediction"])
    assert np.array_equal(V.show_prediction(colors, bg, dev(img), dev(p0), 0.55).cpu().numpy(), g["show_prediction_055"])
    assert np.array_equal(V.show_img(colors, bg, img, np.zeros(gt.shape), gt, p0.astype(np.int64)).cpu().numpy(), g["show_img_1"])
    out = V.show_img(colors, bg, dev(img), None, dev(gt), dev(p0), p1)
    assert out.is_cuda and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), g["show_img_2"])
    # more predictions than one launch holds: chained into the same composite
    five = [p0, p1, gt, p1, p0]
    assert np.array_equal(V.show_img(colors, bg, img, None, gt, *five).cpu().numpy(), R.show_img(colors, bg, img, gt, *five))
    # set_img_color paints in place, numpy array and device tensor alike
    a, b = img.copy(), dev(img)
    assert V.set_img_color(colors, bg, a, gt, show255=True) is a and V.set_img_color(colors, bg, b, dev(gt), show255=True) is b
    want = R.overlay(colors, bg, img, gt, True, 0.55)
    assert np.array_equal(a, want) and np.array_equal(b.cpu().numpy(), want)
    spec = V.LabelSpec.from_json(os.path.join(GOLD, "cityscapes_labels.json"))
    assert np.array_equal(V.show_prediction(spec, spec.background, img, p0).cpu().numpy(), g["show_prediction"])


# ---- 2. the shapes that can break the vector path --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W", [1, 3, 15, 16, 17, 37, 64])
def test_every_panel_layout(W):
    t = tables()
    palette, lut = np.array(t["colors"], dtype=np.uint8), np.arange(256, dtype=np.uint8)[::-1].copy()
    rng = np.random.RandomState(100 + W)
    for H in (1, 5):
        img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        maps = [class_map(rng, H, W) for _ in range(4)]
        for gap in (0, 15):
            for pad_pitch in (False, True):
                for image_panel in (False, True):
                    for panels in range(5):
                        P = panels + image_panel
                        with_ids = P % 2 == 0 or panels == 0          # the ids alone (P == 0), beside an image panel, beside overlays
                        if P == 0 and (gap or pad_pitch):
                            continue                                   # the ids alone know neither gap nor pitch: once is enough
                        render_case(img, maps[:panels] if panels else maps[:int(with_ids)], palette, -1, [bool(i % 2) for i in range(panels)],
                                    [0.55, 1, 0.3, 0.55][:panels], image_panel, gap, pad_pitch, lead=64 if pad_pitch else 67,
                                    lut=lut if with_ids else None)


# ---- 3. class values -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_colors", [19, 256])
@pytest.mark.parametrize("background", [-1, 3])
def test_class_values(n_colors, background):
    rng = np.random.RandomState(n_colors + background)
    H, W = 6, 44
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    palette = np.array(tables()["colors"], dtype=np.uint8) if n_colors == 19 else rng.randint(0, 256, size=(256, 3)).astype(np.uint8)
    m = class_map(rng, H, W)
    m[0, :19] = np.arange(19)                   # every index, on the head / vector / tail pixels of a row
    m[1, :4] = [19, 200, 255, background & 255]
    m[2, -3:] = [255, 18, 19]
    for show255 in (False, True):
        render_case(img, [m, m], palette, background, [show255, not show255], [0.55, 0.55], False, 15, True)
        render_case(img, [m], palette, background, [show255], [1], True, 15, False, lead=65)
    painted = R.overlay(palette, background, img, m, False, 1)
    if n_colors == 19:
        assert np.array_equal(painted[m >= 19], img[m >= 19])                      # no colour: the image shows through
    else:
        assert np.array_equal(painted[m == 200], palette[200][None].repeat((m == 200).sum(), 0))
    if background >= 0:
        assert np.array_equal(painted[m == background], img[m == background])


# ---- 4. every (colour byte, image byte) pair -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_blend_exhaustive_on_the_device():
    palette = (np.arange(258) % 256).astype(np.uint8).reshape(86, 3)               # the 258 channel bytes run through 0..255
    img = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 86, axis=0).repeat(3, axis=2)       # column x holds byte x
    m = np.repeat(np.arange(86, dtype=np.uint8)[:, None], 256, axis=1)             # row r is class r
    assert set(palette.reshape(-1).tolist()) == set(range(256)) and set(img.reshape(-1).tolist()) == set(range(256))
    render_case(img, [m], palette, -1, [False], [0.55], False, 0, True)
    # the restatement the kernel was just held to is the documented rounding: exact off the ties, within 1 on them
    got = R.overlay(palette, -1, img, m, False, 0.55).astype(np.int64)
    c, o = palette[:, None, :].astype(np.int64), img.astype(np.int64)
    tie = (11 * c + 9 * o) % 20 == 10
    exact = (11 * c + 9 * o + 10) // 20
    assert np.array_equal(got[~tie], exact[~tie]) and np.abs(got - exact).max() <= 1 and 0 < tie.mean() <= 0.08


# ---- 5. the label-ID map ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_label_ids_alone_and_with_panels():
    from fasterseg_amd import visualize as V
    spec = V.LabelSpec.from_json(os.path.join(GOLD, "cityscapes_labels.json"))
    rng = np.random.RandomState(5)
    for H, W in ((1, 1), (3, 16), (7, 53), (64, 256)):
        img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        m0, m1 = class_map(rng, H, W), class_map(rng, H, W)
        for lead in (64, 69):
            render_case(img, [m0], spec.palette, -1, [], [], False, 0, False, lead=lead, lut=spec.lut)        # ids alone, no image
            render_case(img, [m0, m1], spec.palette, -1, [False, True], [1, 0.55], True, 15, True, lead=lead, lut=spec.lut)
    ids = R.label_ids(spec.lut, np.array([[0, 18, 19, 255]]))
    assert ids.tolist() == [[7, 33, 0, 0]]


# ---- 6. invalid arguments: a status and a message, nothing launched ---------------------------------------------------------------
@pytest.mark.gpu
def test_invalid_arguments_return_status():
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    h = _lib.lib()
    H, W = 4, 16
    img = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    m = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    pal = torch.zeros((19, 3), dtype=torch.uint8, device="cuda")
    lut = torch.zeros(256, dtype=torch.uint8, device="cuda")
    comp = torch.full((H, 3 * W), SENTINEL, dtype=torch.uint8, device="cuda")
    ids = torch.full((H, W), SENTINEL, dtype=torch.uint8, device="cuda")
    maps = (ctypes.c_void_p * 4)(m.data_ptr(), m.data_ptr(), m.data_ptr(), m.data_ptr())
    holes = (ctypes.c_void_p * 4)(m.data_ptr(), None, None, None)
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def desc(**kw):
        f = dict(H=H, W=W, panels=1, image_panel=0, gap=15, dst_pitch=3 * W, n_colors=19, background=-1, write_ids=0)
        f.update(kw)
        d = _lib.RenderDesc(*[f[n] for n, _ in _lib.RenderDesc._fields_[:9]])
        for i in range(4):
            d.alpha[i], d.beta[i] = 0.55, 0.45
        return d
    good = (p(img), maps, p(pal), p(lut), p(comp), p(ids))
    cases = {
        "null descriptor": (None,) + good,
        "H = 0": (desc(H=0),) + good,
        "W < 0": (desc(W=-3),) + good,
        "panels > 4": (desc(panels=5, dst_pitch=1 << 20),) + good,
        "panels < 0": (desc(panels=-1),) + good,
        "pitch too small": (desc(dst_pitch=3 * W - 1),) + good,
        "pitch too small for two panels": (desc(panels=2, dst_pitch=3 * (2 * W + 15) - 1),) + good,
        "n_colors > 256": (desc(n_colors=257),) + good,
        "n_colors < 0": (desc(n_colors=-1),) + good,
        "null image": (desc(), None) + good[1:],
        "null composite": (desc(),) + good[:4] + (None, good[5]),
        "null map list": (desc(), good[0], None) + good[2:],
        "null second map": (desc(panels=2, dst_pitch=1 << 12), good[0], holes) + good[2:],
        "null palette": (desc(),) + good[:2] + (None,) + good[3:],
        "ids without a table": (desc(write_ids=1),) + good[:3] + (None,) + good[4:],
        "ids without an output": (desc(write_ids=1),) + good[:5] + (None,),
        "nothing to do": (desc(panels=0),) + good,
    }
    for name, args in cases.items():
        d = args[0]
        status = h.fs_render_prediction(K._stream(), ctypes.byref(d) if d is not None else None, *args[1:])
        msg = h.fs_last_error()
        assert status != 0 and msg and b"fs_render_prediction" in msg, (name, status, msg)
    torch.cuda.synchronize()
    assert bool((comp == SENTINEL).all()) and bool((ids == SENTINEL).all())            # nothing was launched
    assert h.fs_render_prediction(K._stream(), ctypes.byref(desc()), *good) == 0
    torch.cuda.synchronize()
    assert not bool((comp == SENTINEL).any())


# ---- 7. SegTester and SegEvaluator end to end -------------------------------------------------------------------------------------
_NET = {}


def student():
    if not _NET:
        from fasterseg_amd import archs
        from oracle.seeded import seeded_state
        net = archs.build_derived(1, training=False, lasts=[2, 1])
        net.load_state_dict(seeded_state(net.state_dict(), 12345))
        _NET["net"] = net.cuda().eval()
    return _NET["net"]


def frames(n, H=256, W=512, seed=11):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        base = rng.randint(0, 256, size=(H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
        img = np.clip(np.kron(base, np.ones((16, 16, 1)))[:H, :W] + rng.randint(-40, 41, size=(H, W, 3)), 0, 255).astype(np.uint8)
        lab = rng.randint(0, 19, size=(H, W)).astype(np.uint8)
        lab[rng.rand(H, W) < 0.05] = 255
        out.append({"data": img, "label": lab, "fn": "frame_%02d" % i})
    return out


def confusion(pred, lab, n=19):
    keep = lab < n
    return np.bincount(n * lab[keep].astype(np.int64) + pred[keep], minlength=n * n).reshape(n, n)


@pytest.mark.gpu
def test_seg_tester_and_evaluator_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    from fasterseg_amd import visualize as V
    from fasterseg_amd.evaluator import SegEvaluator
    from fasterseg_amd.tester import SegTester
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")            # one fixed plan for every engine, as tests/test_ms_eval_gpu.py
    monkeypatch.setenv("FS_ENGINE_FUSE_CELLS", "1")
    net = student()
    spec = V.LabelSpec.from_json(os.path.join(GOLD, "cityscapes_labels.json"))
    data = frames(5)
    # the evaluator with every new argument at its default: today's path, no writer
    plain = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), save_path=None, show_image=False, show_prediction=False, labels=None)
    preds = [plain.func_per_iteration(d).cpu().numpy() for d in data]
    assert plain._writer is None and not plain._states and not os.listdir(tmp_path)
    metric = plain.compute_metric()
    assert np.array_equal(metric["hist"], sum(confusion(p, d["label"]) for p, d in zip(preds, data)))
    assert len({p.tobytes() for p in preds}) == 5 and any(len(np.unique(p)) > 1 for p in preds)
    # SegTester: 5 frames through 2 slots
    out = tmp_path / "test_1_0"
    tester = SegTester(net, 19, MEAN, STD, spec, save_dir=str(out), show_prediction=True, slots=2, workers=2, image_shape=(256, 512))
    got = tester.run_online(data)
    tester.close()
    assert sorted(os.listdir(out)) == sorted([d["fn"] + e for d in data for e in (".png", ".viz.png")])
    assert np.array_equal(got["hist"], metric["hist"]) and got["mean_IU"] == metric["mean_IU"]
    for d, p in zip(data, preds):
        ids, viz = Image.open(out / (d["fn"] + ".png")), Image.open(out / (d["fn"] + ".viz.png"))
        assert ids.mode == "L" and viz.mode == "RGB"
        assert np.array_equal(np.asarray(ids), spec.lut[p])
        assert np.array_equal(np.asarray(viz), R.show_prediction(spec.palette, spec.background, d["data"], p))
    # SegEvaluator(show_image=True): the strip per frame, the metric unchanged
    strips = tmp_path / "strips"
    show = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), save_path=str(strips), show_image=True, labels=spec)
    assert show._writer is None
    for d in data[:2]:
        show.func_per_iteration(d)
    show.finish_writing()
    assert sorted(os.listdir(strips)) == [d["fn"] + ".png" for d in data[:2]]
    for d, p in zip(data[:2], preds):
        strip = Image.open(strips / (d["fn"] + ".png"))
        assert strip.mode == "RGB" and np.array_equal(np.asarray(strip), R.show_img(spec.palette, spec.background, d["data"], d["label"], p))
    two = show.compute_metric()
    assert np.array_equal(two["hist"], sum(confusion(p, d["label"]) for p, d in zip(preds[:2], data[:2])))
    # save_path alone: the raw class map
    raw = SegEvaluator(net, 19, MEAN, STD, image_shape=(256, 512), save_path=str(tmp_path / "raw"))
    raw.func_per_iteration(data[0])
    raw.finish_writing()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "raw" / (data[0]["fn"] + ".png"))), preds[0])
