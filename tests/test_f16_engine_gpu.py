"""InferenceEngine / SegEvaluator / SegTester with dtype=torch.float16 on a real MI355X.

Student arch_1 (lasts=[2, 1], seeded weights and CPU oracle as tests/test_engine_gpu.py::_student) at 1x3x256x512; teacher arch_0 at
2x3x64x128 for the batch > 1 path.

  * the project's 16-bit gate against the oracle (rel <= 5e-2, arg-max agreement >= 97 %) for fuse_cells in {1, 0, auto},
    FS_ENGINE_FUSE_HEAD in {0, 2} and FS_ENGINE_FOLD_RESIZE in {0, 1};
  * the point of the type: with the fp32 engine as the yardstick, max|fp16 - fp32| <= 1/2 max|bf16 - fp32| and fp16's arg-max agreement
    >= bf16's (unit round-off 2^-11 against 2^-8 predicts about 1/8);
  * outputs ("classes", "lowres"), the uint8 input, load_weights(), plan files, and the evaluator / tester modes, where the fp16 class
    map must agree with the fp32 evaluator's at least as well as the bf16 evaluator's does."""
import os

import numpy as np
import pytest
import torch

from tests import _u8_cases as U
from tests.test_engine_gpu import _check, _student

pytestmark = pytest.mark.gpu
H16 = torch.float16
SHAPE = (1, 3, 256, 512)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def _engine(net, shape=SHAPE, **kw):
    from fasterseg_amd import engine
    with torch.no_grad():
        return engine.InferenceEngine(net, shape, **kw)


def _fixed_plan(monkeypatch):
    for k, v in (("FS_ENGINE_AUTOTUNE", "0"), ("FS_ENGINE_FUSE_CELLS", "1"), ("FS_ENGINE_FOLD_RESIZE", "0"), ("FS_ENGINE_FUSE_HEAD", "2")):
        monkeypatch.setenv(k, v)


def _stem_out(eng, run):
    """the stem's fp16 output map of a built engine after `run()`, as fp32 (N, H, W, C)"""
    op = [o for o in eng.ops if o["kind"] == "stem"][0]
    bid, off = op["out"].storage
    run()
    torch.cuda.synchronize()
    return eng.buffers[bid][..., off:off + op["out"].shape[1]].float().clone()


def _frame(h, w, seed):
    return U.frame(1, h, w, seed)[0]


@pytest.mark.parametrize("cells", ["1", "0", "auto"], ids=["fused", "split", "auto"])
def test_oracle_gate_fuse_cells(cells):
    net, x, want = _student(SHAPE)
    eng = _engine(net, dtype=H16, fuse_cells=cells)
    got = eng(x.cuda()).clone()
    assert got.dtype == torch.float32
    _check(got, want, H16, "fp16 engine, fuse_cells=%s" % cells)
    fns = [c["fn"] for c in eng.calls]
    if cells != "auto":
        assert ("fs_zoom_cell_fwd" in fns) == (cells == "1")
    described = [c for c in eng.calls if c.get("desc") is not None]
    assert len(described) >= len(eng.calls) - 1 and all(c["desc"].dtype == 2 for c in described), "a launch of another dtype"
    assert [c["args"][10] for c in eng.calls if c["fn"] == "fs_conv_stem_fwd"] == [2]                 # (the stem carries its dtype by value)
    # every way the plan can be issued
    for name, issue in (("launch list", eng._launch_all), ("launch program", eng._run_program)):
        eng.input.copy_(x.cuda())
        eng.output.zero_()
        issue()
        torch.cuda.synchronize()
        _check(eng.output.clone(), want, H16, name)


@pytest.mark.parametrize("fold", ["0", "1"], ids=["nofold", "fold"])
@pytest.mark.parametrize("head", ["0", "2"], ids=["head0", "head2"])
def test_oracle_gate_head_fusion_and_resize_folds(head, fold, monkeypatch):
    monkeypatch.setenv("FS_ENGINE_FUSE_HEAD", head)
    monkeypatch.setenv("FS_ENGINE_FOLD_RESIZE", fold)
    net, x, want = _student(SHAPE)
    eng = _engine(net, dtype=H16, fuse_cells="0")
    fns = [c["fn"] for c in eng.calls]
    assert ("fs_conv3x3_pw_fwd" in fns) == (head == "2"), "head fusion must be selectable for fp16 exactly as for bf16"
    if fold == "1":
        assert any(getattr(c.get("desc"), "vr_H", 0) > 0 for c in eng.calls), "no resample folded into a conv's staging"
    _check(eng(x.cuda()).clone(), want, H16, "FUSE_HEAD=%s FOLD_RESIZE=%s" % (head, fold))


def _three(monkeypatch=None):
    """logits of the fp32, bf16 and fp16 engines on the same weights and input (built once)"""
    if "three" not in _cache:
        net, x, _ = _student(SHAPE)
        _cache["three"] = {dt: _engine(net, dtype=dt)(x.cuda()).float().cpu().clone() for dt in (torch.float32, torch.bfloat16, H16)}
    return _cache["three"]


def test_fp16_is_closer_to_fp32_than_bf16():
    out = _three()
    ref = out[torch.float32]
    e16, eb = float((out[H16] - ref).abs().max()), float((out[torch.bfloat16] - ref).abs().max())
    a16 = float((out[H16].argmax(1) == ref.argmax(1)).float().mean())
    ab = float((out[torch.bfloat16].argmax(1) == ref.argmax(1)).float().mean())
    print("max|fp16 - fp32| %.4e, max|bf16 - fp32| %.4e, ratio %.4f; arg-max agreement fp16 %.6f bf16 %.6f" % (e16, eb, e16 / eb, a16, ab))
    assert e16 <= 0.5 * eb, (e16, eb)
    assert a16 >= ab, (a16, ab)


def test_teacher_batch_of_two():
    from fasterseg_amd import archs
    from oracle.seeded import seeded_input, seeded_state
    net = archs.build_derived(0, training=False)
    net.load_state_dict(seeded_state(net.state_dict(), 777))
    net = net.cuda().eval()
    shape = (2, 3, 64, 128)
    x = seeded_input(shape, 5).cuda()
    ref = _engine(net, shape, dtype=torch.float32)(x).float().cpu().clone()
    got = {dt: _engine(net, shape, dtype=dt)(x).float().cpu().clone() for dt in (torch.bfloat16, H16)}
    e16, eb = float((got[H16] - ref).abs().max()), float((got[torch.bfloat16] - ref).abs().max())
    print("teacher N=2: max|fp16 - fp32| %.4e, max|bf16 - fp32| %.4e" % (e16, eb))
    assert e16 / float(ref.abs().max()) <= 5e-2 and e16 <= 0.5 * eb
    assert float((got[H16].argmax(1) == ref.argmax(1)).float().mean()) >= 0.97
    assert not torch.equal(got[H16][0], got[H16][1])


def test_classes_lowres_and_logits_dtype(monkeypatch):
    from fasterseg_amd import kernels as K
    _fixed_plan(monkeypatch)
    net, x, _ = _student(SHAPE)
    xd = x.cuda()
    logits = _engine(net, dtype=H16)(xd).clone()
    classes = _engine(net, dtype=H16, output="classes")(xd).clone()
    assert classes.dtype == torch.uint8 and tuple(classes.shape) == (1, 256, 512)
    # the class-map launch blends with bilerp's fixed fma order, the logits writer with its own: equal up to ties in the last bits
    # (csrc/eval.hip); everywhere the logits' top-two margin exceeds 6 x 2^-24 x max|logit| per side the two must agree
    top = logits.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 12 * 2.0 ** -24 * float(logits.abs().max())
    assert float(clear.float().mean()) > 0.999
    assert bool((classes.long()[clear] == logits.argmax(1)[clear]).all())
    low_eng = _engine(net, dtype=H16, output="lowres")
    low = low_eng(xd)
    assert low.dtype == H16 and tuple(low.shape) == (1, 19, 32, 64)
    up = K.bilinear(low, (256, 512), out_nchw=1, channels=19)
    assert torch.equal(up, logits), float((up - logits).abs().max())
    half = _engine(net, dtype=H16, logits_dtype=H16)(xd)
    assert half.dtype == H16
    # one rounding of the fp32 logits, saturating: the fp16 NCHW writer stores what the fp32 writer would have stored, rounded
    assert torch.equal(half, logits.clamp(-65504.0, 65504.0).to(H16))
    with pytest.raises(ValueError, match="logits_dtype"):
        _engine(net, dtype=H16, logits_dtype=torch.bfloat16)


def test_uint8_input_equals_float_input_within_the_stem_bound(monkeypatch):
    """The uint8 engine normalises in the stem; the float engine is fed process_image's fp32 image.  The two stems see inputs that differ
    by fp32 roundings of the normalisation (torch may multiply by 1/255), so their fp16 stem outputs agree within the stem bound
    (1e-4 + 1e-4 |v| + 2^-11 |v|): checked on the stem's own output buffer, and the logits then meet the 16-bit gate against each other."""
    from fasterseg_amd.evaluator import SegEvaluator
    _fixed_plan(monkeypatch)
    net, _, _ = _student(SHAPE)
    img = torch.from_numpy(_frame(256, 512, 21)).cuda()
    u8 = _engine(net, dtype=H16, input="uint8", image_mean=U.MEAN, image_std=U.STD)
    flt = _engine(net, dtype=H16)
    ev = SegEvaluator.__new__(SegEvaluator)
    ev.device = torch.device("cuda")
    ev.image_mean = torch.tensor(np.asarray(U.MEAN, dtype=np.float32), device="cuda").view(1, 3, 1, 1)
    ev.image_std = torch.tensor(np.asarray(U.STD, dtype=np.float32), device="cuda").view(1, 3, 1, 1)
    x = ev.process_image(img)
    a, b = u8(img).clone(), flt(x).clone()
    assert [c["fn"] for c in u8.calls if c["family"] == "stem"] == ["fs_conv_stem_u8_infer_fwd"]
    exact = torch.from_numpy(U.expected(img.cpu().numpy()[None])).cuda()
    c = flt(exact).clone()
    assert torch.equal(a, c), "fed the exact fp32 evaluation of the contract the float engine must give the uint8 engine's bits"
    sa, sb = _stem_out(u8, lambda: u8(img)), _stem_out(flt, lambda: flt(x))
    tol = 2 * (1e-4 + (1e-4 + 2.0 ** -11) * torch.maximum(sa.abs(), sb.abs()))         # each within the stem bound of the exact value
    assert bool(((sa - sb).abs() <= tol).all()), float(((sa - sb).abs() / tol).max())
    rel = float((a - b).abs().max() / a.abs().max())
    agree = float((a.argmax(1) == b.argmax(1)).float().mean())
    print("uint8 vs process_image: rel %.3e, arg-max agreement %.6f" % (rel, agree))
    assert rel <= 5e-2 and agree >= 0.97


def test_load_weights_equals_a_fresh_engine(monkeypatch):
    from fasterseg_amd import archs
    from oracle.seeded import seeded_state
    _fixed_plan(monkeypatch)
    _, x, _ = _student(SHAPE)
    net = archs.build_derived(1, training=False, lasts=[2, 1])
    net.load_state_dict(seeded_state(net.state_dict(), 12345))
    net = net.cuda().eval()
    eng = _engine(net, dtype=H16)
    before = eng(x.cuda()).clone()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 0.02 * float(p.abs().mean() + 1e-3)).cuda())
    eng.load_weights()
    after = eng(x.cuda()).clone()
    fresh = _engine(net, dtype=H16)
    fresh.load_weights()                      # folds its BatchNorms in fs_refresh_weights as the reloaded engine did (tests/test_refresh_weights_gpu.py)
    want = fresh(x.cuda()).clone()
    assert float((after - before).abs().max()) > 1e-3
    assert torch.equal(after, want), "%d values differ, max %.3e" % (int((after != want).sum()), float((after - want).abs().max()))
    packs = [r for r in eng._refresh if r.get("dtype") is not None]
    assert packs and all(r["dtype"] in (H16, torch.float32) for r in packs) and any(r["dtype"] == H16 for r in packs)


def test_plan_file_carries_fp16_and_ignores_a_bf16_plan(tmp_path, monkeypatch):
    net, x, want = _student(SHAPE)
    monkeypatch.setenv("FS_ENGINE_PLAN", str(tmp_path / "plan.json"))
    b = _engine(net, dtype=torch.bfloat16)
    assert ".bf16." in b._plan_path and os.path.exists(b._plan_path)
    a = _engine(net, dtype=H16)
    assert a._plan_in is None, "an fp16 build replayed a plan tuned for another dtype"
    assert a._plan_path.startswith(str(tmp_path / "plan.json") + ".logits.fp16.") and os.path.exists(a._plan_path) and a._plan_path != b._plan_path
    ga = a(x.cuda()).clone()
    c = _engine(net, dtype=H16)
    assert c._plan_in is not None
    assert sorted(q["label"] + q["fn"] for q in a.calls) == sorted(q["label"] + q["fn"] for q in c.calls)
    assert torch.equal(ga, c(x.cuda()))
    _check(ga, want, H16, "fp16 engine with a plan file")
    assert sorted(os.listdir(tmp_path)) == sorted({os.path.basename(a._plan_path), os.path.basename(b._plan_path)})


MODES = {
    "single": dict(),
    "uint8": dict(uint8_input=True),
    "ms_flip": dict(multi_scales=[0.75, 1.25], is_flip=True, crop_size=128),
    "sliding": dict(crop_size=96),                    # one scale, windows of 96 x 96 over the 128 x 256 image
}


def _maps(mode, dtype):
    from fasterseg_amd.evaluator import SegEvaluator
    key = ("maps", mode, dtype)
    if key not in _cache:
        net, _, _ = _student(SHAPE)
        img = _frame(128, 256, 31)
        ev = SegEvaluator(net, 19, U.MEAN, U.STD, image_shape=(128, 256), dtype=dtype, **MODES[mode])
        if mode in ("single", "uint8"):
            out = ev.whole_eval(img)
        else:
            out = ev.sliding_eval(img, MODES[mode]["crop_size"], 5 / 6)
        _cache[key] = out.clone().cpu()
    return _cache[key]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_evaluator_class_map_agrees_with_fp32_at_least_as_well_as_bf16(mode):
    ref, m16, mb = (_maps(mode, dt) for dt in (torch.float32, H16, torch.bfloat16))
    assert m16.dtype == torch.uint8 and tuple(m16.shape) == (128, 256) and len(torch.unique(m16)) > 1
    a16, ab = float((m16 == ref).float().mean()), float((mb == ref).float().mean())
    print("%s: class-map agreement with the fp32 evaluator: fp16 %.6f, bf16 %.6f" % (mode, a16, ab))
    assert a16 >= ab, (mode, a16, ab)


def test_tester_writes_the_fp32_label_png_where_the_maps_agree(tmp_path):
    from fasterseg_amd import visualize as V
    from fasterseg_amd.tester import SegTester
    net, _, _ = _student(SHAPE)
    img = _frame(128, 256, 31)
    spec = V.LabelSpec.from_json(os.path.join(GOLD, "cityscapes_labels.json"))
    out = {}
    for name, dt in (("fp32", torch.float32), ("fp16", H16)):
        t = SegTester(net, 19, U.MEAN, U.STD, spec, save_dir=str(tmp_path / name), image_shape=(128, 256), dtype=dt)
        pred = t.func_per_iteration({"data": img, "label": None, "fn": "frame"}).clone().cpu()
        t.close()
        files = sorted(f for f in os.listdir(tmp_path / name) if f.endswith(".png"))
        assert files, "no PNG written"
        out[name] = (pred, files)
    same = out["fp32"][0] == out["fp16"][0]
    assert float(same.float().mean()) >= 0.97
    assert out["fp32"][1] == out["fp16"][1] == ["frame.png"]
    from PIL import Image
    a = np.asarray(Image.open(os.path.join(str(tmp_path / "fp32"), "frame.png")))
    b = np.asarray(Image.open(os.path.join(str(tmp_path / "fp16"), "frame.png")))
    assert a.shape == (128, 256) and a.shape == b.shape and len(np.unique(a)) > 1
    m = same.numpy()
    assert np.array_equal(a[m], b[m])
