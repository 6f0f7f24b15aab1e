"""InferenceEngine(input="uint8"): the engine takes the uint8 HWC frame and its stem normalises it (fs_conv_stem_u8_fwd), and
SegEvaluator / SegTester(uint8_input=True) hand it that frame.

Only the stem's image loader differs from an input="float" engine, and for the same normalised values the two stems write the same
bits (tests/test_stem_u8_gpu.py), so every comparison here is BIT equality between the uint8 engine fed the frame and a float engine
fed the expected input (tests/_u8_cases.py: the contract evaluated in numpy float32).  Engines are built with FS_ENGINE_AUTOTUNE=0,
FS_ENGINE_FUSE_CELLS=1 and FS_ENGINE_FOLD_RESIZE=0, and with FS_ENGINE_FUSE_HEAD=2 - at its default of 1 the bf16 head fusion is the
one choice that is still timed per engine, and two engines of a pair came out with different plans: no choice is timed and both
engines of a pair get the same plan (asserted launch by launch)."""
import os

import numpy as np
import pytest
import torch

from tests import _u8_cases as U

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = 256, 512
_cache = {}


def _fixed_plan(monkeypatch):
    for k, v in (("FS_ENGINE_AUTOTUNE", "0"), ("FS_ENGINE_FUSE_CELLS", "1"), ("FS_ENGINE_FOLD_RESIZE", "0"), ("FS_ENGINE_FUSE_HEAD", "2")):
        monkeypatch.setenv(k, v)


def _student(seed=12345):
    from fasterseg_amd import archs
    from oracle.seeded import seeded_state
    net = archs.build_derived(1, training=False)
    net.load_state_dict(seeded_state(net.state_dict(), seed))
    return net.cuda().eval()


def _frames(n, seed):
    """(uint8 (n, H, W, 3) frame on the device, expected fp32 (n, 3, H, W) input on the device): host arrays built once and shared"""
    key = (n, seed)
    if key not in _cache:
        img = U.frame(n, H, W, seed)
        assert U.covers_every_byte(img)
        _cache[key] = (img, U.expected(img))
    img, x = _cache[key]
    return torch.from_numpy(img).cuda(), torch.from_numpy(x).cuda()


def _bits(t):
    t = t.contiguous()
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _pair(net, n, dtype, output, use_graph=True):
    from fasterseg_amd import engine
    kw = dict(dtype=dtype, output=output, use_graph=use_graph)
    with torch.no_grad():
        flt = engine.InferenceEngine(net, (n, 3, H, W), **kw)
        u8 = engine.InferenceEngine(net, (n, 3, H, W), input="uint8", image_mean=U.MEAN, image_std=U.STD, **kw)
    return u8, flt


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape
    assert torch.equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.numel())


CASES = [("logits", torch.float32, 1, True), ("classes", torch.bfloat16, 1, True), ("lowres", torch.bfloat16, 2, True),
         ("logits", torch.bfloat16, 1, False)]


@pytest.mark.parametrize("output,dtype,n,use_graph", CASES, ids=["logits-fp32", "classes-bf16", "lowres-bf16-n2", "logits-bf16-nograph"])
def test_uint8_engine_equals_float_engine(output, dtype, n, use_graph, monkeypatch):
    _fixed_plan(monkeypatch)
    net = _student()
    u8, flt = _pair(net, n, dtype, output, use_graph)
    # the network's view of the input is unchanged; the buffer is the frame; the stem launch is the uint8 one with its real byte count
    assert u8.input_shape == (n, 3, H, W) and tuple(u8.input.shape) == (n, H, W, 3) and u8.input.dtype == torch.uint8
    assert int(u8.input.count_nonzero()) == 0
    stems = [c for c in u8.calls if c["family"] == "stem"]
    fstems = [c for c in flt.calls if c["family"] == "stem"]
    assert [c["fn"] for c in stems] == ["fs_conv_stem_u8_fwd"] and [c["fn"] for c in fstems] == ["fs_conv_stem_fwd"]
    assert fstems[0]["bytes"] - stems[0]["bytes"] == n * H * W * 3 * 3 and "u8" in stems[0]["label"]
    assert [c["fn"] for c in u8.calls if c["family"] != "stem"] == [c["fn"] for c in flt.calls if c["family"] != "stem"]
    assert (u8.graph is not None) == use_graph
    img, x = _frames(n, 21)
    if n == 2:
        assert not torch.equal(img[0], img[1])
    first = u8(img).clone()
    _same(first, flt(x), "first frame")
    if output == "classes":
        assert first.dtype == torch.uint8 and len(torch.unique(first)) > 1
    # a second call with another frame: the plan reads self.input, not a copy taken at capture
    img2, x2 = _frames(n, 22)
    second = u8(img2).clone()
    assert not torch.equal(_bits(second), _bits(first))
    _same(second, flt(x2), "second frame")
    if n == 1:
        _same(u8(img2[0]), second, "an (H, W, 3) frame")
        _same(u8(img2.cpu().numpy()), second, "a numpy frame")
    if use_graph:                         # every way the plan can be issued: graph replay, launch list, launch program
        for name, issue in (("graph", lambda e: e.graph.replay()), ("launch list", lambda e: e._launch_all()),
                            ("launch program", lambda e: e._run_program())):
            u8.input.copy_(img)
            flt.input.copy_(x)
            outs = []
            for e in (u8, flt):
                e.output.zero_()
                issue(e)
                torch.cuda.synchronize()
                outs.append(e.output.clone())
            _same(outs[0], outs[1], name)
            _same(outs[0], first, name + " against the first call")


def test_uint8_engine_follows_load_weights(monkeypatch):
    from fasterseg_amd import engine
    _fixed_plan(monkeypatch)
    net = _student()
    img, x = _frames(1, 21)
    with torch.no_grad():
        u8 = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.float32, input="uint8", image_mean=U.MEAN, image_std=U.STD)
        before = u8(img).clone()
        g = torch.Generator().manual_seed(3)
        conv, bn = net.stem[0].conv[0], net.stem[0].conv[1]
        assert conv.weight.shape[1] == 3
        conv.weight.add_((torch.randn(conv.weight.shape, generator=g) * 0.2).cuda())
        bn.weight.mul_(1.25)
        bn.bias.add_(0.1)
        bn.running_mean.add_(0.05)
        bn.running_var.mul_(1.5)
        u8.load_weights()
        after = u8(img).clone()
        fresh = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.float32)
        built = fresh(x).clone()
        fresh.load_weights()
        want = fresh(x)
    assert float((after - before).abs().max()) > 1e-2
    # a fresh float engine folds its BatchNorms on the host, a reload folds them in fs_refresh_weights (within a few ulp of each other,
    # tests/test_refresh_weights_gpu.py): bit equality is against the fresh engine after ITS reload, the fp32 engine bar (1e-3) against
    # the fresh engine as built
    _same(after, want, "after load_weights()")
    err = float((after - built).abs().max())
    assert err <= 1e-3, "after load_weights(): logits differ from a fresh float engine by %.3e (> 1e-3)" % err


def test_refusals(monkeypatch):
    from fasterseg_amd import engine
    _fixed_plan(monkeypatch)
    net = _student()
    with pytest.raises(ValueError, match="image_mean"):
        engine.InferenceEngine(net, (1, 3, H, W), input="uint8", image_std=U.STD, use_graph=False)
    with pytest.raises(ValueError, match="image_mean"):
        engine.InferenceEngine(net, (1, 3, H, W), input="uint8", image_mean=U.MEAN, use_graph=False)
    with pytest.raises(ValueError, match="std"):
        engine.InferenceEngine(net, (1, 3, H, W), input="uint8", image_mean=U.MEAN, image_std=[0.2, 0.0, 0.2], use_graph=False)
    with pytest.raises(ValueError, match="input"):
        engine.InferenceEngine(net, (1, 3, H, W), input="bytes", use_graph=False)
    with torch.no_grad():
        u8 = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.bfloat16, output="classes", input="uint8", image_mean=U.MEAN,
                                    image_std=U.STD, use_graph=False)
    img, x = _frames(1, 21)
    out = u8(img).clone()
    launched = []
    u8.run = lambda: launched.append(1)                                         # nothing may be launched by a refused call
    for bad in (x, img.float(), img.permute(0, 3, 1, 2).contiguous(), img[:, :-1], img.cpu().numpy().astype(np.int32),
                torch.zeros((2, H, W, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="uint8 engine"):
            u8(bad)
    del u8.run
    assert not launched and torch.equal(u8.input, img)
    assert torch.equal(u8(img), out)


def test_evaluator_and_tester_take_the_frame(tmp_path, monkeypatch):
    from fasterseg_amd import engine, visualize as V
    from fasterseg_amd.evaluator import SegEvaluator
    from fasterseg_amd.tester import SegTester
    _fixed_plan(monkeypatch)
    net = _student()
    img, x = _frames(1, 21)
    with torch.no_grad():
        want = engine.InferenceEngine(net, (1, 3, H, W), dtype=torch.bfloat16, output="classes")(x)[0].clone()
    assert want.dtype == torch.uint8 and tuple(want.shape) == (H, W) and len(torch.unique(want)) > 1
    ev = SegEvaluator(net, 19, U.MEAN, U.STD, image_shape=(H, W), uint8_input=True)
    assert ev.engine.input_mode == "uint8" and ev.engine.output_mode == "classes"
    host = img[0].cpu().numpy()
    got = ev.whole_eval(host).clone()
    assert torch.equal(got, want), "numpy image: %d pixels differ" % int((got != want).sum())
    dev = img[0].contiguous()
    got = ev.whole_eval(dev).clone()
    assert torch.equal(got, want), "device tensor: %d pixels differ" % int((got != want).sum())
    # the share of class-map pixels on which today's torch chain (process_image) differs is a figure, not a bar: torch may evaluate
    # `/ 255.0` as a multiplication by the reciprocal, one ulp from the division
    plain = SegEvaluator(net, 19, U.MEAN, U.STD, image_shape=(H, W))
    assert plain.engine.input_mode == "float"
    print("process_image path: %.6f of the class-map pixels differ" % float((plain.whole_eval(host) != want).float().mean()))
    spec = V.LabelSpec.from_json(os.path.join(GOLD, "cityscapes_labels.json"))
    tester = SegTester(net, 19, U.MEAN, U.STD, spec, save_dir=str(tmp_path / "out"), write=False, image_shape=(H, W), uint8_input=True)
    got = tester.func_per_iteration({"data": host, "label": None, "fn": "frame"}).clone()
    tester.close()
    assert tester.engine.input_mode == "uint8"
    assert torch.equal(got, want), "SegTester: %d pixels differ" % int((got != want).sum())
    # a frame of another size builds its own engine on first use
    small = U.frame(1, 128, 256, 5)[0]
    got = ev.whole_eval(small)
    assert tuple(got.shape) == (128, 256) and len(ev._u8_engines) == 2
