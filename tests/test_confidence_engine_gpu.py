"""InferenceEngine(output="classes+confidence"): the plan of a "classes" engine with fs_bilinear_argmax_conf as its final launch.

The seeded student at 256 x 512 under the fixed plan of tests/test_engine_u8_input_gpu.py (nothing is timed, so two engines of one
configuration get the same launches).  Per configuration: the calls equal those of a "classes" engine except the last, the class map is
that engine's bit for bit, and the confidence byte is inside the bound of tests/_confidence_ref.py computed from the engine's OWN
head_logits (the buffer its final launch read), at every pixel.  The same after load_weights with another network; a masked engine equals
the mask applied to the unmasked outputs."""
import gc

import numpy as np
import pytest
import torch

from tests import _confidence_ref as CR
from tests import _u8_cases as U

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _release_engines():
    """Engines own hipGraphs, events and side streams.  What a test leaves behind is destroyed here, at a known point with the device
    idle - not by a later cyclic garbage collection in the middle of another test's graph capture or replay."""
    yield
    gc.collect()
    torch.cuda.synchronize()


H, W = 256, 512
_cache = {}


def _fixed_plan(monkeypatch):
    for k, v in (("FS_ENGINE_AUTOTUNE", "0"), ("FS_ENGINE_FUSE_CELLS", "1"), ("FS_ENGINE_FOLD_RESIZE", "0"), ("FS_ENGINE_FUSE_HEAD", "2")):
        monkeypatch.setenv(k, v)


def _student(seed=12345):
    if ("net", seed) not in _cache:
        from fasterseg_amd import archs
        from oracle.seeded import seeded_state
        net = archs.build_derived(1, training=False)
        net.load_state_dict(seeded_state(net.state_dict(), seed))
        _cache[("net", seed)] = net.cuda().eval()
    return _cache[("net", seed)]


def _frames(n, seed, uint8):
    key = ("frame", n, seed)
    if key not in _cache:
        img = U.frame(n, H, W, seed)
        _cache[key] = (img, U.expected(img))
    img, x = _cache[key]
    return torch.from_numpy(img if uint8 else x).cuda()


def _engine(net, n, dtype, output, uint8, use_graph, **kw):
    from fasterseg_amd import engine
    if uint8:
        kw.update(input="uint8", image_mean=U.MEAN, image_std=U.STD)
    with torch.no_grad():
        return engine.InferenceEngine(net, (n, 3, H, W), dtype=dtype, output=output, use_graph=use_graph, **kw)


def _check_confidence(eng, conf, what):
    """the bytes against the fp64 reference of the logits the final launch read"""
    head = eng.head_logits
    assert head.dtype == eng.dtype and tuple(head.shape[:2]) == (conf.shape[0], 19) and head.stride(1) == 1
    buf = np.ascontiguousarray(head.permute(0, 2, 3, 1).float().cpu().numpy())
    ref = CR.reference(buf, 19, (H, W))
    q = conf.cpu().numpy()
    err = np.abs(q.astype(np.float64) - ref["t"])
    print("%s: max |q - t| = %.4f (bound %.4f), M %.2f A %.2f, q in %d..%d" % (what, err.max(), ref["tol"], ref["M"], ref["A"], q.min(), q.max()))
    bad = CR.failures(q, ref)
    assert not bad.any(), "%s: %d of %d confidence bytes outside the bound" % (what, bad.sum(), bad.size)
    assert len(np.unique(q)) > 1


CONFIGS = [("bf16", False, 1, True), ("fp32", True, 2, False), ("bf16", True, 1, False), ("fp32", False, 1, True), ("fp16", False, 1, False)]


@pytest.mark.parametrize("dtype,uint8,n,use_graph", CONFIGS, ids=["bf16-float-graph", "fp32-u8-n2", "bf16-u8", "fp32-float-graph", "fp16-float"])
def test_plan_classes_and_confidence(dtype, uint8, n, use_graph, monkeypatch):
    _fixed_plan(monkeypatch)
    net = _student()
    tdt = CR.TORCH[dtype]
    both = _engine(net, n, tdt, "classes+confidence", uint8, use_graph)
    plain = _engine(net, n, tdt, "classes", uint8, use_graph)
    assert [(c["fn"], c["label"]) for c in both.calls[:-1]] == [(c["fn"], c["label"]) for c in plain.calls[:-1]]
    last, was = both.calls[-1], plain.calls[-1]
    assert (was["fn"], last["fn"], last["family"]) == ("fs_bilinear_argmax", "fs_bilinear_argmax_conf", "resize_argmax_conf")
    assert last["bytes"] == was["bytes"] + n * H * W and last["bytes"] == (2 if dtype != "fp32" else 4) * n * 32 * 64 * 19 + 2 * n * H * W
    assert (both.graph is not None) == use_graph and not getattr(both, "use_program", False)
    x = _frames(n, 21, uint8)
    classes, conf = both(x)
    assert both.run() is both.output and both.output[0] is classes and both.output[1] is conf
    for t in (classes, conf):
        assert t.dtype == torch.uint8 and tuple(t.shape) == (n, H, W) and t.is_contiguous()
    want = plain(x)
    assert torch.equal(classes, want), "%d class-map pixels differ from the 'classes' engine" % int((classes != want).sum())
    assert len(torch.unique(classes)) > 1
    _check_confidence(both, conf, "%s n=%d" % (dtype, n))
    # another frame: the plan reads self.input
    first = conf.clone()
    classes2, conf2 = both(_frames(n, 22, uint8))
    assert not torch.equal(conf2, first) and torch.equal(classes2, plain(_frames(n, 22, uint8)))


def test_load_weights(monkeypatch):
    """After load_weights(another network) the checks of the test above hold: against a "classes" engine with the same history (built
    for the first network, reloaded with the second) bit for bit, and from the engine's own head_logits for the confidence.  Against
    FRESH engines of the second network the class map is held to the bar tests/test_refresh_weights_gpu.py holds a reloaded class map
    to: a fresh engine folds its BatchNorms on the host, a reload in fs_refresh_weights, a few ulp apart, so the two "classes" engines
    themselves differ at isolated pixels (measured here: 1 of 131 072 in fp32) - printed, and not below 97 %."""
    _fixed_plan(monkeypatch)
    net, other = _student(), _student(54321)
    x = _frames(1, 21, False)
    both = _engine(net, 1, torch.float32, "classes+confidence", False, False)
    plain = _engine(net, 1, torch.float32, "classes", False, False)
    calls = [(c["fn"], c["label"]) for c in both.calls]
    before = [t.clone() for t in both(x)]
    both.load_weights(other)
    plain.load_weights(other)
    classes, conf = (t.clone() for t in both(x))
    assert not torch.equal(conf, before[1]) and [(c["fn"], c["label"]) for c in both.calls] == calls
    want = plain(x)
    assert torch.equal(classes, want), "%d class-map pixels differ from the reloaded 'classes' engine" % int((classes != want).sum())
    _check_confidence(both, conf, "after load_weights")
    fresh = _engine(other, 1, torch.float32, "classes", False, False)
    assert [(c["fn"], c["label"]) for c in fresh.calls[:-1]] == calls[:-1]
    agree = float((classes == fresh(x)).float().mean())
    print("reloaded vs fresh engine: %.6f of the class map agrees" % agree)
    assert agree >= 0.97


def test_masked_engine(monkeypatch):
    _fixed_plan(monkeypatch)
    net = _student(54321)
    x = _frames(1, 21, False)
    classes, conf = (t.clone() for t in _engine(net, 1, torch.bfloat16, "classes+confidence", False, False)(x))
    # the threshold is the median byte of this frame, so about half the pixels keep their class
    cut = int(conf.flatten().float().median())
    kept = float((conf >= cut).float().mean())
    assert 0.25 <= kept <= 0.75 and 0 < cut < 255, (cut, kept)
    masked = _engine(net, 1, torch.bfloat16, "classes+confidence", False, False, min_confidence=cut / 255, ignore_label=254)
    assert masked.min_conf == cut and masked.calls[-1]["args"][-2:] == (cut, 254)
    mc, mq = masked(x)
    assert torch.equal(mq, conf) and torch.equal(mc, torch.where(conf >= cut, classes, torch.full_like(classes, 254)))
    assert int((mc == 254).sum()) == int((conf < cut).sum()) > 0


def test_plan_file_carries_the_output_mode(tmp_path, monkeypatch):
    _fixed_plan(monkeypatch)
    monkeypatch.setenv("FS_ENGINE_PLAN", str(tmp_path / "plan"))
    net = _student()
    x = _frames(1, 21, False)
    first = _engine(net, 1, torch.bfloat16, "classes+confidence", False, False)
    assert ".classes+confidence.bf16." in first._plan_path
    again = _engine(net, 1, torch.bfloat16, "classes+confidence", False, False)
    assert [c["fn"] for c in again.calls] == [c["fn"] for c in first.calls]
    a, b = first(x), again(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
