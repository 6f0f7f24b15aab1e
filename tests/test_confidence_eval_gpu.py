"""SegEvaluator.predict and tester.PseudoLabeler on 128 x 256 frames, in every mode the evaluator has: with min_confidence=0 the class map
is the one the existing method of the mode returns for the same image, and the confidence byte is the fp64 share of the maximum in the
score buffer the mode leaves (canvas / total read back; tests/_confidence_ref.score_reference) - or, in the single-pass modes, inside the
bound of tests/_confidence_ref.reference on the engine's own head_logits."""
import gc
import os

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


H, W = 128, 256
_cache = {}


def _fixed_plan(monkeypatch):
    for k, v in (("FS_ENGINE_AUTOTUNE", "0"), ("FS_ENGINE_FUSE_CELLS", "1"), ("FS_ENGINE_FOLD_RESIZE", "0"), ("FS_ENGINE_FUSE_HEAD", "2")):
        monkeypatch.setenv(k, v)


def _student(seed=12345):
    if seed not in _cache:
        from fasterseg_amd import archs
        from oracle.seeded import seeded_state
        net = archs.build_derived(1, training=False)
        net.load_state_dict(seeded_state(net.state_dict(), seed))
        _cache[seed] = net.cuda().eval()
    return _cache[seed]


def _evaluator(**kw):
    from fasterseg_amd.evaluator import SegEvaluator
    with torch.no_grad():
        return SegEvaluator(_student(), 19, U.MEAN, U.STD, image_shape=(H, W), **kw)


def _score_check(score, classes, conf, what):
    t, tol, cls = CR.score_reference(score.cpu().numpy(), 19)
    q = conf.cpu().numpy().astype(np.float64)
    print("%s: max |q - t| = %.4f, q in %d..%d" % (what, np.abs(q - t).max(), q.min(), q.max()))
    bad = np.abs(q - t) > tol
    assert not bad.any(), "%s: %d of %d confidence bytes outside the bound" % (what, bad.sum(), bad.size)
    assert (classes.cpu().numpy() == cls).all()
    assert len(np.unique(q)) > 1


@pytest.mark.parametrize("uint8_input", [False, True], ids=["float", "uint8"])
def test_plain_mode(uint8_input, monkeypatch):
    _fixed_plan(monkeypatch)
    ev = _evaluator(uint8_input=uint8_input)
    img = U.frame(1, H, W, 31)[0]
    want = ev.whole_eval(img).clone()
    classes, conf = (t.clone() for t in ev.predict(img))
    assert tuple(classes.shape) == tuple(conf.shape) == (H, W) and conf.dtype == torch.uint8
    assert torch.equal(classes, want), "%d pixels differ from whole_eval" % int((classes != want).sum())
    eng = list(ev._conf_engines.values())[0]
    assert eng.input_mode == ("uint8" if uint8_input else "float") and eng.output_mode == "classes+confidence"
    buf = np.ascontiguousarray(eng.head_logits.permute(0, 2, 3, 1).float().cpu().numpy())
    ref = CR.reference(buf, 19, (H, W))
    bad = CR.failures(conf.cpu().numpy()[None], ref)
    assert not bad.any(), "%d of %d confidence bytes outside the bound" % (bad.sum(), bad.size)
    ev.predict(img)
    assert len(ev._conf_engines) == 1                     # built once, kept
    # load_weights refreshes the new engine too
    ev.load_weights(_student(54321))
    classes2, conf2 = ev.predict(img)
    assert torch.equal(classes2, ev.whole_eval(img)) and not torch.equal(conf2, conf)


@pytest.mark.parametrize("mode", ["flip", "padded", "output_size"])
def test_canvas_modes(mode, monkeypatch):
    _fixed_plan(monkeypatch)
    ev = _evaluator(is_flip=(mode == "flip"))
    img = U.frame(1, H, W, 32)[0]
    kw = {"flip": {}, "padded": dict(input_size=(160, 288)), "output_size": dict(output_size=(96, 200))}[mode]
    want = ev.whole_eval(img, **kw).clone()
    classes, conf = ev.predict(img, **kw)
    assert torch.equal(classes, want), "%d pixels differ from whole_eval" % int((classes != want).sum())
    st = ev._states[(H, W)]
    score = st.outputs[(96, 200)][0] if mode == "output_size" else ev._canvas(st, H, W)
    assert tuple(conf.shape) == tuple(score.shape[:2])
    _score_check(score, classes, conf, mode)
    # masked: the same bytes, the mask applied
    cut = int(conf.flatten().float().median())
    classes, conf = classes.clone(), conf.clone()
    mc, mq = ev.predict(img, min_confidence=cut / 255, ignore_label=254, **kw)
    assert torch.equal(mq, conf) and torch.equal(mc, torch.where(conf >= cut, classes, torch.full_like(classes, 254)))


def test_multi_scale(monkeypatch):
    _fixed_plan(monkeypatch)
    ev = _evaluator(multi_scales=[0.75, 1.0], crop_size=128)
    img = U.frame(1, H, W, 33)[0]
    want = ev.sliding_eval(img, 128, ev.stride_rate).clone()
    classes, conf = ev.predict(img)
    assert torch.equal(classes, want), "%d pixels differ from sliding_eval" % int((classes != want).sum())
    _score_check(ev._states[(H, W)].total, classes, conf, "multi-scale")


def test_pseudo_labeler(tmp_path, monkeypatch):
    from PIL import Image
    from fasterseg_amd.tester import PseudoLabeler
    _fixed_plan(monkeypatch)
    frames = U.frame(2, H, W, 34)
    probe = _evaluator()
    cut = int(probe.predict(frames[0])[1].flatten().float().median())          # about half of the pixels are kept
    out = tmp_path / "labels"
    maps = []

    class Recording(PseudoLabeler):          # (a subclass, not a function stored on the instance: that would be a reference cycle
        def func_per_iteration(self, data):  # holding the labeler's engines until some later garbage collection)
            out_ = super().func_per_iteration(data)
            maps.append(tuple(t.cpu().numpy().copy() for t in out_))
            return out_
    with torch.no_grad():
        pl = Recording(_student(), 19, U.MEAN, U.STD, str(out), min_confidence=cut / 255, save_confidence=True, image_shape=(H, W))

    def dataset():
        for i in range(2):
            yield {"data": frames[i], "fn": "frame%d" % i}
    stats = pl.run_online(dataset())
    pl.close()
    assert sorted(os.listdir(out)) == ["frame0.conf.png", "frame0.png", "frame1.conf.png", "frame1.png"]
    kept = np.zeros(19, dtype=np.int64)
    for i, (classes, conf) in enumerate(maps):
        png = np.asarray(Image.open(out / ("frame%d.png" % i)))
        cpng = np.asarray(Image.open(out / ("frame%d.conf.png" % i)))
        assert png.dtype == np.uint8 and png.shape == (H, W) and (png == classes).all() and (cpng == conf).all()
        assert ((classes == 255) == (conf < cut)).all()
        kept += np.bincount(classes[classes != 255], minlength=19)[:19]
    assert stats["frames"] == 2 and (stats["per_class"] == kept).all() and kept.sum() > 0
    assert stats["kept"] == kept.sum() / (2 * H * W) and 0.2 <= stats["kept"] <= 0.8
    # write=False: the same maps and counts, no file
    quiet = tmp_path / "quiet"
    with torch.no_grad():
        pl2 = PseudoLabeler(_student(), 19, U.MEAN, U.STD, str(quiet), min_confidence=cut / 255, write=False, image_shape=(H, W))
    stats2 = pl2.run_online(dataset())
    assert not quiet.exists() and (stats2["per_class"] == kept).all() and stats2["kept"] == stats["kept"]
