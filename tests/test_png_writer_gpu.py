"""GPU: PredictionWriter(device_png=True) and the two public paths that pass the keyword on.  The same frames are written with the host
encoder and with the device's; the files must decode to identical arrays, the device-written ones must carry exactly the reference
encoder's stream, dataloader.py must read them, and flush / close / a worker's exception behave as on the host path."""
import gc
import os

import numpy as np
import pytest
import torch

from tests import _png_ref as R
from tests import _u8_cases as U

pytestmark = pytest.mark.gpu
H, W = 128, 256
_cache = {}


@pytest.fixture(autouse=True)
def _release_engines():
    yield
    gc.collect()
    torch.cuda.synchronize()


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


def _open(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.mode, np.asarray(im).copy()


def _idat(path):
    data = open(path, "rb").read()
    at = data.index(b"IDAT")
    return data[at + 4:at + 4 + int.from_bytes(data[at - 4:at], "big")]


def _maps(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [np.repeat(np.repeat(rng.integers(0, 19, (h // 8 + 1, w // 16 + 1), dtype=np.uint8), 8, axis=0), 16, axis=1)[:h, :w].copy() for _ in range(n)]


def test_prediction_writer_on_rendered_maps(tmp_path):
    """Seven submissions through two slots, each a class map, a confidence-like noise map and an RGB picture, at two sizes (a slot grows)."""
    from fasterseg_amd import kernels as K
    from fasterseg_amd.tester import PredictionWriter, save_png
    rng = np.random.default_rng(11)
    jobs = []
    for i in range(7):
        h, w = ((37, 259), (64, 517))[i % 2]
        jobs.append((i, _maps(1, h, w, i)[0], rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)))
    for mode in (False, True):
        out = tmp_path / ("device" if mode else "host")
        os.makedirs(out)
        encoded = []

        def encode(path, array):
            encoded.append(array.shape)
            save_png(path, array)
        with PredictionWriter(slots=2, workers=2, device="cuda", device_png=mode, encode=encode) as wr:
            for i, cls, conf, pic in jobs:
                dev = [torch.from_numpy(x).cuda() for x in (cls, conf, pic)]
                outputs = [(str(out / ("%d.png" % i)), cls.shape), (str(out / ("%d.conf.png" % i)), conf.shape), (str(out / ("%d.viz.png" % i)), pic.shape)]
                wr.submit(outputs, lambda views, dev=dev: [v.copy_(d) for v, d in zip(views, dev)])
                if i == 3:
                    wr.flush()                                   # every file submitted so far is on disk
                    assert sorted(os.listdir(out)) == sorted("%d%s.png" % (j, e) for j in range(4) for e in ("", ".conf", ".viz"))
        assert len(os.listdir(out)) == 21
        # no worker deflates an (H, W) map on the device path: the host encoder saw the pictures only
        assert sorted(set(len(s) for s in encoded)) == ([3] if mode else [2, 3]) and len(encoded) == (7 if mode else 21)
    for i, cls, conf, pic in jobs:
        for name, want, kind in (("%d.png" % i, cls, "L"), ("%d.conf.png" % i, conf, "L"), ("%d.viz.png" % i, pic, "RGB")):
            host, device = _open(tmp_path / "host" / name), _open(tmp_path / "device" / name)
            assert host[0] == device[0] == kind and np.array_equal(host[1], want) and np.array_equal(device[1], want), name
        for name, want in (("%d.png" % i, cls), ("%d.conf.png" % i, conf)):      # (the picture is PIL's file on both paths)
            assert np.array_equal(R.read_png(open(tmp_path / "device" / name, "rb").read()), want)
        for name, want in (("%d.png" % i, cls), ("%d.conf.png" % i, conf)):
            assert _idat(tmp_path / "device" / name) == R.zstream(want, K.png_rows_per_band(*want.shape)), name
    with pytest.raises(RuntimeError, match="closed"):
        wr.submit([], lambda views: None)


def test_worker_exception_surfaces(tmp_path):
    from fasterseg_amd.tester import PredictionWriter
    cls = torch.from_numpy(_maps(1, 16, 48, 0)[0]).cuda()
    wr = PredictionWriter(slots=1, workers=1, device="cuda", device_png=True)
    wr.submit([(str(tmp_path / "missing" / "a.png"), (16, 48))], lambda views: views[0].copy_(cls))
    with pytest.raises(FileNotFoundError):
        wr.flush()
    wr.submit([(str(tmp_path / "b.png"), (16, 48))], lambda views: views[0].copy_(cls))      # the slot came back, the writer goes on
    wr.flush()
    assert np.array_equal(_open(tmp_path / "b.png")[1], cls.cpu().numpy())
    wr.submit([(str(tmp_path / "missing" / "c.png"), (16, 48))], lambda views: views[0].copy_(cls))
    with pytest.raises(FileNotFoundError):
        wr.close()

    def broken(views):
        raise KeyError("render failed")
    with PredictionWriter(slots=1, workers=1, device="cuda", device_png=True) as wr2:
        with pytest.raises(KeyError):
            wr2.submit([(str(tmp_path / "d.png"), (16, 48))], broken)
        wr2.submit([(str(tmp_path / "e.png"), (16, 48))], lambda views: views[0].copy_(cls))   # the slot was given back
    assert os.path.exists(tmp_path / "e.png") and not os.path.exists(tmp_path / "d.png")


def test_seg_tester_files(tmp_path, monkeypatch):
    from fasterseg_amd import visualize as V
    from fasterseg_amd.tester import SegTester
    from _util import GOLD
    _fixed_plan(monkeypatch)
    spec = V.LabelSpec.from_json(os.path.join(GOLD, "cityscapes_labels.json"))
    frames = U.frame(3, H, W, 21)
    data = [{"data": frames[i], "label": None, "fn": "frame%d" % i} for i in range(3)]
    preds = {}
    for mode in (False, True):
        out = tmp_path / ("device" if mode else "host")
        with torch.no_grad():
            tester = SegTester(_student(), 19, U.MEAN, U.STD, spec, save_dir=str(out), show_prediction=True, slots=2, workers=2,
                               device_png=mode, image_shape=(H, W))
        assert tester.writer.device_png is mode
        preds[mode] = [tester.func_per_iteration(d).cpu().numpy() for d in data]
        tester.writer.flush()
        tester.close()
        assert sorted(os.listdir(out)) == sorted(d["fn"] + e for d in data for e in (".png", ".viz.png"))
    for i, d in enumerate(data):
        assert np.array_equal(preds[False][i], preds[True][i])
        for ext, kind in ((".png", "L"), (".viz.png", "RGB")):
            host, device = _open(tmp_path / "host" / (d["fn"] + ext)), _open(tmp_path / "device" / (d["fn"] + ext))
            assert host[0] == device[0] == kind and np.array_equal(host[1], device[1])
        assert np.array_equal(_open(tmp_path / "device" / (d["fn"] + ".png"))[1], spec.lut[preds[True][i]])
    assert len({p.tobytes() for p in preds[True]}) == 3 and any(len(np.unique(p)) > 1 for p in preds[True])


def test_pseudo_labeler_files_and_the_loader_reads_them(tmp_path, monkeypatch):
    from PIL import Image
    from fasterseg_amd.dataloader import FileListSource
    from fasterseg_amd.tester import PseudoLabeler
    _fixed_plan(monkeypatch)
    frames = U.frame(2, H, W, 34)
    maps = {}
    for mode in (False, True):
        out = tmp_path / ("device" if mode else "host")
        with torch.no_grad():
            pl = PseudoLabeler(_student(), 19, U.MEAN, U.STD, str(out), min_confidence=0.3, save_confidence=True, device_png=mode, image_shape=(H, W))
        assert pl.writer.device_png is mode
        maps[mode] = [tuple(t.cpu().numpy().copy() for t in pl.func_per_iteration({"data": frames[i], "fn": "frame%d" % i})) for i in range(2)]
        stats = pl.run_online([])
        pl.close()
        assert stats["frames"] == 2
        assert sorted(os.listdir(out)) == ["frame0.conf.png", "frame0.png", "frame1.conf.png", "frame1.png"]
    for i in range(2):
        classes, conf = maps[True][i]
        assert np.array_equal(classes, maps[False][i][0]) and np.array_equal(conf, maps[False][i][1])
        assert len(np.unique(classes)) > 1 and len(np.unique(conf)) > 8
        for name, want in (("frame%d.png" % i, classes), ("frame%d.conf.png" % i, conf)):
            host, device = _open(tmp_path / "host" / name), _open(tmp_path / "device" / name)
            assert host[0] == device[0] == "L" and np.array_equal(host[1], want) and np.array_equal(device[1], want)
    # the label format dataloader.py reads: the device-written files as the ground truth of a file list
    for i in range(2):
        Image.fromarray(frames[i]).save(tmp_path / ("img%d.png" % i))
    with open(tmp_path / "list.txt", "w") as f:
        f.write("".join("img%d.png device/frame%d.png\n" % (i, i) for i in range(2)))
    source = FileListSource(str(tmp_path), str(tmp_path), str(tmp_path / "list.txt"))
    for i in range(2):
        img, lbl = source.get(i)
        assert np.array_equal(lbl.cpu().numpy(), maps[True][i][0]) and np.array_equal(img.cpu().numpy(), frames[i])
