"""GPU: training batches on the device (fs_train_batch, fs_resize_u8, fasterseg_amd.dataloader) against the reference's TrainPre and
BaseDataset._open_image restated in numpy (tests/cv2_numpy.py).  Images are compared bit for bit (torch.equal on fp32), labels
exactly.  The 8-bit resize restates OpenCV 4's formulas; it has not been checked against a cv2 build."""
import ctypes
import random

import numpy as np
import pytest
import torch

import cv2_numpy as cv

pytestmark = pytest.mark.gpu

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])


class Cfg:
    def __init__(self, h, w, g=1, scales=(0.75, 1, 1.25), batch=2, niters=2, d=1):
        self.image_height, self.image_width, self.gt_down_sampling = h, w, g
        self.train_scale_array = None if scales is None else list(scales)
        self.image_mean, self.image_std = MEAN, STD
        self.batch_size, self.niters_per_epoch, self.down_sampling = batch, niters, d


def rand_pair(seed, H, W):
    rs = np.random.RandomState(seed)
    gt = rs.randint(0, 19, (H, W)).astype(np.uint8)
    gt[rs.rand(H, W) < 0.05] = 255
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8), gt


def check(got_img, got_gt, want_img, want_gt, what):
    want_img, want_gt = torch.from_numpy(want_img), torch.from_numpy(want_gt)
    assert got_img.dtype == torch.float32 and got_gt.dtype == torch.int64
    gi, gg = got_img.cpu(), got_gt.cpu()
    assert gi.shape == want_img.shape and gg.shape == want_gt.shape, what
    if not torch.equal(gi, want_img):
        bad = (gi != want_img).nonzero()
        raise AssertionError("%s: %d image elements differ, first %s: %r vs %r" % (what, len(bad), bad[0].tolist(),
                                                                                 float(gi[tuple(bad[0])]), float(want_img[tuple(bad[0])])))
    assert torch.equal(gg, want_gt), "%s: %d label elements differ" % (what, int((gg != want_gt).sum()))


@pytest.mark.parametrize("g", [1, 8])
def test_train_batch_bit_exact_over_the_grid(g):
    from fasterseg_amd.dataloader import _Batcher
    from fasterseg_amd import train_plan as tp
    crop_h, crop_w = 48, 64
    bt = _Batcher(crop_h, crop_w, g, MEAN, STD, "cuda")
    sizes = [(60, 90), (37, 53), (48, 64), (33, 45), (97, 130)]
    sources = [rand_pair(10 + i, *s) for i, s in enumerate(sizes)]
    dev = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in sources]
    cases = 0
    for scale in (0.75, 1, 1.25, 0.6, 1.37, None):
        for mirror in (0.1, 0.9):
            for edge in ("min", "max"):
                draws, want, idx = [], [], []
                for k, (H, W) in enumerate(sizes):       # a batch mixing source sizes: crops smaller and larger than the scaled image
                    class R:
                        pass
                    r = R()
                    r.random = lambda m=mirror: m
                    r.choice = lambda seq, s=scale: s
                    r.randint = lambda a, b, e=edge: b if e == "max" else (a + b) // 3
                    cfg = Cfg(crop_h, crop_w, g, scales=None if scale is None else [scale])
                    d = tp.draw_sample(r, H, W, crop_h, crop_w, cfg.train_scale_array)
                    draws.append(d)
                    wi, wg, _ = cv.train_pre(sources[k][0], sources[k][1], cfg, MEAN, STD, r)
                    want.append((wi, wg))
                imgs, target = bt.run(draws, [s[0] for s in dev], [s[1] for s in dev])
                for k in range(len(sizes)):
                    check(imgs[k], target[k], want[k][0], want[k][1], "scale %s mirror %s edge %s size %s g %d" % (
                        scale, mirror, edge, sizes[k], g))
                    cases += 1
    assert cases == 6 * 2 * 2 * len(sizes)


@pytest.mark.parametrize("ds", [1, 2, (30, 44), 3])
def test_resize_u8_matches_open_image(ds):
    from fasterseg_amd.dataloader import ArraySource
    img, gt = rand_pair(7, 62, 90)
    src = ArraySource([img], [gt], down_sampling=ds)
    got_i, got_g = src.get(0)
    want_i, want_g = cv.open_resize(img, ds), cv.open_resize(gt, ds)
    assert src.size(0) == want_g.shape
    assert torch.equal(got_i.cpu(), torch.from_numpy(want_i)) and torch.equal(got_g.cpu(), torch.from_numpy(want_g))
    host = ArraySource([img], [gt], down_sampling=ds, resident=False)
    hi, hg = host.get(0)
    assert torch.equal(hi.cpu(), torch.from_numpy(want_i)) and torch.equal(hg.cpu(), torch.from_numpy(want_g))


def test_trainpre_under_random_seed_equals_the_reference():
    from fasterseg_amd.dataloader import TrainPre
    for k, (cfg, ds) in enumerate([(Cfg(64, 128, 1, scales=[0.5, 0.75, 1, 1.25, 1.5, 1.75]), 1),
                                   (Cfg(32, 64, 8, scales=[0.5, 0.75, 1, 1.25, 1.5]), 2),
                                   (Cfg(40, 56, 8, scales=None), (50, 70))]):
        img, gt = rand_pair(30 + k, 96, 160)
        img_l, gt_l = cv.open_resize(img, ds), cv.open_resize(gt, ds)
        pre = TrainPre(cfg, MEAN, STD)
        for seed in range(6):
            random.seed(seed)
            p_img, p_gt, extra = pre(img_l, gt_l)
            state = random.getstate()
            random.seed(seed)
            w_img, w_gt, _ = cv.train_pre(img_l, gt_l, cfg, MEAN, STD)
            assert extra is None and random.getstate() == state
            check(p_img, p_gt, w_img, w_gt, "config %d seed %d" % (k, seed))


def _source(n=5, H=70, W=100, ds=1):
    from fasterseg_amd.dataloader import ArraySource
    pairs = [rand_pair(50 + i, H, W) for i in range(n)]
    return ArraySource([p[0] for p in pairs], [p[1] for p in pairs], down_sampling=ds), pairs


def test_loader_reproducible_shapes_and_out():
    from fasterseg_amd.dataloader import DeviceTrainLoader, get_train_loader
    cfg = Cfg(48, 64, 8, batch=3, niters=4)
    src, pairs = _source()
    a = list(DeviceTrainLoader(cfg, src, seed=5))
    b = list(get_train_loader(cfg, src, seed=5))
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x["data"].dtype == torch.float32 and tuple(x["data"].shape) == (3, 3, 48, 64)
        assert x["label"].dtype == torch.int64 and tuple(x["label"].shape) == (3, 6, 8)
        assert torch.equal(x["data"], y["data"]) and torch.equal(x["label"], y["label"])
    c = list(get_train_loader(cfg, src, seed=6))
    assert not all(torch.equal(x["data"], y["data"]) for x, y in zip(a, c))
    # the first batch restated: epoch order and augmentation draws from the loader's documented generators
    ld = DeviceTrainLoader(cfg, src, seed=5)
    order = ld.epoch_share(0)
    rng = random.Random(5 * 65537)
    for k in range(3):
        w_img, w_gt, _ = cv.train_pre(*pairs[int(order[k])], cfg, MEAN, STD, rng)
        check(a[0]["data"][k], a[0]["label"][k], w_img, w_gt, "loader sample %d" % k)
    # out= writes in place
    imgs = torch.full((3, 3, 48, 64), 7.0, device="cuda")
    tgt = torch.full((3, 6, 8), 7, dtype=torch.int64, device="cuda")
    batch = ld.next_batch(out=(imgs, tgt))
    assert batch["data"].data_ptr() == imgs.data_ptr() and batch["label"].data_ptr() == tgt.data_ptr()
    assert torch.equal(imgs, a[0]["data"]) and torch.equal(tgt, a[0]["label"])


def test_loader_ranks_take_disjoint_shares():
    from fasterseg_amd import train_plan as tp
    from fasterseg_amd.dataloader import DeviceTrainLoader
    cfg = Cfg(32, 32, 1, batch=2, niters=3)
    src, _ = _source(n=7, H=40, W=40)
    shares = [DeviceTrainLoader(cfg, src, seed=1, rank=r, world=2).epoch_share(0) for r in range(2)]
    assert len(shares[0]) == len(shares[1]) == 6
    full = DeviceTrainLoader(cfg, src, seed=1, rank=0, world=2)
    assert sorted(np.concatenate(shares).tolist()) == sorted(tp.epoch_indices(7, 12, 1, 0).tolist())
    assert len(list(full)) == 3


def test_invalid_arguments_return_a_status():
    from fasterseg_amd import _lib
    h = _lib.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    pinned = torch.zeros(4096, dtype=torch.uint8).pin_memory()
    out = torch.zeros(4096, dtype=torch.float32, device="cuda")
    lbl = torch.zeros(4096, dtype=torch.int64, device="cuda")
    tab = torch.zeros(4096, dtype=torch.int32, device="cuda")
    norm = torch.zeros(768, dtype=torch.float32, device="cuda")
    s = (_lib.TrainSample * 1)(_lib.TrainSample(8, 8, 0, 8, 8, 0, 0, 0, 0, 8, 8, 0, 16, 32, 40, 0))
    ptrs = (ctypes.c_void_p * 1)(buf.data_ptr())
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(d, samples=s, images=ptrs, labels=ptrs, tables=tab):
        return h.fs_train_batch(None, ctypes.byref(d), samples, images, labels, P(tables), P(norm), P(pinned), P(buf), P(out), P(lbl))

    ok = _lib.TrainBatchDesc(1, 8, 8, 1, 48, 56, 4096)
    assert call(ok) == 0
    torch.cuda.synchronize()
    for bad, msg in [(_lib.TrainBatchDesc(1, 8, 6, 1, 48, 56, 4096), b"multiple of 4"),
                     (_lib.TrainBatchDesc(0, 8, 8, 1, 48, 56, 4096), b"batch size"),
                     (_lib.TrainBatchDesc(1, 8, 8, 3, 48, 56, 4096), b"divide"),
                     (_lib.TrainBatchDesc(1, 8, 8, 1, 4094, 56, 4096), b"outside")]:
        assert call(bad) != 0 and msg in h.fs_last_error(), (msg, h.fs_last_error())
    assert h.fs_train_batch(None, ctypes.byref(ok), s, None, ptrs, P(tab), P(norm), P(pinned), P(buf), P(out), P(lbl)) != 0
    null_src = (ctypes.c_void_p * 1)(None)
    assert call(ok, images=null_src) != 0 and b"null source" in h.fs_last_error()
    far = (_lib.TrainSample * 1)(_lib.TrainSample(8, 8, 0, 8, 8, 2, 0, 0, 0, 8, 8, 0, 16, 32, 40, 0))      # crop past the scaled image
    assert call(ok, samples=far) != 0 and b"does not fit" in h.fs_last_error()
    assert h.fs_resize_u8(None, P(buf), 8, 8, 3, P(buf), 4, 4, P(tab), P(tab), 0) != 0 and b"in-place" in h.fs_last_error()
    assert h.fs_resize_u8(None, P(buf), 8, 8, 5, P(out), 4, 4, P(tab), P(tab), 0) != 0
    torch.cuda.synchronize()


def test_student_and_supernet_steps_on_loader_batches():
    from fasterseg_amd.dataloader import DeviceTrainLoader
    from fasterseg_amd.train_step import StudentDistillStep, SupernetStep
    src, _ = _source(n=4, H=160, W=300)
    ld = DeviceTrainLoader(Cfg(128, 256, 1, scales=[0.75, 1, 1.25], batch=2, niters=1), src, seed=2)
    b = ld.next_batch()
    st = StudentDistillStep(2, 128, 256)
    loss = st.step(b["data"], b["label"])
    assert torch.isfinite(loss).all()
    # the C3 preset: 3 x 256x512 crops of 1024x2048 sources loaded at d = 2, labels at 1/8
    big, _ = _source(n=3, H=1024, W=2048, ds=2)
    ld = DeviceTrainLoader(Cfg(256, 512, 8, scales=[0.5, 0.75, 1, 1.25, 1.5], batch=3, niters=1), big, seed=3)
    b = ld.next_batch()
    assert tuple(b["label"].shape) == (3, 32, 64)
    np.random.seed(0)
    sn = SupernetStep(pretrain=True)
    out = sn.step(b["data"], b["label"])
    loss = out[0] if isinstance(out, (tuple, list)) else out
    assert torch.isfinite(torch.as_tensor(loss)).all()


def test_file_list_source_png_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from fasterseg_amd.dataloader import FileListSource
    pairs = [rand_pair(80 + i, 36, 52) for i in range(3)]
    lines = []
    for i, (img, gt) in enumerate(pairs):
        Image.fromarray(img, "RGB").save(tmp_path / ("img%d.png" % i))
        Image.fromarray(gt, "L").save(tmp_path / ("gt%d.png" % i))
        lines.append("img%d.png gt%d.png\n" % (i, i))
    (tmp_path / "train.txt").write_text("".join(lines))
    src = FileListSource(str(tmp_path), str(tmp_path), str(tmp_path / "train.txt"), down_sampling=2, portion=0.7)
    assert len(src) == 2
    for i in range(2):
        gi, gg = src.get(i)
        assert torch.equal(gi.cpu(), torch.from_numpy(cv.open_resize(pairs[i][0], 2)))
        assert torch.equal(gg.cpu(), torch.from_numpy(cv.open_resize(pairs[i][1], 2)))
