"""CPU: the host plan of the device training pipeline (fasterseg_amd/train_plan.py) against the reference's TrainPre restated in
tests/cv2_numpy.py and, where the reference tree is present, against the reference's own img_utils.py / search/dataloader.py run on
the numpy stand-in for cv2.  The device gather of fs_train_batch is emulated here in numpy from the plan's tables."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import pytest

import cv2_numpy as cv
from fasterseg_amd import train_plan as tp
from fasterseg_amd.eval_plan import linear_taps

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])       # config_train.py / config_search.py
SCALES = [0.5, 0.75, 1, 1.25, 1.5, 1.75]


class Cfg:
    def __init__(self, h, w, g=1, scales=SCALES, batch=2, niters=3, d=1):
        self.image_height, self.image_width, self.gt_down_sampling = h, w, g
        self.train_scale_array = scales
        self.image_mean, self.image_std = MEAN, STD
        self.batch_size, self.niters_per_epoch, self.down_sampling = batch, niters, d


def rand_pair(rs, H, W):
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8), rs.randint(0, 19, (H, W)).astype(np.uint8)


def emulate(d, img, gt, cfg, store=None):
    """fs_train_batch for one sample in numpy, from the plan's tables only (integer gathers, as the kernel does)."""
    store = store or tp.TableStore()
    gy, gx = store.label_tables(cfg.image_height, cfg.image_width, cfg.gt_down_sampling)
    ylin, xlin, ynn, xnn = store.scale_tables(d.H, d.W, d.sh, d.sw)
    T = store.array()
    ch, cw = cfg.image_height, cfg.image_width
    yp = T[ylin:ylin + 2 * d.sh].reshape(-1, 2)
    xp = T[xlin:xlin + 2 * d.sw].reshape(-1, 2)
    mir = (lambda i: d.W - 1 - i) if d.mirror else (lambda i: i)
    S = img.astype(np.int64)
    sy0 = np.clip(yp[:, 0], 0, d.H - 1)
    sy1 = np.minimum(sy0 + 1, d.H - 1)
    sx0 = np.clip(xp[:, 0], 0, d.W - 1)
    sx1 = np.minimum(sx0 + 1, d.W - 1)
    a0, a1 = (xp[:, 1] & 0xffff).astype(np.int64), ((xp[:, 1] >> 16) & 0xffff).astype(np.int64)
    b0, b1 = (yp[:, 1] & 0xffff).astype(np.int64), ((yp[:, 1] >> 16) & 0xffff).astype(np.int64)
    D = S[:, mir(sx0)] * a0[None, :, None] + S[:, mir(sx1)] * a1[None, :, None]
    u = np.clip((((b0[:, None, None] * (D[sy0] >> 4)) >> 16) + ((b1[:, None, None] * (D[sy1] >> 4)) >> 16) + 2) >> 2, 0, 255)
    norm = tp.norm_table(MEAN, STD)
    scaled = np.stack([norm[c][u[:, :, c]] for c in range(3)])                       # (3, sh, sw)
    out = np.zeros((3, ch, cw), np.float32)
    out[:, d.top:d.top + d.rows, d.left:d.left + d.cols] = scaled[:, d.pos_h:d.pos_h + d.rows, d.pos_w:d.pos_w + d.cols]
    sgt = gt[T[ynn:ynn + d.sh]][:, mir(T[xnn:xnn + d.sw])]
    pgt = np.full((ch, cw), 255, np.int64)
    pgt[d.top:d.top + d.rows, d.left:d.left + d.cols] = sgt[d.pos_h:d.pos_h + d.rows, d.pos_w:d.pos_w + d.cols]
    g = cfg.gt_down_sampling
    return out, pgt[T[gy:gy + ch // g]][:, T[gx:gx + cw // g]]


def test_draw_order_and_counts_match_restated_trainpre():
    for seed in range(60):
        H, W = 40 + seed % 7, 64 + 4 * (seed % 5)
        cfg = Cfg(32, 48, scales=[0.6, 1, 1.37] if seed % 3 else None)
        r1, r2 = random.Random(seed), random.Random(seed)
        d = tp.draw_sample(r1, H, W, cfg.image_height, cfg.image_width, cfg.train_scale_array)
        img, gt = rand_pair(np.random.RandomState(seed), H, W)
        _, _, want = cv.train_pre(img, gt, cfg, MEAN, STD, r2)
        assert d.mirror == want["mirror"] and (d.pos_h, d.pos_w) == want["pos"]
        assert d.scale == want.get("scale")
        assert r1.getstate() == r2.getstate(), "the plan consumed a different number of draws"


def test_plan_reproduces_restated_outputs():
    store = tp.TableStore()
    for seed in range(24):
        rs = np.random.RandomState(100 + seed)
        H, W = rs.randint(20, 60), rs.randint(20, 80)
        cfg = Cfg(24, 32, g=(1, 2, 4, 8)[seed % 4], scales=[0.75, 1, 1.25, 0.6, 1.37])
        img, gt = rand_pair(rs, H, W)
        d = tp.draw_sample(random.Random(seed), H, W, cfg.image_height, cfg.image_width, cfg.train_scale_array)
        want_img, want_gt, _ = cv.train_pre(img, gt, cfg, MEAN, STD, random.Random(seed))
        got_img, got_gt = emulate(d, img, gt, cfg, store)
        assert np.array_equal(got_img.view(np.uint32), want_img.view(np.uint32)), seed
        assert np.array_equal(got_gt, want_gt), seed


class _Fixed:
    """An rng whose draws are scripted."""

    def __init__(self, mirror, scale, pos_h=None, pos_w=None):
        self.r, self.s, self.pos = mirror, scale, [p for p in (pos_h, pos_w) if p is not None]

    def random(self):
        return self.r

    def choice(self, seq):
        return self.s

    def randint(self, a, b):
        return b if self.pos.pop(0) == "max" else a


def test_randint_upper_bound_pads_the_bottom_row():
    d = tp.draw_sample(_Fixed(0.9, 1, "max", "max"), 40, 60, 32, 48, [1])
    assert (d.pos_h, d.pos_w) == (9, 13) and (d.rows, d.cols) == (31, 47)
    assert (d.top, d.bottom, d.left, d.right) == (0, 1, 0, 1)
    cfg = Cfg(32, 48, scales=[1])
    img, gt = rand_pair(np.random.RandomState(1), 40, 60)
    got_img, got_gt = emulate(d, img, gt, cfg)
    assert (got_img[:, 31] == 0).all() and (got_gt[31] == 255).all() and (got_gt[:, 47] == 255).all()
    assert (got_gt[:31, :47] != 255).all()


def test_small_scaled_image_is_centred_odd_pixel_bottom_right():
    d = tp.draw_sample(_Fixed(0.1, 0.5), 41, 61, 32, 48, [0.5])
    assert (d.sh, d.sw) == (20, 30) and (d.pos_h, d.pos_w) == (0, 0)
    assert (d.top, d.bottom, d.left, d.right) == (6, 6, 9, 9)
    d = tp.draw_sample(_Fixed(0.1, 0.5), 43, 63, 32, 48, [0.5])
    assert (d.sh, d.sw) == (21, 31) and (d.top, d.bottom, d.left, d.right) == (5, 6, 8, 9)


def test_scaled_size_truncates_and_axes_have_their_own_factor():
    d = tp.draw_sample(_Fixed(0.1, 1.37, "min", "min"), 1024, 2048, 512, 1024, [1.37])
    assert (d.sh, d.sw) == (int(1024 * 1.37), int(2048 * 1.37)) == (1402, 2805)          # cvRound would give 1403, 2806
    d = tp.draw_sample(_Fixed(0.1, 0.6, "min", "min"), 37, 53, 8, 8, [0.6])
    assert (d.sh, d.sw) == (22, 31)
    store = tp.TableStore()
    ylin, xlin, _, _ = store.scale_tables(37, 53, 22, 31)
    T = store.array()
    idx, coef = linear_taps(53, 31, 31 / 53)
    assert np.array_equal(T[xlin:xlin + 62].reshape(-1, 2)[:, 0], idx)
    yidx, ycoef = linear_taps(37, 22, 22 / 37)
    assert np.array_equal(T[ylin:ylin + 44].reshape(-1, 2)[:, 0], yidx) and 22 / 37 != 31 / 53
    assert not np.array_equal(ycoef, linear_taps(37, 22, 31 / 53)[1])                        # one common factor would be wrong


def test_nearest_tables_follow_the_double_formula():
    for src, dst in [(2048, 1024), (1024, 1402), (37, 22), (53, 31), (512, 64), (448, 56), (7, 19)]:
        inv = dst / src
        want = [min(int(np.floor(x * (1.0 / inv))), src - 1) for x in range(dst)]
        assert tp.nearest_index(src, dst, inv).tolist() == want


def test_norm_table_is_bitwise_the_numpy_normalize():
    import torch
    table = tp.norm_table(MEAN, STD)
    img = np.random.RandomState(0).randint(0, 256, (17, 23, 3)).astype(np.uint8)
    x = img.astype(np.float32) / 255.0
    x = x - MEAN
    x = x / STD
    want = torch.from_numpy(np.ascontiguousarray(x)).float().numpy()
    got = np.stack([table[c][img[:, :, c]] for c in range(3)], axis=2)
    assert table.dtype == np.float32 and table.shape == (3, 256)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_exact_half_linear_is_the_area_average():
    img = np.random.RandomState(3).randint(0, 256, (38, 50, 3)).astype(np.uint8)        # exact 2x: cv2 switches to INTER_AREA
    got = cv.open_resize(img, 2)
    assert got.shape == (19, 25, 3)
    assert np.array_equal(got, cv.area_half(img))
    (h, w), (ylin, xlin), (ynn, xnn) = tp.load_tables(38, 50, 2)
    S = img.astype(np.int64)
    a0, a1, b0, b1 = xlin[:, 1] & 0xffff, xlin[:, 1] >> 16, ylin[:, 1] & 0xffff, ylin[:, 1] >> 16
    assert (a0 == 1024).all() and (a1 == 1024).all() and (b0 == 1024).all() and (b1 == 1024).all()
    D = S[:, xlin[:, 0]] * a0[None, :, None] + S[:, xlin[:, 0] + 1] * a1[None, :, None]
    u = (((b0[:, None, None] * (D[ylin[:, 0]] >> 4)) >> 16) + ((b1[:, None, None] * (D[ylin[:, 0] + 1] >> 4)) >> 16) + 2) >> 2
    assert np.array_equal(u, cv.area_half(img).astype(np.int64))


def test_mirrored_source_indices_equal_resize_of_flip():
    img = np.random.RandomState(4).randint(0, 256, (29, 45, 3)).astype(np.uint8)
    for sw in (31, 45, 61, 22):
        i0, i1, a0, a1 = cv.linear_taps(45, sw, sw / 45)
        S = img.astype(np.int64)
        Dm = S[:, 44 - i0] * a0[None, :, None] + S[:, 44 - i1] * a1[None, :, None]
        want = cv.flip(img, 1).astype(np.int64)
        Dw = want[:, i0] * a0[None, :, None] + want[:, i1] * a1[None, :, None]
        assert np.array_equal(Dm, Dw)
        assert np.array_equal(cv.resize(cv.flip(img, 1), (sw, 29)), cv.resize(img[:, ::-1].copy(), (sw, 29)))


def test_load_tables_match_open_image_resize():
    img, gt = rand_pair(np.random.RandomState(5), 45, 70)
    for ds in (2, 3, (30, 44), (45, 70)):
        plan = tp.load_tables(45, 70, ds)
        want_i, want_g = cv.open_resize(img, ds), cv.open_resize(gt, ds)
        if plan is None:
            assert want_i.shape[:2] == (45, 70)
            continue
        (h, w), (ylin, xlin), (ynn, xnn) = plan
        assert (h, w) == want_i.shape[:2] == want_g.shape
        assert np.array_equal(gt[ynn][:, xnn], want_g)


def test_rank_shares_are_disjoint_and_cover_the_epoch():
    for n, length, world in [(10, 24, 3), (7, 7, 1), (5, 12, 4), (2975, 2 * 12 * 100, 2)]:
        idx = tp.epoch_indices(n, length, seed=3, epoch=1)
        assert len(idx) == length and np.bincount(idx, minlength=n).max() - np.bincount(idx, minlength=n).min() <= 1
        shares = [tp.rank_share(idx, r, world) for r in range(world)]
        pos = np.concatenate([np.arange(r, length, world) for r in range(world)])
        assert sorted(pos.tolist()) == list(range(length))
        assert sorted(np.concatenate(shares).tolist()) == sorted(idx.tolist())
    assert np.array_equal(tp.epoch_indices(10, 24, 3, 1), tp.epoch_indices(10, 24, 3, 1))
    assert not np.array_equal(tp.epoch_indices(10, 24, 3, 1), tp.epoch_indices(10, 24, 3, 2))


def test_file_list_parsing_and_portion(tmp_path):
    lines = ["leftImg8bit/a_%d.png gtFine/a_%d_labelTrainIds.png\n" % (i, i) for i in range(10)]
    src = tmp_path / "train.txt"
    src.write_text("".join(lines))
    names = tp.read_file_list(str(src))
    assert names[3] == ("leftImg8bit/a_3.png", "gtFine/a_3_labelTrainIds.png") and len(names) == 10
    assert [n[0] for n in tp.read_file_list(str(src), 0.35)] == ["leftImg8bit/a_%d.png" % i for i in range(3)]
    assert [n[0] for n in tp.read_file_list(str(src), -0.35)] == ["leftImg8bit/a_%d.png" % i for i in range(6, 10)]


# ---- the reference's own code, on the numpy stand-in for cv2 -----------------------------------------------------------------
REFERENCE = os.environ.get("FASTERSEG_REFERENCE", "/root/reference")


@pytest.fixture
def reference_trainpre(monkeypatch):
    if not os.path.isfile(os.path.join(REFERENCE, "search", "dataloader.py")):
        pytest.skip("reference tree not present")
    cv.install_iterable_alias()
    monkeypatch.setitem(sys.modules, "cv2", cv)
    spec = importlib.util.spec_from_file_location("ref_img_utils", os.path.join(REFERENCE, "tools", "utils", "img_utils.py"))
    img_utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(img_utils)
    pkg = types.ModuleType("utils")
    pkg.img_utils = img_utils
    monkeypatch.setitem(sys.modules, "utils", pkg)
    monkeypatch.setitem(sys.modules, "utils.img_utils", img_utils)
    spec = importlib.util.spec_from_file_location("ref_search_dataloader", os.path.join(REFERENCE, "search", "dataloader.py"))
    dl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dl)
    return dl.TrainPre


def test_plan_reproduces_the_reference_trainpre(reference_trainpre):
    store = tp.TableStore()
    for seed in range(30):
        rs = np.random.RandomState(200 + seed)
        H, W = rs.randint(16, 70), rs.randint(16, 90)
        cfg = Cfg(24, 36, g=(1, 2, 4)[seed % 3], scales=None if seed % 5 == 4 else [0.5, 0.75, 1, 1.25, 1.5, 1.75, 0.6, 1.37])
        img, gt = rand_pair(rs, H, W)
        pre = reference_trainpre(cfg, MEAN, STD)
        random.seed(seed)
        p_img, p_gt, extra = pre(img, gt)
        after_ref = random.getstate()
        random.seed(seed)
        d = tp.draw_sample(random, H, W, cfg.image_height, cfg.image_width, cfg.train_scale_array)
        assert random.getstate() == after_ref and extra is None
        # the reference's crop / margins from the same state
        random.seed(seed)
        ref_mirror = random.random() >= 0.5
        assert ref_mirror == d.mirror
        got_img, got_gt = emulate(d, img, gt, cfg, store)
        import torch
        want_img = torch.from_numpy(np.ascontiguousarray(p_img)).float().numpy()
        want_gt = torch.from_numpy(np.ascontiguousarray(p_gt)).long().numpy()
        assert np.array_equal(got_img.view(np.uint32), want_img.view(np.uint32)), seed
        assert np.array_equal(got_gt, want_gt), seed
        valid = np.zeros((cfg.image_height, cfg.image_width), bool)
        valid[d.top:d.top + d.rows, d.left:d.left + d.cols] = True
        assert (p_img.transpose(1, 2, 0)[~valid] == 0).all()
