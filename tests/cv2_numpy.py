"""A numpy restatement of the few OpenCV 4 functions the reference's training pipeline calls (tools/utils/img_utils.py,
search|train/dataloader.py TrainPre, tools/datasets/BaseDataset._open_image), usable as a stand-in `cv2` module, and the reference's
TrainPre restated on top of it.

- resize: uint8 INTER_LINEAR in 8-bit fixed point (resize.cpp: fx = (float)((dx + 0.5) * scale - 0.5), INTER_RESIZE_COEF_BITS = 11,
  HResizeLinear in int32, VResizeLinear's (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2) and INTER_NEAREST
  (resizeNN: min(cvFloor(d * (1 / inv_scale)), src - 1) in double); the scale of each axis from dsize; same size: a copy;
- flip(img, 1), copyMakeBorder(BORDER_CONSTANT).
Written from OpenCV 4's formulas; not checked against a cv2 build."""
import collections
import collections.abc
import random

import numpy as np

INTER_NEAREST, INTER_LINEAR = 0, 1
BORDER_CONSTANT = 0
IMREAD_GRAYSCALE, IMREAD_COLOR = 0, 1


def setNumThreads(n):          # noqa: N802 (cv2's name)
    pass


def linear_taps(src, dst, inv_scale):
    scale = 1.0 / inv_scale
    fx = ((np.arange(dst) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = (fx - sx.astype(np.float32)).astype(np.float32)
    fx[sx < 0] = 0
    sx[sx < 0] = 0
    fx[sx >= src - 1] = 0
    sx[sx >= src - 1] = src - 1
    c0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    return sx, np.minimum(sx + 1, src - 1), c0, c1


def nearest_taps(src, dst, inv_scale):
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * (1.0 / inv_scale)).astype(np.int64), src - 1)


def resize(img, dsize, interpolation=INTER_LINEAR):
    H, W = img.shape[:2]
    w, h = int(dsize[0]), int(dsize[1])
    if (h, w) == (H, W):
        return img.copy()
    if interpolation == INTER_NEAREST:
        return np.ascontiguousarray(img[nearest_taps(H, h, h / H)][:, nearest_taps(W, w, w / W)])
    assert interpolation == INTER_LINEAR and img.dtype == np.uint8, "only uint8 INTER_LINEAR is restated"
    y0, y1, b0, b1 = linear_taps(H, h, h / H)
    x0, x1, a0, a1 = linear_taps(W, w, w / W)
    S = img.astype(np.int64)
    if S.ndim == 2:
        S = S[:, :, None]
    D = S[:, x0] * a0[None, :, None] + S[:, x1] * a1[None, :, None]
    out = (((b0[:, None, None] * (D[y0] >> 4)) >> 16) + ((b1[:, None, None] * (D[y1] >> 4)) >> 16) + 2) >> 2
    out = np.clip(out, 0, 255).astype(np.uint8)
    return out if img.ndim == 3 else out[:, :, 0]


def flip(img, code):
    assert code == 1, "only the horizontal flip is restated"
    return np.ascontiguousarray(img[:, ::-1])


def copyMakeBorder(img, top, bottom, left, right, borderType, value=0):      # noqa: N802 (cv2's name)
    assert borderType == BORDER_CONSTANT
    pads = ((int(top), int(bottom)), (int(left), int(right))) + ((0, 0),) * (img.ndim - 2)
    return np.pad(img, pads, constant_values=value)


def area_half(img):
    """cv2's INTER_AREA 2x down-sample of uint8: (s00 + s01 + s10 + s11 + 2) >> 2."""
    H, W = img.shape[:2]
    h, w = H // 2, W // 2
    S = img[:2 * h, :2 * w].astype(np.int64)
    return ((S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2] + 2) >> 2).astype(np.uint8)


# ---- the reference's pipeline restated (img_utils.py, dataloader.py TrainPre, BaseDataset._open_image / __getitem__) ----------
def open_resize(img, down_sampling):
    """BaseDataset._open_image's down-sampling of a decoded image (3-D: INTER_LINEAR) or label (2-D: INTER_NEAREST)."""
    H, W = img.shape[:2]
    mode = INTER_LINEAR if img.ndim == 3 else INTER_NEAREST
    if isinstance(down_sampling, int):
        return resize(img, (W // down_sampling, H // down_sampling), mode)
    return resize(img, (down_sampling[1], down_sampling[0]), mode)


def pad_to(img, shape, value):
    ph, pw = max(shape[0] - img.shape[0], 0), max(shape[1] - img.shape[1], 0)
    return copyMakeBorder(img, ph // 2, ph // 2 + ph % 2, pw // 2, pw // 2 + pw % 2, BORDER_CONSTANT, value)


def train_pre(img, gt, config, mean, std, rng=random):
    """TrainPre.__call__ then BaseDataset's .float() / .long(): (p_img (3, H, W) float32, p_gt (h, w) int64, draws)."""
    draws = {}
    if rng.random() >= 0.5:
        img, gt = flip(img, 1), flip(gt, 1)
        draws["mirror"] = True
    else:
        draws["mirror"] = False
    if config.train_scale_array is not None:
        s = rng.choice(config.train_scale_array)
        sh, sw = int(img.shape[0] * s), int(img.shape[1] * s)
        img = resize(img, (sw, sh), INTER_LINEAR)
        gt = resize(gt, (sw, sh), INTER_NEAREST)
        draws["scale"] = s
    x = img.astype(np.float32) / 255.0
    x = x - mean
    x = x / std
    ch, cw = config.image_height, config.image_width
    h, w = x.shape[:2]
    ph = rng.randint(0, h - ch + 1) if h > ch else 0
    pw = rng.randint(0, w - cw + 1) if w > cw else 0
    draws["pos"] = (ph, pw)
    p_img = pad_to(x[ph:ph + ch, pw:pw + cw], (ch, cw), 0)
    p_gt = pad_to(gt[ph:ph + ch, pw:pw + cw], (ch, cw), 255)
    g = config.gt_down_sampling
    p_gt = resize(p_gt, (cw // g, ch // g), INTER_NEAREST)
    return np.ascontiguousarray(p_img.transpose(2, 0, 1)).astype(np.float32), p_gt.astype(np.int64), draws


def install_iterable_alias():
    """tools/utils/img_utils.py's get_2dshape reads collections.Iterable (removed in Python 3.10)."""
    if not hasattr(collections, "Iterable"):
        collections.Iterable = collections.abc.Iterable
