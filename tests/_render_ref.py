"""Reference arithmetic of the rendering tests: a stand-in `cv2` module for the reference's tools/utils/visualize.py (what
tests/cv2_numpy.py restates, plus addWeighted and imwrite), and numpy restatements of set_img_color / show_prediction / show_img
and of the submission's trainId -> labelId map, written against the kernel's contract (include/fasterseg_hip.h,
fs_render_prediction) rather than copied from the reference.

addWeighted restates OpenCV 4's 8-bit formula in its fp32 form with the contraction fixed - saturate(rint(fma(src1, (float)alpha,
(float)(src2 * (float)beta)) + gamma)) - emulated exactly: the product of a byte and a float is exact in float64, the second product
is rounded to float32 first, their float64 sum is exact for the weights used here and is rounded to float32 once.  It has not been
checked against a cv2 build (none is installed where the fixtures are made)."""
import types

import numpy as np

try:
    import cv2_numpy                      # pytest puts tests/ on sys.path (as the other test modules import it)
except ImportError:
    from tests import cv2_numpy

PIVOT = 15


def blend(c, o, w):
    """Bytes c (painted) and o (image), any broadcastable shapes -> the blended bytes for weight_foreground w."""
    alpha = np.float32(w)
    beta = np.float32(1.0 - w)            # the reference's (1 - weight_foreground) in double, then cv2's cast
    second = (np.asarray(o).astype(np.float32) * beta).astype(np.float32)
    s = (np.asarray(c).astype(np.float64) * np.float64(alpha) + second.astype(np.float64)).astype(np.float32)
    return np.clip(np.rint(s), 0, 255).astype(np.uint8)


def addWeighted(src1, alpha, src2, beta, gamma, dst=None):          # noqa: N802 (cv2's name)
    assert src1.dtype == np.uint8 and src2.dtype == np.uint8 and src1.shape == src2.shape
    a, b = np.float32(alpha), np.float32(beta)
    second = (src2.astype(np.float32) * b).astype(np.float32)
    s = (src1.astype(np.float64) * np.float64(a) + second.astype(np.float64)).astype(np.float32)
    if gamma:
        s = (s + np.float32(gamma)).astype(np.float32)
    out = np.clip(np.rint(s), 0, 255).astype(np.uint8)
    if dst is not None:
        dst[...] = out
        return dst
    return out


def cv2_module(written=None):
    """A module object to install as sys.modules['cv2']: tests/cv2_numpy.py's functions, addWeighted, and an imwrite that records
    (path, array) in `written` instead of encoding a file."""
    m = types.ModuleType("cv2")
    for k, v in vars(cv2_numpy).items():
        if not k.startswith("_"):
            setattr(m, k, v)
    m.addWeighted = addWeighted

    def imwrite(path, img, params=None):
        if written is not None:
            written.append((path, np.array(img)))
        return True
    m.imwrite = imwrite
    return m


def overlay(palette, background, img, classes, show255, w):
    """One overlay panel: palette (n, 3) uint8, img (H, W, 3) uint8, classes (H, W) integer."""
    palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    k = np.asarray(classes).astype(np.int64)
    painted = (k < len(palette)) & (k != background) & (k >= 0)
    c = np.where(painted[..., None], palette[np.where(painted, k, 0)], img)
    if show255:
        c = np.where((k == 255)[..., None], 0, c)
    return blend(c, img, w)


def show_prediction(palette, background, img, pred, w=1):
    return overlay(palette, background, img, pred, False, w)


def composite(palette, background, img, maps, show255, weights, image_panel, gap=PIVOT):
    """The panels side by side with `gap` black columns between them (None for no panel at all)."""
    panels = [np.asarray(img, dtype=np.uint8)] if image_panel else []
    panels += [overlay(palette, background, img, m, s, w) for m, s, w in zip(maps, show255, weights)]
    if not panels:
        return None
    out = panels[0]
    bar = np.zeros((out.shape[0], gap, 3), dtype=np.uint8)
    for p in panels[1:]:
        out = np.concatenate([out, bar, p], axis=1)
    return out


def show_img(palette, background, img, gt, *pds):
    maps = list(pds) + [gt]
    return composite(palette, background, img, maps, [False] * len(pds) + [True], [0.55] * len(maps), True)


def label_ids(lut, classes):
    return np.asarray(lut, dtype=np.uint8)[np.asarray(classes).astype(np.uint8)]
