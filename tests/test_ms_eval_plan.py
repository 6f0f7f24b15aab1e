"""CPU: the host plan of multi-scale / sliding-window evaluation (fasterseg_amd.eval_plan) against a literal restatement of the
reference's scale_process grid loop and pad_image_to_shape (tools/engine/evaluator.py:228-295, tools/utils/img_utils.py:60-74),
and its tap tables against an independent restatement of cv2's 8-bit INTER_LINEAR coefficients (INTER_RESIZE_COEF_BITS = 11)."""
import math

import numpy as np
import pytest

from fasterseg_amd import eval_plan as EP


def ref_dsize(H, W, s):
    # cv2.resize(img, None, fx=s, fy=s): dsize = Size(saturate_cast<int>(W * s), saturate_cast<int>(H * s)); saturate_cast rounds
    # to nearest, ties to even
    def rnd(v):
        f = math.floor(v)
        d = v - f
        if d > 0.5 or (d == 0.5 and f % 2 == 1):
            return int(f) + 1
        return int(f)
    return rnd(H * s), rnd(W * s)


def ref_pad(rows, cols, shape):
    margin = np.zeros(4, np.uint32)
    pad_height = shape[0] - rows if shape[0] - rows > 0 else 0
    pad_width = shape[1] - cols if shape[1] - cols > 0 else 0
    margin[0] = pad_height // 2
    margin[1] = pad_height // 2 + pad_height % 2
    margin[2] = pad_width // 2
    margin[3] = pad_width // 2 + pad_width % 2
    return rows + margin[0] + margin[1], cols + margin[2] + margin[3], [int(m) for m in margin]


def ref_scale_process(new_rows, new_cols, crop_size, stride_rate):
    """The control flow of scale_process with the arrays left out: (sliding, canvas shape, margins, windows)."""
    long_size = new_cols if new_cols > new_rows else new_rows
    if long_size <= crop_size:
        pr, pc, margin = ref_pad(new_rows, new_cols, (crop_size, crop_size))
        return False, (pr, pc), margin, [(0, 0)]
    stride = int(np.ceil(crop_size * stride_rate))
    pad_rows, pad_cols, margin = ref_pad(new_rows, new_cols, (crop_size, crop_size))
    r_grid = int(np.ceil((pad_rows - crop_size) / stride)) + 1
    c_grid = int(np.ceil((pad_cols - crop_size) / stride)) + 1
    windows = []
    for grid_yidx in range(r_grid):
        for grid_xidx in range(c_grid):
            s_x = grid_xidx * stride
            s_y = grid_yidx * stride
            e_x = min(s_x + crop_size, pad_cols)
            e_y = min(s_y + crop_size, pad_rows)
            s_x = e_x - crop_size
            s_y = e_y - crop_size
            windows.append((s_y, s_x))
    return True, (pad_rows, pad_cols), margin, windows


CASES = [
    (256, 512, 256, 5 / 6, 0.5),       # exactly the crop: one padded pass
    (256, 512, 256, 5 / 6, 0.6),       # 153.6 x 307.2 -> 154 x 307, odd column pad, sliding
    (256, 512, 256, 5 / 6, 0.75),
    (256, 512, 256, 5 / 6, 1.25),      # 2 x 3 windows, the last of each pulled back to the edge
    (200, 328, 256, 5 / 6, 0.6),       # smaller than the crop: 120 x 197, odd pads split floor / ceil
    (1024, 2048, 1024, 5 / 6, 1.75),   # the Cityscapes protocol's largest scale
    (1024, 2048, 1024, 2 / 3, 1.0),
    (97, 131, 64, 0.5, 1.5),
    (1024, 2048, 1024, 5 / 6, 0.6),
]


@pytest.mark.parametrize("H,W,crop,rate,s", CASES)
def test_plan_matches_scale_process(H, W, crop, rate, s):
    (p,) = EP.scale_plan(H, W, [s], crop, rate)
    rows, cols = ref_dsize(H, W, s)
    assert (p.rows, p.cols) == (rows, cols)
    sliding, canvas, margin, windows = ref_scale_process(rows, cols, crop, rate)
    assert p.sliding == sliding
    assert (p.canvas_h, p.canvas_w) == canvas
    assert list(p.margins) == margin and (p.top, p.left) == (margin[0], margin[2])
    assert p.windows == windows
    assert p.pad_mode == (EP.PAD_UINT8 if sliding else EP.PAD_NORMALISED)
    for oy, ox in p.windows:                           # every window lies in the canvas, and together they cover it
        assert 0 <= oy and oy + crop <= p.canvas_h and 0 <= ox and ox + crop <= p.canvas_w
    cover = np.zeros((p.canvas_h, p.canvas_w), bool)
    for oy, ox in p.windows:
        cover[oy:oy + crop, ox:ox + crop] = True
    assert cover.all()


def test_plan_edge_cases_are_exercised():
    # s = 0.6 rounds: 256 * 0.6 = 153.6 -> 154 and 512 * 0.6 = 307.2 -> 307; half-way cases go to even
    assert EP.resized_size(256, 512, 0.6) == (154, 307)
    assert EP.resized_size(5, 7, 0.5) == (2, 4)        # 2.5 -> 2, 3.5 -> 4
    (p,) = EP.scale_plan(200, 328, [0.6], 256, 5 / 6)
    assert not p.sliding and p.margins == (68, 68, 29, 30)
    (p,) = EP.scale_plan(256, 512, [1.25], 256, 5 / 6)
    assert p.sliding and p.windows[-1] == (64, 384) and p.windows[1][1] == 214    # pulled back: 428 + 256 > 640
    plans = EP.scale_plan(1024, 2048, [0.5, 0.75, 1, 1.25, 1.5, 1.75], 1024, 5 / 6)
    assert [len(p.windows) for p in plans] == [1, 2, 3, 6, 8, 8] and EP.n_passes(plans, True) == 56


def ref_taps(src, dst, s):
    """cv2 resize.cpp (INTER_LINEAR, 8-bit): scale_x = 1 / inv_scale_x; per dx fx = (float)((dx + 0.5) * scale_x - 0.5),
    sx = cvFloor(fx), fx -= sx; clamp; ialpha = saturate_cast<short>((1 - fx) * 2048), saturate_cast<short>(fx * 2048)."""
    scale = 1.0 / s
    idx, coef = [], []
    for dx in range(dst):
        fx = np.float32((dx + 0.5) * scale - 0.5)
        sx = int(math.floor(fx))
        fx = np.float32(fx - np.float32(sx))
        if sx < 0:
            fx, sx = np.float32(0), 0
        if sx >= src - 1:
            fx, sx = np.float32(0), src - 1
        c0 = np.float32(np.float32(1) - fx) * np.float32(2048)
        c1 = fx * np.float32(2048)
        idx.append(sx)
        coef.append((int(np.rint(c0)), int(np.rint(c1))))
    return np.array(idx), np.array(coef)


@pytest.mark.parametrize("src,s", [(200, 0.5), (200, 0.6), (328, 0.75), (97, 1.0), (131, 1.25), (256, 1.5), (64, 1.75), (2048, 0.6)])
def test_tap_tables(src, s):
    dst = EP.cv_round(src * s)
    idx, coef = EP.linear_taps(src, dst, s)
    want_idx, want_coef = ref_taps(src, dst, s)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(coef.astype(np.int64), want_coef)
    assert (coef.astype(np.int64).sum(1) == 2048).all()
    packed = EP.pack_taps(idx, coef)
    assert packed.dtype == np.int32 and packed.shape == (dst, 2)
    np.testing.assert_array_equal(packed[:, 0], want_idx)
    np.testing.assert_array_equal(packed[:, 1] & 0xffff, want_coef[:, 0])
    np.testing.assert_array_equal(packed[:, 1] >> 16, want_coef[:, 1])
    if s == 1.0:                                       # identity taps: every pixel is itself with weight 2048
        np.testing.assert_array_equal(idx, np.arange(src))
        assert (coef[:, 0] == 2048).all()
