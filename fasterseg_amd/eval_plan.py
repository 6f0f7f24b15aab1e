"""Host-side plan of multi-scale / sliding-window evaluation (tools/engine/evaluator.py:228-295 sliding_eval / scale_process,
tools/utils/img_utils.py:60-74 pad_image_to_shape), pure Python + numpy so it can be checked without a GPU.

For an (H, W) image, a crop size and a stride rate, `scale_plan` returns per scale what the device kernels of fasterseg_amd.evaluator
need: the resized size cv2.resize(img, None, fx=s, fy=s) produces, the padded canvas, its margins, the pad mode, the window origins
and cv2's fixed-point bilinear tap tables (INTER_LINEAR on uint8, INTER_RESIZE_COEF_BITS = 11) for both axes."""
import numpy as np

COEF_BITS = 11
COEF_SCALE = 1 << COEF_BITS
PAD_UINT8 = 0            # pad the uint8 image with 0: pad pixels become -mean/std after normalisation (sliding branch, :256-257)
PAD_NORMALISED = 1       # pad with 0 after normalisation (process_image(img, crop_size), :331-332)


def cv_round(v):
    """cvRound: round half to even (saturate_cast<int> of a double)."""
    return int(np.rint(v))


def resized_size(H, W, s):
    """(rows, cols) of cv2.resize(img, None, fx=s, fy=s): dsize = (cvRound(W * s), cvRound(H * s))."""
    return cv_round(H * s), cv_round(W * s)


def pad_margins(rows, cols, crop_h, crop_w):
    """pad_image_to_shape (img_utils.py:60-74): (top, bottom, left, right), the odd pixel at the bottom / right."""
    ph, pw = max(crop_h - rows, 0), max(crop_w - cols, 0)
    return ph // 2, ph // 2 + ph % 2, pw // 2, pw // 2 + pw % 2


def linear_taps(src_size, dst_size, inv_scale):
    """cv2 INTER_LINEAR taps of one axis for uint8 data: (index (dst,) int32, coefficients (dst, 2) int16).

    fx = (float)((dx + 0.5) * (1 / inv_scale) - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> (0, fx = 0); sx >= src - 1 -> (src - 1, fx = 0);
    coefficients cvRound((1 - fx) * 2048), cvRound(fx * 2048) in float.  The second tap reads index + 1 (clamped to the last pixel,
    where its coefficient is 0)."""
    scale = 1.0 / inv_scale
    d = np.arange(dst_size, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(f).astype(np.int64)
    f = (f - sx.astype(np.float32)).astype(np.float32)
    low = sx < 0
    sx[low], f[low] = 0, 0
    high = sx >= src_size - 1
    sx[high], f[high] = src_size - 1, 0
    c0 = np.rint((np.float32(1) - f) * np.float32(COEF_SCALE)).astype(np.int16)
    c1 = np.rint(f * np.float32(COEF_SCALE)).astype(np.int16)
    return sx.astype(np.int32), np.stack([c0, c1], axis=1)


def pack_taps(index, coef):
    """Device tap table: int32 (n, 2) rows [index, c0 | c1 << 16] (both coefficients are in 0..2048)."""
    packed = coef[:, 0].astype(np.int32) | (coef[:, 1].astype(np.int32) << 16)
    return np.ascontiguousarray(np.stack([index.astype(np.int32), packed], axis=1))


class ScalePlan:
    """One scale of scale_process.  The resized image sits at (top, left) of a canvas_h x canvas_w canvas; every window is
    crop x crop with its origin at one of `windows` (row, col) in canvas coordinates; the score is the canvas rectangle
    [top, top + rows) x [left, left + cols).  sliding: the windows' exp-scores are summed on the canvas (evaluator.py:260-292);
    otherwise the single window is the whole padded canvas (:247-252)."""

    def __init__(self, s, H, W, crop, stride_rate):
        self.scale = s
        self.crop = crop
        self.rows, self.cols = resized_size(H, W, s)
        self.sliding = max(self.rows, self.cols) > crop
        top, bottom, left, right = pad_margins(self.rows, self.cols, crop, crop)
        self.margins = (top, bottom, left, right)
        self.top, self.left = top, left
        self.canvas_h, self.canvas_w = self.rows + top + bottom, self.cols + left + right
        if self.sliding:
            self.pad_mode = PAD_UINT8
            self.stride = int(np.ceil(crop * stride_rate))
            r_grid = int(np.ceil((self.canvas_h - crop) / self.stride)) + 1
            c_grid = int(np.ceil((self.canvas_w - crop) / self.stride)) + 1
            self.windows = []
            for gy in range(r_grid):
                for gx in range(c_grid):
                    e_x = min(gx * self.stride + crop, self.canvas_w)
                    e_y = min(gy * self.stride + crop, self.canvas_h)
                    self.windows.append((e_y - crop, e_x - crop))
        else:
            self.pad_mode = PAD_NORMALISED
            self.stride = None
            self.windows = [(0, 0)]
        self.y_index, self.y_coef = linear_taps(H, self.rows, s)
        self.x_index, self.x_coef = linear_taps(W, self.cols, s)

    def __repr__(self):
        return "ScalePlan(s=%g, resized=%dx%d, canvas=%dx%d, margins=%s, %s, %d windows)" % (
            self.scale, self.rows, self.cols, self.canvas_h, self.canvas_w, self.margins,
            "sliding" if self.sliding else "padded", len(self.windows))


def scale_plan(H, W, scales, crop, stride_rate):
    """[ScalePlan] of sliding_eval over `scales` for an (H, W) image."""
    crop = int(crop)
    assert crop > 0 and stride_rate > 0 and all(s > 0 for s in scales)
    plans = [ScalePlan(float(s), H, W, crop, stride_rate) for s in scales]
    for p in plans:
        assert p.rows > 0 and p.cols > 0, "scale %g resizes a %dx%d image to nothing" % (p.scale, H, W)
    return plans


def two_d(size):
    """get_2dshape: an int n -> (n, n)."""
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    h, w = size
    return int(h), int(w)


def n_passes(plans, is_flip):
    """Network passes of sliding_eval (the mirrored pass of each window counts)."""
    return sum(len(p.windows) for p in plans) * (2 if is_flip else 1)

