"""Host-side plan of the reference's training augmentation (search|train/dataloader.py TrainPre, tools/utils/img_utils.py,
tools/datasets/BaseDataset.py), pure Python + numpy so it can be checked without a GPU.

Per sample, `draw_sample` makes the reference's random draws in its order - random() for the mirror, choice() of the scale,
randint() of the crop row, randint() of the crop column, each only when its condition holds - and derives the scaled size, the crop
origin, the pad margins and the valid rows / columns of the crop.  `TableStore` holds every float-derived index the device needs
(cv2's 8-bit INTER_LINEAR taps and INTER_NEAREST indices) once per (source size, scaled size) and per (crop, g); `norm_table` is
the normalisation as a 3 x 256 fp32 lookup table.  fs_train_batch (csrc/train_input.hip) then only does integer arithmetic."""
import numpy as np

from .eval_plan import linear_taps, pack_taps, pad_margins

SAMPLE_INTS = 16            # int32 fields of fs_train_sample


def nearest_index(src_size, dst_size, inv_scale):
    """cv2 INTER_NEAREST source indices of one axis (OpenCV 4 resizeNN): min(cvFloor(d * (1 / inv_scale)), src - 1) in double,
    inv_scale = dsize / ssize as cv2.resize derives it."""
    ifx = 1.0 / inv_scale
    return np.minimum(np.floor(np.arange(dst_size, dtype=np.float64) * ifx).astype(np.int64), src_size - 1).astype(np.int32)


def norm_table(mean, std):
    """(3, 256) fp32: img_utils.normalize of every uint8 value, (u.astype(float32) / 255.0 - mean) / std with the caller's mean /
    std objects (float64 arrays in the configs), rounded to fp32 as torch.from_numpy(...).float() does."""
    img = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)[None]           # (1, 256, 3) uint8 "image"
    x = img.astype(np.float32) / 255.0
    x = x - mean
    x = x / std
    return np.ascontiguousarray(np.asarray(x)[0].astype(np.float32).T)


def load_size(H, W, down_sampling):
    """Size after BaseDataset._open_image: an int d -> (H // d, W // d); an (h, w) pair -> (h, w)."""
    if isinstance(down_sampling, (int, np.integer)):
        d = int(down_sampling)
        assert d >= 1, "down_sampling must be >= 1"
        return H // d, W // d
    h, w = down_sampling
    return int(h), int(w)


class SampleDraw:
    """One sample of TrainPre: mirror, scale, scaled size (sh, sw), crop origin (pos_h, pos_w) in the scaled image, pad margins
    (top, bottom, left, right) and the valid rows / cols of the crop."""
    __slots__ = ("H", "W", "mirror", "scale", "sh", "sw", "pos_h", "pos_w", "rows", "cols", "top", "bottom", "left", "right")

    def __repr__(self):
        return "SampleDraw(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def draw_sample(rng, H, W, crop_h, crop_w, scales):
    """The draws of TrainPre.__call__ for an (H, W) source from `rng` (anything with random / choice / randint: the `random` module,
    random.Random): random_mirror, random_scale (if scales is not None), generate_random_crop_pos, random_crop_pad_to_shape."""
    d = SampleDraw()
    d.H, d.W = int(H), int(W)
    d.mirror = rng.random() >= 0.5
    if scales is not None:
        d.scale = rng.choice(scales)
        d.sh, d.sw = int(H * d.scale), int(W * d.scale)          # truncation, not cvRound
    else:
        d.scale = None
        d.sh, d.sw = d.H, d.W
    assert d.sh > 0 and d.sw > 0, "scale %r resizes a %dx%d source to nothing" % (d.scale, H, W)
    # randint's bounds are inclusive: pos = h - crop + 1 leaves the crop one row / column short, padded at the bottom / right
    d.pos_h = rng.randint(0, d.sh - crop_h + 1) if d.sh > crop_h else 0
    d.pos_w = rng.randint(0, d.sw - crop_w + 1) if d.sw > crop_w else 0
    d.rows, d.cols = min(crop_h, d.sh - d.pos_h), min(crop_w, d.sw - d.pos_w)
    d.top, d.bottom, d.left, d.right = pad_margins(d.rows, d.cols, crop_h, crop_w)
    return d


class TableStore:
    """The int32 tables fs_train_batch reads, appended once per key into one array; offsets count int32 entries, the pair tables
    start at even offsets.  `n` grows monotonically: a device copy of array()[:n] stays valid for every offset handed out."""

    def __init__(self):
        self._chunks = []
        self.n = 0
        self._index = {}

    def _add(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
        if self.n % 2:
            self._chunks.append(np.zeros(1, np.int32))
            self.n += 1
        off = self.n
        self._chunks.append(a)
        self.n += a.size
        return off

    def scale_tables(self, H, W, sh, sw):
        """(ylin, xlin, ynn, xnn): cv2.resize(., (sw, sh)) of an (H, W) source - INTER_LINEAR taps and INTER_NEAREST indices, the
        scale per axis from dsize (inv_scale_x = sw / W, inv_scale_y = sh / H)."""
        key = ("scale", H, W, sh, sw)
        if key not in self._index:
            ylin = self._add(pack_taps(*linear_taps(H, sh, sh / H)))
            xlin = self._add(pack_taps(*linear_taps(W, sw, sw / W)))
            ynn = self._add(nearest_index(H, sh, sh / H))
            xnn = self._add(nearest_index(W, sw, sw / W))
            self._index[key] = (ylin, xlin, ynn, xnn)
        return self._index[key]

    def label_tables(self, crop_h, crop_w, g):
        """(gy, gx): cv2.resize(p_gt, (crop_w // g, crop_h // g), INTER_NEAREST) of the padded crop."""
        key = ("label", crop_h, crop_w, g)
        if key not in self._index:
            lh, lw = crop_h // g, crop_w // g
            self._index[key] = (self._add(nearest_index(crop_h, lh, lh / crop_h)), self._add(nearest_index(crop_w, lw, lw / crop_w)))
        return self._index[key]

    def array(self):
        if len(self._chunks) > 1:
            self._chunks = [np.concatenate(self._chunks)]
        return self._chunks[0] if self._chunks else np.zeros(0, np.int32)


def sample_row(d, tables):
    """The fs_train_sample fields of a draw (int32 (16,)); tables = TableStore.scale_tables of its sizes."""
    ylin, xlin, ynn, xnn = tables
    return np.array([d.H, d.W, int(d.mirror), d.sh, d.sw, d.pos_h, d.pos_w, d.top, d.left, d.rows, d.cols, ylin, xlin, ynn, xnn, 0],
                    dtype=np.int32)


def load_tables(H, W, down_sampling):
    """Tables of the down-sampling at load (fs_resize_u8): ((h, w), image (ytab, xtab) linear pairs, label (ytab, xtab) nearest),
    or None when the size does not change (cv2.resize copies)."""
    h, w = load_size(H, W, down_sampling)
    assert h > 0 and w > 0, "down_sampling %r leaves nothing of a %dx%d image" % (down_sampling, H, W)
    if (h, w) == (H, W):
        return None
    lin = (pack_taps(*linear_taps(H, h, h / H)), pack_taps(*linear_taps(W, w, w / W)))
    nn = (nearest_index(H, h, h / H), nearest_index(W, w, w / W))
    return (h, w), lin, nn


def read_file_list(source, portion=None):
    """[(img_name, gt_name)] of a reference file list (one "img gt" pair per line, split on one space), cut by `portion` as
    BaseDataset._get_file_names does: > 0 the first floor(portion * n) lines, < 0 the lines from floor((1 + portion) * n) on.
    (The reference then shuffles the list with the global `random`; the loader draws its own order.)"""
    with open(source) as f:
        files = f.readlines()
    if portion is not None:
        n = len(files)
        if portion > 0:
            files = files[:int(np.floor(portion * n))]
        elif portion < 0:
            files = files[int(np.floor((1 + portion) * n)):]
    out = []
    for item in files:
        item = item.strip().split(" ")
        out.append((item[0], item[1]))
    return out


def epoch_indices(n_samples, length, seed, epoch):
    """The sample indices of one epoch of `length` draws: every sample length // n times plus a random length % n of them
    (BaseDataset._construct_new_file_names), shuffled; from np.random.default_rng((seed, epoch))."""
    assert n_samples > 0 and length >= 0
    g = np.random.default_rng((int(seed), int(epoch)))
    idx = np.concatenate([np.tile(np.arange(n_samples), length // n_samples), g.permutation(n_samples)[:length % n_samples]])
    return g.permutation(idx)


def rank_share(indices, rank, world):
    """Rank `rank`'s share of an epoch: every world-th index from `rank` on (disjoint, together the whole epoch)."""
    assert 0 <= rank < world
    return indices[rank::world]
