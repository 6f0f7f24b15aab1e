"""fp64 reference, per-element bound and parameter zoo for the multi-tensor SGD kernel (csrc/optim.hip sgd_multi_kernel, driven by
optim.FlatSGD).  Plain numpy: nothing here calls the library or a torch kernel (rne16 of tests/_bounds.py, one CPU conversion, is the
only torch call).  Users: tests/test_sgd_ref_selfcheck.py (CPU: honest emulations pass, mutants fail), tests/test_sgd_layout.py (CPU: the
chunk decode restated), tests/test_flat_sgd_gpu.py (the kernel itself).

The update, element-wise, on fp32 values widened to fp64 (exact) and the fp32-rounded scalars the C ABI receives:
    b = mu m + (c g + wd p),     m' = b,     p' = p - lr b.

The bound counts the fp32 operations of sgd_multi_kernel (both walks compute the same expression):
    g' = grads[e] * clip + weight_decay * p     two products and one sum (or one product and one fma)
    b  = momentum * mom[e] + g'                 one product and one sum (or one fma)
    p' = p - lr * b                             one product and one difference (or one fma)
Every operation is charged E32 = 2^-23 of the magnitude it rounds (tests/_bounds.py: twice the unit roundoff, which covers the
second-order terms and either contraction choice of the compiler).  |c g| and |wd p| are rounded by their product, the inner sum and
the outer sum: 3 each; |mu m| by its product and the outer sum: 2.  With S = |c g| + |wd p| + |mu m|:
    |m'_dev - m'_64| <= 3 E32 S + TINY
p' inherits lr times that, the product lr * b rounds lr |b| once and the difference rounds |p - lr b| <= |p| + lr |b| once:
    |p'_dev - p'_64| <= lr 3 E32 S + E32 (|p| + 2 lr |b_64|) + TINY
The issue that asked for these tests proposed 2 E32 (|p| + lr |b_64|) for the second term; the count gives |p| ONE rounding (only the
difference touches it), so the bound here is the tighter one.  `c_rel`: the caller knows c only to that relative error (step() forms
it on the device in three fp32 operations); it widens the |c g| term."""
import numpy as np
import torch

from tests._bounds import E32, TINY, rne16

SENTINEL = 7.25                      # exact in bf16 and fp32 (tests/test_bwd_bounds_gpu.py)
GUARD = 64                           # sentinel elements in front of, between and behind the parameters
SCALES = (1e-4, 1e-2, 1.0, 30.0)
CHUNK, TILE_O, TILE_POS = 4096, 16, 256                  # csrc/optim.hip SGD_CHUNK, SGD_TO, SGD_POS


def f32(x):
    """the fp32-rounded scalar the C ABI receives, widened"""
    return float(np.float32(x))


def step64(p, m, g, c, lr, mu, wd):
    """-> (m', p') in fp64.  Element-wise: gradient order against parameter order is the caller's business."""
    b = mu * m + (c * g + wd * p)
    return b, p - lr * b


def bound(p, m, g, c, lr, mu, wd, c_rel=0.0):
    """-> (bound of m', bound of p'), see the module docstring"""
    cg = np.abs(c * g)
    S = cg + np.abs(wd * p) + np.abs(mu * m)
    b64 = np.abs(mu * m + (c * g + wd * p))
    eb = 3 * E32 * S + c_rel * cg
    return eb + TINY, lr * eb + E32 * (np.abs(p) + 2 * lr * b64) + TINY


def to_grad_order(a):
    """OIHW -> the [O][R][S][I] order of a filter's gradient / momentum slice and of its forward pack; other tensors as they are"""
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)) if a.ndim == 4 else a


def to_param_order(a, shape):
    """a flat slice in gradient order -> the parameter's shape"""
    if len(shape) == 4:
        O, I, R, S = shape
        return np.ascontiguousarray(a.reshape(O, R, S, I).transpose(0, 3, 1, 2))
    return a.reshape(shape)


def pack_bits(v64, dtype):
    """the bit patterns (int32 / int16) of fp32 values stored in `dtype`: identity for fp32, round to nearest even for bf16"""
    if dtype == torch.float32:
        return np.ascontiguousarray(v64.astype(np.float32)).view(np.int32)
    return rne16(dtype, torch.from_numpy(v64.copy(order="C"))).view(torch.int16).numpy()


def packs64(p_new, dtype):
    """-> (fwd [O][R][S][I], flip [I][R][S][O]) bit patterns: fwd[o,r,s,i] = round(p[o,i,r,s]), flip[i,r,s,o] = round(p[o,i,R-1-r,S-1-s])"""
    fwd = p_new.transpose(0, 2, 3, 1)
    flip = p_new[:, :, ::-1, ::-1].transpose(1, 2, 3, 0)
    return pack_bits(fwd, dtype), pack_bits(flip, dtype)


def packable(shape):
    """optim.FlatSGD's rule for a resident pack (given a pack dtype)"""
    return len(shape) == 4 and shape[0] % 8 == 0 and shape[1] % 8 == 0 and shape[2] == shape[3] and shape[2] in (1, 3)


# ---- the kernel's chunk decode, restated --------------------------------------------------------------------------------------------------
def tile_i(taps):
    return 1 if taps >= TILE_POS else TILE_POS // taps


def chunk_model(numel, I, taps, has_packs):
    """-> ("linear", [(begin, end)]) or ("tiled", [(o0, rows, i0, ni)]), one entry per block in chunk-index order; None for a filter the
    kernel cannot hold (taps > 256)"""
    if taps > TILE_POS:
        return None
    if taps == 1 and not has_packs:
        return "linear", [(b, min(b + CHUNK, numel)) for b in range(0, numel, CHUNK)]
    O, IT = numel // (taps * I), tile_i(taps)
    npt = -(-I // IT)
    out = []
    for c in range(-(-O // TILE_O) * npt):
        o0, i0 = (c // npt) * TILE_O, (c % npt) * IT
        out.append((o0, min(TILE_O, O - o0), i0, min(IT, I - i0)))
    return "tiled", out


def geometry(shape):
    """(numel, I, taps) as optim.FlatSGD describes a parameter"""
    n = int(np.prod(shape))
    return (n, shape[1], shape[2] * shape[3]) if len(shape) == 4 else (n, 1, 1)


# ---- the parameter zoo --------------------------------------------------------------------------------------------------------------------
# (shape, scale index of p, m, g, walk without packs, walk with a pack dtype, (o tiles, i tiles, rows of the last o tile, input channels
# of the last i tile) or the number of linear chunks, what the shape is there for).  The scales come from SCALES per tensor and per
# operand; the table is written out, not drawn, so that tensors of a few elements keep operands every mutant of the self-check shows on
# (a parameter of 1e-4 under a momentum of 30 hides its weight decay below the bound at every element), while the large tensors take the
# harsh combinations.  p = 30 with g = 1e-4 (three tensors): |wd p| >> |c g|, the decay term carries the update.
ZOO = [
    ((1,),              2, 2, 1, "linear", "linear", 1,              "one element"),
    ((8, 8, 1, 1),      2, 1, 2, "linear", "tiled",  (1, 1, 8, 8),   "packed 1x1: O < 16, I < IT = 256; linear without packs"),
    ((255,),            1, 0, 1, "linear", "linear", 1,              "less than one block of threads"),
    ((16, 3, 3, 3),     2, 3, 2, "tiled",  "tiled",  (1, 1, 16, 3),  "O == 16, I < IT = 28"),
    ((16, 256, 1, 1),   3, 2, 0, "linear", "tiled",  (1, 1, 16, 256), "packed 1x1: I == IT = 256, one full tile; decay carries it"),
    ((4096,),           0, 1, 0, "linear", "linear", 1,              "exactly one chunk"),
    ((17, 28, 3, 3),    1, 2, 3, "tiled",  "tiled",  (2, 1, 1, 28),  "O % 16 == 1, I == IT"),
    ((24, 264, 1, 1),   2, 0, 1, "linear", "tiled",  (2, 2, 8, 8),   "packed 1x1: I == IT + 8, O % 16 == 8"),
    ((4097,),           2, 3, 3, "linear", "linear", 2,              "one chunk and one element"),
    ((5, 29, 3, 3),     3, 1, 0, "tiled",  "tiled",  (1, 2, 5, 1),   "O < 16, I == IT + 1; decay carries it"),
    ((40, 32, 3, 3),    1, 1, 2, "tiled",  "tiled",  (3, 2, 8, 4),   "packed 3x3: three o tiles, I == IT + 4"),
    ((19, 7),           3, 0, 0, "linear", "linear", 1,              "2-D weight; decay carries it"),
    ((33, 57, 3, 3),    0, 1, 1, "tiled",  "tiled",  (3, 3, 1, 1),   "O == 2 * 16 + 1, I == 2 * IT + 1"),
    ((8, 56, 3, 3),     2, 2, 3, "tiled",  "tiled",  (1, 2, 8, 28),  "packed 3x3: I == 2 * IT"),
    ((10, 12, 1, 1),    1, 3, 2, "linear", "linear", 1,              "1x1 filter that is not packable: linear even with a pack dtype"),
    ((8, 10, 1, 3),     2, 0, 3, "tiled",  "tiled",  (1, 1, 8, 10),  "taps == 3 (R != S), IT = 85"),
    ((4, 6, 5, 5),      3, 3, 1, "tiled",  "tiled",  (1, 1, 4, 6),   "taps == 25, I < IT = 10"),
    ((8, 5, 7, 7),      1, 1, 1, "tiled",  "tiled",  (1, 1, 8, 5),   "taps == 49, I == IT = 5"),
    ((3, 2, 16, 16),    2, 2, 2, "tiled",  "tiled",  (1, 2, 3, 1),   "taps == 256, IT = 1: the largest filter the LDS tile holds"),
]
SHAPES = [z[0] for z in ZOO]


class Values:
    """the zoo's operands: per tensor p, m, g (float32, parameter shape; m and g are ALSO held in the parameter's shape - use
    to_grad_order for the flat buffers).  A quarter of the gradient elements and an eighth of the momentum elements are exactly zero
    (tensors of fewer than 8 elements keep all of theirs)."""

    def __init__(self, seed=20):
        self.p, self.m, self.g = [], [], []
        for k, (shape, sp, sm, sg) in enumerate(z[:4] for z in ZOO):
            rng = np.random.default_rng(seed * 1000 + k)
            p, m, g = (np.float32(SCALES[s]) * rng.standard_normal(shape).astype(np.float32) for s in (sp, sm, sg))
            if p.size >= 8:
                g[rng.random(shape) < 0.25] = 0.0
                m[rng.random(shape) < 0.125] = 0.0
            self.p.append(p), self.m.append(m), self.g.append(g)


def param_layout():
    """offsets (elements) of the zoo's parameters in ONE buffer with GUARD sentinel elements around each -> (offsets, total)"""
    offs, off = [], GUARD
    for shape in SHAPES:
        offs.append(off)
        off += int(np.prod(shape)) + GUARD
    return offs, off
