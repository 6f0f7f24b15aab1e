"""Host reference of the per-pixel confidence byte (fs_bilinear_argmax_conf, fs_score_confidence) and the cases the tests share.

Reference, per output pixel: the align_corners=True up-sample of tests/_resize_ref.upsample (fp32 taps, fp64 blend of the stored values),
a_c = v_c - max_c v_c, p = 1 / sum_{c<C} exp(a_c) in fp64, t = 255 p.  A byte q passes iff |q - t| <= 0.5 + 255 eps with

    eps = (12 M + 3 A + 8 + C) * 2^-24,      M = max |x| over the C real channels of the case, A = max |a_c| of the case.

Derivation against the kernel's operation order (csrc/confidence.hip), u = 2^-24 (half an fp32 ulp, relative):
  * v_c: bilerp's two products and a sum per line and once more for the rows, of values bounded by M with weights in [0, 1]: at most
    6 u M absolute per blended value (the bound tests/test_logits_upsample_tiled_gpu.py derives; the 16-bit storage types are exact in
    fp32, the taps are the reference's own fp32 taps).  a_c = v_c - v_max carries it twice: 12 u M.  The kernel's v_max is the fp32
    maximum; where the fp64 maximum is another class the two values are within those 12 u M of each other, so the same term covers it.
  * the subtraction rounds once (u |a|), the product with log2 e rounds once (u |a|) and log2 e itself is an fp32 constant (u |a|): an
    absolute error of 3 u A in the exponent of e_c, i.e. a relative error of 12 u M + 3 u A in e_c (first order; the exponent errors are
    below 1e-4 in every case here).  The winner's own term is exact: a = 0, exp2(0) = 1.
  * v_exp_f32 is good to 1 ulp = 2 u, v_rcp_f32 to 1 ulp = 2 u, the fma 255 p + 0.5 rounds once (u of a value <= 255.5, i.e. about u in
    units of p), the conversion to int truncates the exact floor: 5 u, taken as the constant 8 u.
  * the sum of C non-negative terms in index order rounds C - 1 times, each by at most u of the partial sum <= the total: C u.
p = 1 / sum is at most 1 and its relative error is at most the largest relative error of a term plus the sum's and the reciprocal's, so
eps bounds |p_kernel - p| absolutely.  255 eps is 0.001 - 0.03 in the cases below: the bound decides the byte everywhere except within
that distance of a half-integer t, where either neighbour passes.  No pixel is exempt.

fs_score_confidence: conf = max / sum on an fp32 buffer whose values are exact inputs: C - 1 roundings of the sum, one of the division,
one of the fma: relative (C + 4) u is the bar the issue sets, plus the half byte; a zero or non-finite sum gives exactly 0."""
import numpy as np
import torch

from tests import _resize_ref as R

U = 2.0 ** -24
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# (N, C, x_cs, (Hi, Wi), (Ho, Wo))
CASES = {
    "x8-two-images": (2, 19, 32, (8, 12), (64, 96)),
    "x8-tight-stride": (1, 19, 20, (8, 12), (64, 96)),
    "x8-several-blocks": (1, 19, 32, (12, 40), (96, 320)),
    "generic-ratio": (1, 19, 20, (9, 13), (72, 100)),
    "c21-odd-rows": (1, 21, 24, (5, 7), (33, 52)),
    "down-sample": (1, 19, 32, (16, 24), (8, 12)),
    "one-class": (1, 1, 4, (3, 3), (24, 24)),
    "two-classes": (1, 2, 4, (3, 3), (24, 24)),
}
_cache = {}


def store(a, dtype):
    """fp32 array rounded to the storage type, as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH[dtype]).float().numpy()


def logits(case, dtype, scale=2.0, seed=7):
    """(buffer (N, Hi, Wi, x_cs) fp32 holding values exact in `dtype`, C): scale * randn logits in the first C lanes, the pad lanes hold
    finite junk larger than any logit (1e4; 6e4 for fp16)."""
    key = (case, dtype, scale, seed)
    if key not in _cache:
        N, C, cs, (Hi, Wi), _ = CASES[case]
        rng = np.random.default_rng(seed)
        buf = np.full((N, Hi, Wi, cs), 6e4 if dtype == "fp16" else 1e4, dtype=np.float32)
        buf[..., :C] = scale * rng.standard_normal((N, Hi, Wi, C)).astype(np.float32)
        _cache[key] = (store(buf, dtype), C)
    return _cache[key]


def epsilon(M, A, C):
    return (12.0 * M + 3.0 * A + 8.0 + C) * U


def reference(buf, C, size):
    """dict(t = 255 p fp64 (N, Ho, Wo), cls = fp64 arg-max, vmax = the winner's value, tol = 0.5 + 255 eps, eps, M, A) of the first C
    lanes of an NHWC buffer"""
    x = np.asarray(buf[..., :C], dtype=np.float64).transpose(0, 3, 1, 2)
    v = R.upsample(x, size)
    a = v - v.max(axis=1, keepdims=True)
    p = 1.0 / np.exp(a).sum(axis=1)
    M, A = float(np.abs(x).max()), float(np.abs(a).max())
    eps = epsilon(M, A, C)
    return dict(t=255.0 * p, cls=v.argmax(axis=1), vmax=v.max(axis=1), tol=0.5 + 255.0 * eps, eps=eps, M=M, A=A)


def failures(q, ref):
    """boolean map of the bytes outside the bound"""
    return np.abs(np.asarray(q, dtype=np.float64) - ref["t"]) > ref["tol"]


def score_reference(score, C):
    """(t = 255 * fp64 share of the maximum over the first C lanes, 0 where the sum is zero or not finite; tol per pixel; first arg-max)"""
    s = np.asarray(score[..., :C], dtype=np.float64)
    with np.errstate(all="ignore"):
        total = s.sum(axis=-1)
        ok = np.isfinite(total) & (total > 0)
        share = np.where(ok, s.max(axis=-1) / np.where(ok, total, 1.0), 0.0)
    return 255.0 * share, 0.5 + 255.0 * share * (C + 4) * U, s.argmax(axis=-1)


# ---- the contract evaluated in numpy float32, and the mistakes the bound must catch ------------------------------------------------
def fp32_bytes(buf, C, size, truncate=False, scale=255.0, soft_dtype=None, with_pads=False, subtract_max=True):
    """q of the contract in fp32 (bilerp's operation order without the fused multiply-adds).  truncate: floor(255 p) instead of rounding;
    scale: 256 instead of 255; soft_dtype: the up-sampled values rounded to that storage type before the softmax; with_pads: the pad lanes
    enter the sum; subtract_max=False: exp of the raw values."""
    f = np.float32
    x = np.asarray(buf, dtype=f).transpose(0, 3, 1, 2)
    h0, h1, a0, a1 = R.taps(x.shape[2], size[0])
    w0, w1, b0, b1 = R.taps(x.shape[3], size[1])
    a0, a1, b0, b1 = (np.asarray(w, dtype=f) for w in (a0, a1, b0, b1))
    top = (b1 * x[:, :, h0][:, :, :, w1] + b0 * x[:, :, h0][:, :, :, w0]).astype(f)
    bot = (b1 * x[:, :, h1][:, :, :, w1] + b0 * x[:, :, h1][:, :, :, w0]).astype(f)
    v = (a1[:, None] * bot + a0[:, None] * top).astype(f)
    if soft_dtype is not None:
        v = store(v, soft_dtype)
    best = v[:, :C].max(axis=1, keepdims=True)
    terms = v if with_pads else v[:, :C]
    with np.errstate(all="ignore"):
        a = (terms - best).astype(f) if subtract_max else terms
        e = np.exp2((a * f(1.4426950408889634)).astype(f)).astype(f)
        s = np.zeros_like(e[:, 0])
        for c in range(e.shape[1]):
            s = (s + e[:, c]).astype(f)
        p = (np.exp2((best[:, 0] * f(1.4426950408889634)).astype(f)).astype(f) / s if not subtract_max else f(1) / s).astype(f)
        t = (f(scale) * p + f(0.0 if truncate else 0.5)).astype(f)
        t = np.where(np.isnan(t), f(0), t)
    return np.clip(np.floor(t), 0, 255).astype(np.uint8)
