"""Per-element error bounds of the kernels against fp64 references: the 16-bit inference kernels (tests/test_f16_kernels_gpu.py,
tests/test_bf16_kernels_gpu.py, tests/test_bounds_selfcheck.py) and, in the second half of the module, the training backward kernels
(tests/test_bwd_bounds_gpu.py, tests/test_bwd_bounds_selfcheck.py, the weight gradients of tests/_grouped_cases.py), and in the third
section the train-mode BatchNorm forward (tests/test_bn_fwd_bounds_gpu.py, tests/test_bn_fwd_bounds_selfcheck.py, the BatchNorm units of
tests/_grouped_cases.py).  Every helper takes the storage dtype; `For(dtype)` binds it, so a test module names its type once.

UNIT[dtype] is the unit roundoff of one round-to-nearest store: half an ulp relative to the value, 2^-p for a p-bit significand (hidden
bit included).  fp16 has 11 bits, bf16 has 8: 2^-8, not 2^-9 - a correctly rounded bf16 value just above a power of two is off by up to
2^-8 of itself.  Single-stage kernels, per element:
    |got - ref| <= UNIT |ref| + K 2^-23 sum|x w| + 2^-24
(one output rounding + the fp32 accumulation bound; K = taps x channels, 4 for a resample).  Kernels that round an intermediate map to
the storage type get the same bound PROPAGATED stage by stage (`stage`, `resample`): an input known to e gives the contraction
sum|w| e more, scale / shift add two fp32 roundings, and each stored stage adds UNIT (|value| + its error) + 2^-24.

fp32 storage has UNIT = 2^-24.  Throughout, ONE fp32 rounding is charged E32 = 2^-23 of the magnitude it rounds - twice the unit
roundoff: it covers a matrix core that truncates where the vector ALU rounds to nearest, and the second-order terms of the products of
(1 + delta) factors, so the counts below are plain counts of operations."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import _resize_ref as R

UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
E32, TINY = 2.0 ** -23, 2.0 ** -24


def rnd16(dtype, *shape, seed, scale=1.0):
    """seeded normal values already rounded to `dtype`, as float64"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).double()


def grid(*shape, seed, den, lim, density=1.0):
    """j / den with |j| <= lim (float64), a fraction `density` of them non-zero"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-lim, lim + 1, shape, generator=g).double() / den
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density).double()
    return v


def bits(t):
    """16-bit NHWC view / tensor -> int16 bit patterns in logical (N, C, H, W) order, on the CPU"""
    return t.contiguous().view(torch.int16).cpu()


def rne16(dtype, v64):
    """round-to-nearest-even of exact float64 values to `dtype`.  fp16: numpy converts float64 -> float16 in one correctly rounded step.
    bf16: torch goes through fp32, so the value must be an fp32 number already (asserted) - the conversion is then a single rounding."""
    if dtype == torch.float16:
        return torch.from_numpy(v64.numpy().astype(np.float16))
    assert dtype == torch.bfloat16, dtype
    assert bool((v64.float().double() == v64).all()), "not exactly representable in fp32: float64 -> bf16 would round twice"
    return v64.float().to(torch.bfloat16)


def dev16(dtype, x64):
    from fasterseg_amd import kernels
    return kernels.to_nhwc(x64.float().cuda(), dtype)


def conv64(x, w, stride, pad):
    if pad < 0:
        return F.conv2d(x[:, :, -pad:, -pad:], w, None, stride, 0)
    return F.conv2d(x, w, None, stride, pad)


def assert_within(got, ref, bound, what):
    err = (got.detach().double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print("%s: max |err| %.3e, worst err / bound %.3f" % (what, float(err.max()), worst))
    assert bool((err <= bound).all()), "%s: %d of %d above the bound, worst err / bound %.3f" % (what, int((err > bound).sum()), err.numel(), worst)


def single_bound(dtype, ref, mag, k):
    return UNIT[dtype] * ref.abs() + k * E32 * mag + TINY


def _stage(dtype, v, e, w, s, b, relu, stride=1, pad=1, store=True):
    """One conv stage of a chain: v fp64 values the device holds to within e (per element).  Returns (values, bound) of the stage's output:
    contraction (K fp32 roundings on sum|x w|, the input error through sum|w|), scale / shift (two more), ReLU (1-Lipschitz), and, when
    the stage is stored in `dtype`, one rounding of the erroneous value."""
    k = w.shape[1] * w.shape[2] * w.shape[3]
    sv = s.view(1, -1, 1, 1) if s is not None else 1.0
    bv = b.view(1, -1, 1, 1) if b is not None else 0.0
    o = conv64(v, w, stride, pad) * sv + bv
    prop = conv64(e, w.abs(), stride, pad) * (sv.abs() if s is not None else 1.0) if e is not None else 0.0
    mag = conv64(v.abs(), w.abs(), stride, pad) * (sv.abs() if s is not None else 1.0) + (bv.abs() if b is not None else 0.0)
    err = prop + (k + 2) * E32 * (mag + prop)
    if relu:
        o = F.relu(o)
    if store:
        err = err + UNIT[dtype] * (o.abs() + err) + TINY
    return o, err


def _resample(dtype, v, e, size, relu=False, store=True, exact_taps=False):
    """bilinear (align_corners=True, fp32 taps as the kernels compute them) of values held to within e: 4 taps.  The NCHW logits writers
    compute the tap weights exactly as the reference does (make_tap_rn, exact_taps=True).  The other kernels use make_tap, where the
    compiler may contract scale * dst - i0 into one fma: a weight is then off by up to half an ulp of src, 2^-24 * in_size at most, per
    axis (csrc/resize.hip says so above make_tap_rn) - an uncertainty of the REFERENCE's weights, which moves the blend by at most that
    times the four neighbours' magnitudes."""
    o = torch.from_numpy(R.upsample(v.numpy(), size))
    mag = torch.from_numpy(R.upsample(v.abs().numpy(), size))
    err = 4 * E32 * mag + (torch.from_numpy(R.upsample(e.numpy(), size)) if e is not None else 0.0)
    if not exact_taps:
        h0, h1, _, _ = R.taps(v.shape[2], size[0])
        w0, w1, _, _ = R.taps(v.shape[3], size[1])
        a = v.abs()
        nb = a[:, :, h0][:, :, :, w0] + a[:, :, h0][:, :, :, w1] + a[:, :, h1][:, :, :, w0] + a[:, :, h1][:, :, :, w1]
        err = err + TINY * (v.shape[2] + v.shape[3]) * nb
    if relu:
        o = F.relu(o)
    if store:
        err = err + UNIT[dtype] * (o.abs() + err) + TINY
    return o, err


def _second_stage_exact(t, w2, pad):
    """every sum of |terms| of the second contraction is a multiple of 2^-12 below 2^12: 24 bits, exact in fp32 in any order"""
    terms = conv64(t.abs(), w2.abs(), 1, pad)
    assert bool(((t * 4096).round() == t * 4096).all()) and bool(((w2 * 4096).round() == w2 * 4096).all())
    assert float(terms.max()) < 2.0 ** 12, float(terms.max())


def _argmax_inputs(dtype, case, seed):
    n, c, cs, (hi, wi), size = case
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, c, hi, wi, generator=g) * 4.0).to(dtype)
    x[:, 1] = x[:, 0]                                                          # classes 0 and 1 tie exactly everywhere: the lower index wins
    buf = torch.randn(n, hi, wi, cs, generator=g).to(dtype)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    up, err = _resample(dtype, x.double(), None, size, store=False)
    top = up.topk(2, dim=1)
    decided = (top.values[:, 0] - top.values[:, 1]) > 2 * err.max(1).values
    tie01 = (top.indices[:, 0] <= 1) & (top.indices[:, 1] <= 1)               # the planted tie: margin 0, the answer must be class 0
    third = up.topk(3, dim=1).values
    tie_ok = tie01 & ((third[:, 1] - third[:, 2]) > 2 * err.max(1).values)
    want = torch.where(tie_ok, torch.zeros_like(top.indices[:, 0]), top.indices[:, 0])
    return buf, want, decided | tie_ok, tie_ok


class For:
    """the helpers above with the storage dtype bound"""

    def __init__(self, dtype):
        self.dtype, self.E = dtype, UNIT[dtype]

    def rnd16(self, *shape, seed, scale=1.0):
        return rnd16(self.dtype, *shape, seed=seed, scale=scale)

    def rne16(self, v64):
        return rne16(self.dtype, v64)

    def dev16(self, x64):
        return dev16(self.dtype, x64)

    def single_bound(self, ref, mag, k):
        return single_bound(self.dtype, ref, mag, k)

    def _stage(self, v, e, w, s, b, relu, stride=1, pad=1, store=True):
        return _stage(self.dtype, v, e, w, s, b, relu, stride=stride, pad=pad, store=store)

    def _resample(self, v, e, size, relu=False, store=True, exact_taps=False):
        return _resample(self.dtype, v, e, size, relu=relu, store=store, exact_taps=exact_taps)

    def _argmax_inputs(self, case, seed):
        return _argmax_inputs(self.dtype, case, seed)


# =========================================================================================================================================
# The training backward kernels.  References are fp64 on the CPU on operands already rounded to the storage type; every bound counts the
# roundings the kernel performs (E32 each, see the header) on the magnitudes they round.
# =========================================================================================================================================
WGRAD_P_MAX = 2048                      # P^2 2^-23 << 1: one lost pixel of a P-pixel contraction stands out of a bound of P roundings
WGRAD_SLAB_MIN_PIXELS, WGRAD_BCH = 256, 64                 # csrc/wgrad.hip: SLAB_MIN_PIXELS, BCH
WGRAD_KC = {torch.float32: 64, torch.bfloat16: 128}        # csrc/wgrad.hip: Chunk<T>::KC, pixels staged per iteration
WGRAD_TARGET_BLOCKS = 1024                                 # wgrad_prepare's target_blocks of a single launch
WORKSPACE_BYTES, WS_COUNTER_BYTES = 16 << 20, 65536        # kernels.WORKSPACE_BYTES, kernels.WS_COUNTER_BYTES


def conv_out_hw(H, W, k, stride, pad):
    if pad < 0:                                                                # FactorizedReduce's second branch convolves x[:, :, 1:, 1:]
        return (H + pad - k) // stride + 1, (W + pad - k) // stride + 1
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def wgrad_slabs(M, cout, cin, taps, dtype, blocks_wanted=WGRAD_TARGET_BLOCKS, ws_bytes=0):
    """wgrad_prepare's slab rule (csrc/wgrad.hip) restated: (number of pixel slabs = gridDim.x, pixels per slab).  ws_bytes > 0: the
    bit-reproducible mode, where the partial tiles must fit the workspace in front of its arrival counters."""
    kc = WGRAD_KC[dtype]
    other = -(-cout // WGRAD_BCH) * -(-cin // WGRAD_BCH) * taps
    slabs = -(-blocks_wanted // other)
    slabs = max(1, min(slabs, -(-M // max(kc, WGRAD_SLAB_MIN_PIXELS))))
    slab = -(-(-(-M // slabs)) // kc) * kc
    if ws_bytes > WS_COUNTER_BYTES and other * 4 <= WS_COUNTER_BYTES:
        fit = (ws_bytes - WS_COUNTER_BYTES) // (WGRAD_BCH * WGRAD_BCH * 4) // other
        if fit >= 1 and slabs > fit:
            slabs = fit
            slab = -(-(-(-M // slabs)) // kc) * kc
    return -(-M // slab), slab


def wgrad_max_slabs(M):
    """no launch, single or grouped, splits M pixels into more slabs than this (wgrad_prepare's max_slabs)"""
    return -(-M // WGRAD_SLAB_MIN_PIXELS)


def wgrad_ksplits(cout, cin):
    """the pixel splits of the narrow tiles (csrc/wgrad.hip `ksplit`, atomics mode): the set over the 64 x 64 channel tiles of a problem"""
    def narrow(c):
        return [c - t * WGRAD_BCH <= 32 for t in range(-(-c // WGRAD_BCH))]
    return {(2 if a else 1) * (2 if b else 1) for a in narrow(cout) for b in narrow(cin)}


def _cols(x, k, stride, pad):
    """im2col: (N, C k k, Ho Wo), zero outside the image"""
    if pad < 0:
        x, pad = x[:, :, -pad:, -pad:], 0
    return F.unfold(x, k, padding=pad, stride=stride)


def wgrad_ref(x, dy, k, stride, pad):
    """fp64 weight gradient [Cout][Cin][R][S] of conv(x) for the output gradient dy, the same contraction on absolute values, and P[r][s],
    the number of output pixels whose tap (r, s) lands inside the image (as a (1, 1, R, S) tensor)"""
    N, cout = dy.shape[:2]
    cin = x.shape[1]
    a = dy.reshape(N, cout, -1)
    cols = _cols(x, k, stride, pad)
    assert cols.shape[2] == a.shape[2], (tuple(cols.shape), tuple(a.shape))
    ref = torch.einsum("nol,nkl->ok", a, cols).view(cout, cin, k, k)
    mag = torch.einsum("nol,nkl->ok", a.abs(), cols.abs()).view(cout, cin, k, k)
    P = _cols(torch.ones(N, 1, x.shape[2], x.shape[3], dtype=torch.float64), k, stride, pad).sum((0, 2)).view(1, 1, k, k)
    return ref, mag, P


def wgrad_bound(mag, P, S, base=None, p_max=WGRAD_P_MAX):
    """dw (fp32 in both dtypes) = base + sum_m dy x, per element:
        |got - ref| <= (P + S + 1) 2^-23 sum_m |dy x| + S 2^-23 |base| + 2^-24
    P accumulator roundings: one per pixel whose tap lands inside the image, what a serial fp32 accumulation performs (a masked pixel
    adds an exact zero; the products of bf16 operands are exact in fp32).  The matrix cores add several pixels per instruction - two in
    the fp32 MFMA, sixteen in the bf16 one - and are taken to round no more often than once per product added; E32 per rounding leaves
    room for one that truncates.  S roundings for the one atomic or ordered add per slab, on the running sum and on what the gradient
    tensor held (`base`); one spare for the narrow tiles' pixel shares meeting in the atomics.  The fp32 kernel in split mode
    (fs_set_fp32_split(1), the default) contracts three-way bf16 splits of the operands and drops only the low x low partial products,
    2^-32 of |dy x| each: inside the bound, no term of its own (its eight MFMAs per 16 pixels update the accumulator eight times per 16
    pixels, fewer than once per pixel).
    The bound is only as sharp as P^2 2^-23 is small: P <= p_max is asserted (p_max=None for a caller that knows and says why)."""
    assert p_max is None or float(P.max()) <= p_max, "P = %d: a lost pixel would hide in the bound" % int(P.max())
    b = (P + S + 1) * E32 * mag + TINY
    if base is not None:
        b = b + S * E32 * base.abs()
    return b


def dgrad_s2_ref(x_shape, w, dy, stride, pad):
    """fp64 data gradient of the stride-2 convolution, the same contraction on absolute values, and K per element: the taps that meet a
    real pixel for the element's output-parity class (1 / 2 / 2 / 4 of 9 for a 3x3; the largest count over the class, a border pixel's
    missing taps add exact zeros) times Cout.  Classes without any tap have K = 0."""
    def back(w_, dy_):
        x0 = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
        conv64(x0, w_, stride, pad).backward(dy_)
        return x0.grad
    ref, mag = back(w, dy), back(w.abs(), dy.abs())
    cnt = back(torch.ones_like(w[:1, :1]).expand(1, x_shape[1], -1, -1).contiguous(), torch.ones_like(dy[:, :1]))[:, :1]
    K = torch.zeros_like(cnt)
    for a in range(2):
        for b in range(2):
            cls = cnt[:, :, a::2, b::2]
            if cls.numel():
                K[:, :, a::2, b::2] = float(cls.max())
    return ref, mag, K * w.shape[0]


def cand_range(in_size, out_size):
    """csrc/resize.hip cand_range restated in fp32: per input index i the output range [lo, hi] the backward gather visits"""
    f = np.float32
    scale = f(in_size - 1) / f(out_size - 1) if out_size > 1 else f(0)
    i = np.arange(in_size)
    if scale <= 0:
        return np.zeros(in_size, dtype=np.int64), np.full(in_size, out_size - 1, dtype=np.int64)
    inv = f(1) / scale
    lo = np.floor((i - 1).astype(f) * inv).astype(np.int64) - 1
    hi = np.ceil((i + 1).astype(f) * inv).astype(np.int64) + 1
    return np.clip(lo, 0, None), np.clip(hi, None, out_size - 1)


def tap_matrix(in_size, out_size):
    """(out, in) fp64 matrix of the forward's tap weights, tests/_resize_ref.taps: w[o][i] = l0 [i0 == i] + l1 [i1 == i]"""
    i0, i1, l0, l1 = R.taps(in_size, out_size)
    w = torch.zeros(out_size, in_size, dtype=torch.float64)
    o = torch.arange(out_size)
    w[o, torch.from_numpy(i0).long()] += torch.from_numpy(l0)
    w[o, torch.from_numpy(i1).long()] += torch.from_numpy(l1)
    return w


def near_matrix(in_size, out_size):
    """(out, in) 0 / 1: output o lies in the widened candidate range of input i"""
    lo, hi = cand_range(in_size, out_size)
    o = np.arange(out_size)[:, None]
    return torch.from_numpy(((o >= lo[None, :]) & (o <= hi[None, :])).astype(np.float64))


def resample_bwd(dtype, dy, yo, in_hw, relu, extra=0):
    """bilinear backward dx[i] = sum_o w(o, i) g[o], g = dy [y_out > 0] (N, C, Ho, Wo fp64) -> (ref, bound), (N, C, Hi, Wi):
        (n_o + 2 + extra) 2^-23 sum_o |w g|  +  2^-24 (Hi + Wi) sum_{o near i} |g[o]|  +  UNIT (|ref| + the above)  +  2^-24
    n_o contributing outputs: per output the product wh * ww, the product with g and the accumulation, n_o + 2 roundings on sum |w g|
    (`extra` = 1 for the separable NCHW form, which rounds the row pass's intermediate once more).  The second term is the weight
    uncertainty `_resample` documents: make_tap may be contracted into an fma, so a weight - or the pixel a near-integer tap is attributed
    to - moves by at most half an ulp of the source coordinate, 2^-24 * in_size per axis, at any output the gather visits ("near": the
    widened candidate range of i).  Then one store in `dtype`."""
    hi_, wi_ = in_hw
    g = dy * (yo > 0).double() if relu else dy
    wh, ww = tap_matrix(hi_, dy.shape[2]), tap_matrix(wi_, dy.shape[3])
    ref = torch.einsum("ah,ncab,bw->nchw", wh, g, ww)
    mag = torch.einsum("ah,ncab,bw->nchw", wh, g.abs(), ww)
    near = torch.einsum("ah,ncab,bw->nchw", near_matrix(hi_, dy.shape[2]), g.abs(), near_matrix(wi_, dy.shape[3]))
    n_o = (wh > 0).sum(0).double()[:, None] * (ww > 0).sum(0).double()[None, :]
    e = (n_o + 2 + extra) * E32 * mag + TINY * (hi_ + wi_) * near
    return ref, e + UNIT[dtype] * (ref.abs() + e) + TINY


BN_BWD_ROUNDINGS = 9


def bn_bwd(dtype, z, dy, yo, mean, invstd, gamma, relu, dg_acc=None, db_acc=None):
    """BatchNorm(+ReLU) backward on its own inputs: z, dy, y_out (G, n, C) fp64 values of `dtype`, the GIVEN fp32 mean / invstd (G, C)
    and gamma (C).  g = dy [y_out > 0], xh = (z - mu) is, A0 = sum g, A1 = sum g xh, dz = gamma is (g - A0 / n - xh A1 / n).
      eA0 = n 2^-23 sum|g|, eA1 = (n + 3) 2^-23 sum|g xh|: n - 1 additions in any order (wave shuffles, LDS in wave order, block
        partials, atomics), the product, and the two roundings of xh (subtraction, product).
      dz: c = 9 fp32 roundings at most on any term - xh 2, 1 / n 1, xh * A1 * (1 / n) 2, the two subtractions 2, gamma * is and the
        product with it 2 (the A0 term carries 6 of them, g 4) - plus the reductions' errors through 1 / n, then one store:
        |gamma is| [c 2^-23 (|g| + |A0| / n + |xh A1| / n) + (eA0 + |xh| eA1) / n]  +  UNIT (|ref| + that)  +  2^-24.
      dbeta = sum_G A0, dgamma = sum_G A1: the groups' eA plus one rounding per group total added (G 2^-23 sum_G |A|); accumulators
        given: 2^-23 (|acc| + |ref|) more, and the reference is acc + the sum.
    Returns dict(dz, dz_bound, dbeta, dbeta_bound, dgamma, dgamma_bound)."""
    G, n, C = z.shape
    g = dy * (yo > 0).double() if relu else dy
    mu, is_ = mean[:, None, :], invstd[:, None, :]
    xh = (z - mu) * is_
    a0, a1 = g.sum(1, keepdim=True), (g * xh).sum(1, keepdim=True)
    e0, e1 = n * E32 * g.abs().sum(1, keepdim=True), (n + 3) * E32 * (g * xh).abs().sum(1, keepdim=True)
    k = (gamma.view(1, 1, C) * is_)
    ref = k * (g - a0 / n - xh * a1 / n)
    e = k.abs() * (BN_BWD_ROUNDINGS * E32 * (g.abs() + a0.abs() / n + (xh * a1).abs() / n) + (e0 + xh.abs() * e1) / n)
    out = dict(dz=ref, dz_bound=e + UNIT[dtype] * (ref.abs() + e) + TINY)
    for name, a, ea, acc in (("dbeta", a0, e0, db_acc), ("dgamma", a1, e1, dg_acc)):
        tot = a.sum(0).view(C)
        b = ea.sum(0).view(C) + G * E32 * a.abs().sum(0).view(C) + TINY
        out[name], out[name + "_bound"] = tot, b
        if acc is not None:
            out[name + "_acc"], out[name + "_acc_bound"] = acc + tot, b + E32 * (acc.abs() + tot.abs())
    return out


def bn_operands(dtype, G, n, C, relu, seed):
    """operands of a BatchNorm backward: z with a non-zero mean, the saved statistics computed in fp64 and rounded ONCE to fp32"""
    z = rnd16(dtype, G, n, C, seed=seed).mul(1.5).add(0.3).to(dtype).double()
    dy = rnd16(dtype, G, n, C, seed=seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    gamma = (torch.randn(C, generator=g).abs() + 0.5).double()
    beta = (torch.randn(C, generator=g) * 0.2).double()
    mean = z.mean(1).float().double()
    invstd = (1.0 / torch.sqrt(z.var(1, unbiased=False) + 1e-5)).float().double()
    y = gamma * (z - mean[:, None]) * invstd[:, None] + beta
    yo = (F.relu(y) if relu else y).to(dtype).double()
    return z, dy, yo, mean, invstd, gamma


def old_bars(err, ref):
    """how many elements the three older bars flag: 2e-2 max|ref|, 2e-4 max|ref| + 1e-4, 1e-4 + 1e-4 |ref|"""
    m = float(ref.abs().max())
    return int((err > 2e-2 * m).sum()), int((err > 2e-4 * m + 1e-4).sum()), int((err > 1e-4 + 1e-4 * ref.abs()).sum())


# =========================================================================================================================================
# The train-mode BatchNorm forward.  An any-order fp32 sum of n terms has to be allowed n roundings, and at a few thousand pixels that
# allowance hides a lost pixel.  The sharp instrument is the "grid" family of operands: z = j / 16 with small integers j, whose sums
# and sums of squares are exact in fp32 in ANY order (atomics, wave shuffles, block partials, s2 += v * v contracted into an fma or
# not), so the bound has no term in n.  Every grid value is a bf16 number.  The "normal" family is the older tests' 1.5 N(0, 1) + 0.3.
# =========================================================================================================================================
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
BN_GRID_DEN, BN_GRID_JMAX = 16, 64
BN_NORMAL_N_MAX = 2048                  # n^2 2^-23 <= 1/2, the reasoning of WGRAD_P_MAX: one lost pixel stands out of n roundings


def f32(v):
    """the fp32 number nearest to a Python float, as a Python float (eps and momentum reach the kernels as fp32 arguments)"""
    return float(np.float32(v))


def bn_fwd_operands(dtype, G, n, C, seed, family, jmax=BN_GRID_JMAX):
    """(z (G, n, C), gamma, beta, rm0, rv0 (C)) in fp64; z values of `dtype`, the parameters fp32 numbers.  One gamma is negative.
    family="grid": z = j / 16, j uniform in [-jmax / 4, jmax]: a non-zero mean, so E[z^2] - m^2 cancels about half its bits.  Channel 0
    is constant (j = 3 jmax / 4: its variance is exactly 0, var clamps and invstd = 1 / sqrt(eps)), channel 1 has a small variance on
    a large mean (j in {jmax - 1, jmax}).  sum_n j^2 < 2^24 and n max|j| < 2^24 per (group, channel) are asserted: every partial sum
    of z and of z^2 is then an integer multiple of 2^-8 below 2^16, exact in fp32.  A caller with more pixels than jmax = 64 allows
    narrows jmax; the assertion stays.
    family="normal": 1.5 N(0, 1) + 0.3 rounded to `dtype`, at most BN_NORMAL_N_MAX pixels per group."""
    g = torch.Generator().manual_seed(seed)
    if family == "grid":
        assert jmax % 4 == 0 and 4 <= jmax <= BN_GRID_JMAX
        j = torch.randint(-jmax // 4, jmax + 1, (G, n, C), generator=g).double()
        j[:, :, 0] = 3 * jmax // 4
        if C > 1:
            j[:, :, 1] = torch.randint(jmax - 1, jmax + 1, (G, n), generator=g).double()
        assert float((j * j).sum(1).max()) < 2.0 ** 24, "sum j^2 = %d: the sums of squares would round" % int((j * j).sum(1).max())
        assert n * float(j.abs().max()) < 2.0 ** 24
        z = j / BN_GRID_DEN
        assert bool((z.to(torch.bfloat16).double() == z).all())
    else:
        assert family == "normal", family
        assert n <= BN_NORMAL_N_MAX, "n = %d: a lost pixel would hide in a bound of n roundings" % n
        z = torch.randn(G, n, C, generator=g).to(dtype).double().mul(1.5).add(0.3).to(dtype).double()
    gamma = (torch.randn(C, generator=g).abs() + 0.5).float().double()
    gamma[C // 2] = -gamma[C // 2]
    beta = (torch.randn(C, generator=g) * 0.2).float().double()
    rm0 = (torch.randn(C, generator=g) * 0.1).float().double()
    rv0 = (torch.randn(C, generator=g).abs() + 0.5).float().double()
    return z, gamma, beta, rm0, rv0


def bn_fwd(dtype, z, gamma, beta, rm0, rv0, relu_from, exact_sums, eps=BN_EPS, momentum=BN_MOMENTUM):
    """Train-mode BatchNorm (+ReLU from channel `relu_from` on; None: no ReLU, 0: every channel) of z (G, n, C), G groups normalised
    independently with the same parameters, running statistics updated group after group.  References in fp64 and per-element bounds:
      s1 = sum z, s2 = sum z^2 in any order: e1 = n 2^-23 sum|z|, e2 = (n + 1) 2^-23 sum z^2 (the product too); both 0 with exact_sums
      m = s1 / n:    em = e1 / n + 2^-23 |m|;      q = s2 / n:    eq = e2 / n + 2^-23 q
      var = max(q - m^2, 0):   ev = eq + 2 |m| em + em^2 + 2 2^-23 (q + m^2)        (product and subtraction, fused or not)
      invstd = 1 / sqrt(var + eps) as an INTERVAL: [(1 - 3 2^-23) / sqrt(var + ev + eps), (1 + 3 2^-23) / sqrt(max(var - ev, 0) + eps)]
        (add, sqrt, divide).  No first-order form: at a constant channel ev is of the size of eps.  e_is = the wider side.
      scale = gamma invstd:   e_sc = |gamma| e_is + 2^-23 (|scale| + |gamma| e_is)
      shift = beta - m scale: e_sh = |m| e_sc + |scale| em + em e_sc + 2 2^-23 (|beta| + |m scale| + |m| e_sc + |scale| em)
      y = z scale + shift:    e_y = |z| e_sc + e_sh + 2 2^-23 (|z scale| + |shift| + |z| e_sc + e_sh), or the form below that takes
        the scale's error once, whichever is smaller; ReLU is 1-Lipschitz; one store.
      running statistics r <- (1 - momentum) r + momentum v per group in order, as `_stage` propagates: four roundings (1 - momentum,
        two products, the sum) on the terms and on the errors carried in; v = m, or var n / (n - 1) with two more roundings.
    Returns mean / invstd / scale / shift (G, C) with *_bound (invstd also invstd_lo, invstd_hi), saved / saved_bound (G, 4, C),
    y / y_bound (G, n, C), rm / rv with *_bound (C), stats = [s1 | s2] (G, 2 C)."""
    G, n, C = z.shape
    eps, momentum = f32(eps), f32(momentum)
    s1, s2 = z.sum(1), (z * z).sum(1)
    e1, e2 = (0.0, 0.0) if exact_sums else (n * E32 * z.abs().sum(1), (n + 1) * E32 * s2)
    m, q = s1 / n, s2 / n
    em, eq = e1 / n + E32 * m.abs(), e2 / n + E32 * q
    var = (q - m * m).clamp(min=0.0)
    ev = eq + 2 * m.abs() * em + em * em + 2 * E32 * (q + m * m)
    is_ = 1.0 / torch.sqrt(var + eps)
    lo, hi = (1 - 3 * E32) / torch.sqrt(var + ev + eps), (1 + 3 * E32) / torch.sqrt((var - ev).clamp(min=0.0) + eps)
    e_is = torch.maximum(hi - is_, is_ - lo)
    ga, be = gamma.view(1, C), beta.view(1, C)
    scale = ga * is_
    e_sc = ga.abs() * e_is + E32 * (scale.abs() + ga.abs() * e_is)
    shift = be - m * scale
    e_sh = m.abs() * e_sc + scale.abs() * em + em * e_sc + 2 * E32 * (be.abs() + (m * scale).abs() + m.abs() * e_sc + scale.abs() * em)
    sc, sh, esc, esh = scale[:, None], shift[:, None], e_sc[:, None], e_sh[:, None]
    y = z * sc + sh
    e_y = z.abs() * esc + esh + 2 * E32 * ((z * sc).abs() + sh.abs() + z.abs() * esc + esh)
    # the same y, with the scale's error taken ONCE: every body multiplies z and (inside shift) m by one and the same computed invstd, so
    # y^ - y = (z - m)(s^ - s) + (m - m^) s^ + roundings.  Three roundings on shift's terms (m * gamma * invstd is two products where
    # scale is one, and the subtraction), two on y's.  Both forms hold; the smaller is the bound.  This one keeps e_is out of a channel
    # whose values lie close to its mean - the constant channel above all, where y = beta whatever invstd is.
    mm, emm = m[:, None], em[:, None]
    s_hi = sc.abs() + esc
    e_yc = (z - mm).abs() * esc + emm * s_hi + 3 * E32 * (be.abs() + (mm.abs() + emm) * s_hi) + 2 * E32 * (z.abs() * s_hi + sh.abs() + esh)
    e_y = torch.minimum(e_y, e_yc)
    if relu_from is not None:
        y = torch.cat([y[..., :relu_from], F.relu(y[..., relu_from:])], -1)
    out = dict(mean=m, mean_bound=em, invstd=is_, invstd_bound=e_is, invstd_lo=lo, invstd_hi=hi, scale=scale, scale_bound=e_sc, shift=shift,
               shift_bound=e_sh, y=y, y_bound=e_y + UNIT[dtype] * (y.abs() + e_y) + TINY, stats=torch.cat([s1, s2], 1))
    out["saved"], out["saved_bound"] = torch.stack([m, is_, scale, shift], 1), torch.stack([em, e_is, e_sc, e_sh], 1)
    unb = n / (n - 1.0) if n > 1 else 1.0
    vu, evu = var * unb, (ev + (2 * E32 * (var + ev) if n > 1 else 0.0)) * unb
    keep = 1.0 - momentum
    for name, r, v, e_v in (("rm", rm0.clone(), m, em), ("rv", rv0.clone(), vu, evu)):
        er = torch.zeros_like(r)
        for g in range(G):
            er = keep * er + momentum * e_v[g] + 4 * E32 * (keep * (r.abs() + er) + momentum * (v[g].abs() + e_v[g]))
            r = keep * r + momentum * v[g]
        out[name], out[name + "_bound"] = r, er
    return out


def assert_between(got, lo, hi, what):
    got = got.detach().double().cpu()
    bad = ~((got >= lo) & (got <= hi))                                          # a NaN is outside
    print("%s: worst position in [lo, hi] %.3f" % (what, float(((got - lo) / (hi - lo)).max())))
    assert not bool(bad.any()), "%s: %d of %d outside the interval" % (what, int(bad.sum()), got.numel())


BN_FWD_OUTPUTS = ("mean", "invstd", "scale", "shift", "y", "rm", "rv")


def bn_fwd_check(want, got, what, only=BN_FWD_OUTPUTS):
    """got: dict with any of saved (G, 4, C), y (G, n, C), rm, rv (C), every one finite and within its bound at every element; the inverse
    deviation within its interval too"""
    got = {k: v.detach().double().cpu() for k, v in got.items()}
    if "saved" in got:
        sv = got.pop("saved").reshape(want["saved"].shape)
        got.update(mean=sv[:, 0], invstd=sv[:, 1], scale=sv[:, 2], shift=sv[:, 3])
    for k in only:
        if k in got:
            v = got[k].reshape(want[k].shape)
            assert bool(torch.isfinite(v).all()), "%s %s: %d elements are not finite (never written?)" % (what, k, int((~torch.isfinite(v)).sum()))
            assert_within(v, want[k], want[k + "_bound"], "%s %s" % (what, k))
            if k == "invstd":
                assert_between(v, want["invstd_lo"], want["invstd_hi"], "%s invstd interval" % what)


def bn_old_bars(dtype, got, want):
    """which outputs the bars of tests/test_bn_group_gpu.py flag (its `_close`: y at 2e-5 + 2e-5 max|ref| in fp32 and 2e-2 max|ref| in bf16;
    mean, invstd and the running statistics at the fp32 bar): the names, in BN_FWD_OUTPUTS order"""
    flagged = []
    for k in ("mean", "invstd", "y", "rm", "rv"):
        ref = want[k]
        err = float((got[k].double().reshape(ref.shape) - ref).abs().max())
        top = float(ref.abs().max())
        tol = 2e-2 * max(top, 1e-3) if (k == "y" and dtype != torch.float32) else 2e-5 + 2e-5 * top
        if not err <= tol:
            flagged.append(k)
    return flagged
