"""Per-element error bounds of the 16-bit inference kernels against fp64 references, shared by tests/test_f16_kernels_gpu.py,
tests/test_bf16_kernels_gpu.py and tests/test_bounds_selfcheck.py.  Every helper takes the storage dtype; `For(dtype)` binds it, so a
test module names its type once.

UNIT[dtype] is the unit roundoff of one round-to-nearest store: half an ulp relative to the value, 2^-p for a p-bit significand (hidden
bit included).  fp16 has 11 bits, bf16 has 8: 2^-8, not 2^-9 - a correctly rounded bf16 value just above a power of two is off by up to
2^-8 of itself.  Single-stage kernels, per element:
    |got - ref| <= UNIT |ref| + K 2^-23 sum|x w| + 2^-24
(one output rounding + the fp32 accumulation bound; K = taps x channels, 4 for a resample).  Kernels that round an intermediate map to
the storage type get the same bound PROPAGATED stage by stage (`stage`, `resample`): an input known to e gives the contraction
sum|w| e more, scale / shift add two fp32 roundings, and each stored stage adds UNIT (|value| + its error) + 2^-24."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import _resize_ref as R

UNIT = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
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
