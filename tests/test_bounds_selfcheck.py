"""The per-element bounds of tests/_bounds.py, checked on the CPU: they pass an honest kernel and fail a subtly wrong one.

The "kernel" is a small emulation of what the 16-bit inference kernels do: operands already rounded to the storage type, products and sums
in fp32 in an order that is not the reference's (im2col rows contracted 16 k-values at a time), scale / shift / ReLU in fp32, ONE
round-to-nearest-even store.  It runs for fp16 and bf16 on
  * the 3x3 convolution 2x40x9x33 -> 128 (channel tail, ragged width, four 32-channel output tiles),
  * a `_stage -> _stage` chain, 3x3 (scale, shift, ReLU, stored) -> 1x1 (scale, shift),
  * a `_resample -> _stage` chain, 5x8 -> 9x24 (ReLU, stored) -> 3x3.
The honest emulation must lie within the bound everywhere.  Planted defects, each of which must put at least one element above it:
  1. the store truncates instead of rounding to nearest even;
  2. one operand (x) loses its last significand bit;
  3. one product is missing at one pixel (all output channels of that pixel);
  4. one tap is missing on the last column;
  5. the last 8 input channels are missing;
  7. two bilinear tap weights are swapped on the last output column.  With align_corners=True the last column lands on the last source
     pixel and both taps read it - a swap changes nothing - unless the fp32 product scale * dst falls short of in - 1.  8 -> 24 is such a
     width (asserted: the taps are pixels 6 and 7 with weights ~0 and ~1), so the defect changes the result there.
Defect 6, the intermediate map of a chain kept in fp32 where the kernel stores it in 16 bits, deviates from the contract in the benign
direction; whether it exceeds the bound is printed and recorded in DESIGN.md, not asserted.
On the exact grids of the GPU tests (x = j / 512 for fp16, j / 256 for bf16, w = j / 8: every partial sum exact in fp32) the honest
emulation gives the bits of round-to-nearest-even of the exact sum, and defects 1-5 each change at least one output bit (defect 2 for
bf16 only: the fp16 grid never sets the 11th significand bit, so clearing it leaves the exact sum unchanged).
For the record each test prints how many elements the tensor-wide bar of the older bf16 tests, 2e-2 * max|ref|, flags (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

from tests import _bounds as B
from tests import _resize_ref as R

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
DEFECTS = ["truncating_store", "operand_bit_lost", "product_dropped", "tap_dropped_last_column", "channel_tail_dropped"]


# ---- the emulated kernel ---------------------------------------------------------------------------------------------------------------
def store16(v32, dtype, truncate=False):
    """fp32 -> storage type, as float64: round to nearest even, or (defect 1) toward zero"""
    r = v32.to(dtype)
    if truncate:                                                               # where rounding went away from zero, one step back
        over = r.float().abs() > v32.abs()
        r = torch.where(over, (r.view(torch.int16) - 1).view(dtype), r)        # sign-magnitude: bits - 1 is one ulp toward zero
    return r.double()


def clear_last_bit(x64, dtype):
    return (x64.float().to(dtype).view(torch.int16) & ~1).view(dtype).double()


def emu_conv(x64, w64, dtype, scale=None, shift=None, relu=False, pad=1, defect=None, store=True):
    """(N, Cin, H, W) x (Cout, Cin, R, R) at stride 1: fp32 im2col contraction in 16-wide k-steps, fp32 epilogue, one store"""
    N, cin, H, W = x64.shape
    cout, _, ks, _ = w64.shape
    if defect == "operand_bit_lost":
        x64 = clear_last_bit(x64, dtype)
    A = F.unfold(x64.float(), ks, padding=pad).transpose(1, 2).reshape(N * H * W, cin, ks * ks).clone()      # [pixel][channel][tap]
    if defect == "product_dropped":
        A[(H // 2) * W + W // 2, cin // 2, ks * ks // 2] = 0.0                 # image 0, the centre pixel, one channel of the centre tap
    if defect == "tap_dropped_last_column":
        A.view(N, H, W, cin, ks * ks)[:, :, W - 1, :, 0] = 0.0
    if defect == "channel_tail_dropped":
        A[:, cin - 8:] = 0.0
    A = A.reshape(N * H * W, cin * ks * ks)
    Wm = w64.float().reshape(cout, cin * ks * ks).t().contiguous()
    acc = torch.zeros(N * H * W, cout, dtype=torch.float32)
    for k0 in range(0, A.shape[1], 16):
        acc = acc + A[:, k0:k0 + 16] @ Wm[k0:k0 + 16]
    if scale is not None:
        acc = acc * scale.float() + shift.float()
    if relu:
        acc = F.relu(acc)
    out = acc.view(N, H, W, cout).permute(0, 3, 1, 2)
    return store16(out, dtype, truncate=(defect == "truncating_store")) if store else out.double()


def emu_resample(x64, size, dtype, relu=False, swap_last_column=False, store=True):
    """bilinear, align_corners=True, with the fp32 taps of tests/_resize_ref.py and the blend in fp32; one store"""
    h0, h1, a0, a1 = R.taps(x64.shape[2], size[0])
    w0, w1, b0, b1 = R.taps(x64.shape[3], size[1])
    a0, a1, b0, b1 = (torch.from_numpy(t).float() for t in (a0, a1, b0, b1))
    if swap_last_column:
        b0, b1 = b0.clone(), b1.clone()
        b0[-1], b1[-1] = b1[-1].item(), b0[-1].item()
    x = x64.float()
    top = x[:, :, h0][:, :, :, w0] * b0 + x[:, :, h0][:, :, :, w1] * b1
    bot = x[:, :, h1][:, :, :, w0] * b0 + x[:, :, h1][:, :, :, w1] * b1
    o = top * a0[:, None] + bot * a1[:, None]
    if relu:
        o = F.relu(o)
    return store16(o, dtype) if store else o.double()


def flagged(got, ref, bound, what):
    """elements above the per-element bound; prints both bars' counts"""
    err = (got - ref).abs()
    new, old = int((err > bound).sum()), int((err > 2e-2 * float(ref.abs().max())).sum())
    print("%-44s worst err / bound %9.3f   above the bound %6d   above 2e-2 max|ref| %6d   of %d"
          % (what, float((err / bound).max()), new, old, err.numel()))
    return new


# ---- 1. the single 3x3 convolution -----------------------------------------------------------------------------------------------------
_cache = {}


def conv_case(dtype):
    """operands, fp64 reference and bound of 2x40x9x33 -> 128, computed once per dtype and left unchanged"""
    if dtype not in _cache:
        N, cin, H, W, cout = 2, 40, 9, 33, 128
        x = B.rnd16(dtype, N, cin, H, W, seed=240)
        w = B.rnd16(dtype, cout, cin, 3, 3, seed=241, scale=(2.0 / (cin * 9)) ** 0.5)
        ref, mag = B.conv64(x, w, 1, 1), B.conv64(x.abs(), w.abs(), 1, 1)
        _cache[dtype] = (x, w, ref, B.single_bound(dtype, ref, mag, 9 * cin))
    return _cache[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_honest_conv_is_within_the_bound(dtype):
    x, w, ref, bound = conv_case(dtype)
    B.assert_within(emu_conv(x, w, dtype), ref, bound, "honest 3x3 conv, %s" % dtype)
    assert flagged(emu_conv(x, w, dtype), ref, bound, "honest %s" % dtype) == 0


@pytest.mark.parametrize("defect", DEFECTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_conv_defect_is_above_the_bound(dtype, defect):
    x, w, ref, bound = conv_case(dtype)
    assert flagged(emu_conv(x, w, dtype, defect=defect), ref, bound, "%s %s" % (defect, dtype)) >= 1


# ---- 2. chains -------------------------------------------------------------------------------------------------------------------------
def stage_chain(dtype, keep_fp32=False):
    """3x3 40 -> 64 (scale, shift, ReLU, stored) -> 1x1 64 -> 19 (scale, shift) on 2 x 7 x 17"""
    N, cin, H, W, c3, cout = 2, 40, 7, 17, 64, 19
    x = B.rnd16(dtype, N, cin, H, W, seed=440)
    w3 = B.rnd16(dtype, c3, cin, 3, 3, seed=441, scale=(2.0 / (9 * cin)) ** 0.5)
    w2 = B.rnd16(dtype, cout, c3, 1, 1, seed=442, scale=(2.0 / c3) ** 0.5)
    g = torch.Generator().manual_seed(443)
    s3, b3 = (torch.rand(c3, generator=g) + 0.5).double(), (torch.randn(c3, generator=g) * 0.5).double()
    s2, b2 = (torch.rand(cout, generator=g) + 0.5).double(), (torch.randn(cout, generator=g) * 0.5).double()
    t, e = B._stage(dtype, x, None, w3, s3, b3, True)
    ref, bound = B._stage(dtype, t, e, w2, s2, b2, False, pad=0)
    mid = emu_conv(x, w3, dtype, s3, b3, True, store=not keep_fp32)
    return emu_conv(mid, w2, dtype, s2, b2, False, pad=0), ref, bound


def resample_chain(dtype, keep_fp32=False, swap=False):
    """bilinear 5 x 8 -> 9 x 24 (ReLU, stored) -> 3x3 40 -> 32 (ReLU)"""
    N, cin, cout, size = 2, 40, 32, (9, 24)
    x = B.rnd16(dtype, N, cin, 5, 8, seed=340)
    w = B.rnd16(dtype, cout, cin, 3, 3, seed=341, scale=(2.0 / (9 * cin)) ** 0.5)
    w0, w1, b0, b1 = R.taps(8, size[1])
    assert (w0[-1], w1[-1]) == (6, 7) and b0[-1] != b1[-1], "the last column must blend two different pixels, or a swap changes nothing"
    v, e = B._resample(dtype, x, None, size, relu=True)
    ref, bound = B._stage(dtype, v, e, w, None, None, True)
    mid = emu_resample(x, size, dtype, relu=True, swap_last_column=swap, store=not keep_fp32)
    return emu_conv(mid, w, dtype, relu=True), ref, bound


@pytest.mark.parametrize("chain", [stage_chain, resample_chain], ids=["stage-stage", "resample-stage"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_honest_chain_is_within_the_propagated_bound(dtype, chain):
    got, ref, bound = chain(dtype)
    B.assert_within(got, ref, bound, "honest %s, %s" % (chain.__name__, dtype))
    got, ref, bound = chain(dtype, keep_fp32=True)                             # defect 6: recorded, not asserted (module docstring)
    flagged(got, ref, bound, "intermediate kept in fp32, %s %s" % (chain.__name__, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_swapped_tap_weights_are_above_the_bound(dtype):
    got, ref, bound = resample_chain(dtype, swap=True)
    assert flagged(got, ref, bound, "tap weights swapped on the last column, %s" % dtype) >= 1


# ---- 3. exact grids --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_grid_defects_change_bits(dtype):
    N, cin, H, W, cout = 1, 32, 5, 7, 32                                      # the rule_5x7 case of the GPU files
    x = B.grid(N, cin, H, W, seed=21, den=512 if dtype == torch.float16 else 256, lim=512 if dtype == torch.float16 else 256)
    w = B.grid(cout, cin, 3, 3, seed=22, den=8, lim=8)
    assert bool((x.float().to(dtype).double() == x).all())
    uses_last_bit = bool((clear_last_bit(x, dtype) != x).any())               # j / 256 fills bf16's 8 bits; j / 512 needs 10 of fp16's 11,
    assert uses_last_bit == (dtype == torch.bfloat16)                         # so defect 2 leaves the exact fp16 sum as it is
    want = B.bits(B.rne16(dtype, B.conv64(x, w, 1, 1)))
    assert torch.equal(B.bits(emu_conv(x, w, dtype).to(dtype)), want), "the honest emulation must give the bits of the correctly rounded exact sum"
    for defect in DEFECTS:
        if defect == "operand_bit_lost" and not uses_last_bit:
            continue
        changed = int((B.bits(emu_conv(x, w, dtype, defect=defect).to(dtype)) != want).sum())
        print("%-28s %s: %d of %d outputs change bits" % (defect, dtype, changed, want.numel()))
        assert changed >= 1, defect
