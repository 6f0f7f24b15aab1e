"""The tiled NCHW logits up-sample (csrc/resize.hip, bilinear_fwd_nchw_tiled_kernel: a block stages the source window of a 32 x 256 output
tile into LDS once, lanes walk down the rows with the horizontal interpolations in registers) against a host reference
(tests/_resize_ref.py: fp32 taps exactly as make_tap computes them, fp64 blend) and against the gather kernel it replaces.

Bound for the fp32 output: |got - ref| <= 6 * 2^-24 * max|x|.  Each of h0, h1 and the final blend is two products and a sum of values
bounded by max|x| with weights in [0, 1], i.e. at most 3 roundings of at most 2^-24 * max|x| each (fewer where the compiler contracts
a product into an fma), and the two h errors enter the blend with weights that sum to 1: 3 + 3.  bf16 output: plus half a bf16 ulp of
the value.  bf16 keeps 8 significant bits, so half an ulp of v is 2^(floor(log2 |v|) - 8), between 2^-9 |v| and 2^-8 |v|: the exact
half ulp is used here (taken at |ref| plus the fp32 bound, for a value the rounding carries across a power of two); 2^-9 |ref| alone
is below the format's rounding error for most values - a correctly rounded result measured up to exactly 2^(e-8).
Old against new on the same input: both are within 6 of the exact value, so within 12 of each other (bf16 output: plus one ulp where
a rounding boundary lies between the two)."""
import numpy as np
import pytest
import torch

from tests import _resize_ref as R

pytestmark = pytest.mark.gpu

# (N, C, x_cs, (Hi, Wi), (Ho, Wo), tiled?)
CASES = [
    (2, 19, 32, (8, 12), (64, 96), True),          # the shape of tests/test_kernels_gpu.py::test_bilinear_logits_nchw
    (1, 19, 20, (9, 13), (70, 100), True),         # non-integer ratio, partial tile in both directions, tight channel stride
    (1, 4, 4, (2, 2), (40, 264), True),            # two source rows, more than one tile across, one channel group
    (1, 21, 24, (5, 7), (33, 52), True),           # last channel group holds one channel, odd Ho
    (1, 19, 32, (12, 40), (100, 1028), True),      # 4 x 5 tiles of 32 x 256 with remainders in both directions
    (1, 19, 32, (16, 24), (8, 12), False),         # down-sample: the window of a tile does not fit -> gather kernel
    (1, 19, 32, (8, 12), (20, 30), False),         # Wo % 4 != 0: scalar kernel
]
U = 2.0 ** -24


def _input(case, dtype):
    n, c, cs, (hi, wi), _, _ = case
    g = torch.Generator().manual_seed(1000 + 31 * hi + wi + c)
    x = torch.randn(n, c, hi, wi, generator=g).to(dtype)
    buf = torch.randn(n, hi, wi, cs, generator=g).to(dtype)          # the pad channels hold finite junk, as in a live buffer
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return x.float().numpy(), buf


_refs = {}


def _reference(case, dtype):
    key = (case, dtype)
    if key not in _refs:
        x, buf = _input(case, dtype)
        ref = R.upsample(x, case[4])
        ref.setflags(write=False)
        _refs[key] = (float(np.abs(x).max()), buf, ref)
    return _refs[key]


def _run(buf, case, mode):
    from fasterseg_amd import kernels as k
    n, c, cs, (hi, wi), size, _ = case
    view = buf.cuda().permute(0, 3, 1, 2)[:, :c]
    out = k.bilinear(view, size, out_nchw=mode, channels=c)
    torch.cuda.synchronize()
    assert out.is_contiguous() and out.shape == (n, c) + tuple(size)
    return out


@pytest.mark.parametrize("mode", [1, 2], ids=["f32out", "storage_out"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d_%dx%d_to_%dx%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4][0], c[4][1]))
def test_tiled_logits_upsample(case, dtype, mode):
    from fasterseg_amd import _lib
    lib = _lib.lib()
    xmax, buf, ref = _reference(case, dtype)
    try:
        lib.fs_debug_logits_tiled(1)
        new = _run(buf, case, mode)
        lib.fs_debug_logits_tiled(0)
        old = _run(buf, case, mode)
    finally:
        lib.fs_debug_logits_tiled(1)
    out_f32 = mode == 1 or dtype == torch.float32
    assert new.dtype == (torch.float32 if out_f32 else dtype)
    half_ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref) + 6 * U * xmax, 2.0 ** -126))) - 8)       # of bf16, at the value
    tol = 6 * U * xmax + (0.0 if out_f32 else half_ulp)
    for name, got in (("default path", new), ("gather kernel", old)):
        err = np.abs(got.float().cpu().numpy().astype(np.float64) - ref)
        print("%s: max err %.3e = %.2f x 2^-24 max|x| (bound 6)" % (name, err.max(), err.max() / (U * xmax)))
        assert (err <= tol).all(), "%s: max err %.3e, %d of %d above the bound" % (name, err.max(), int((err > tol).sum()), err.size)
    if out_f32:
        d = float((new - old).abs().max())
        print("new - old: %.2f x 2^-24 max|x| (bound 12)" % (d / (U * xmax)))
        assert d <= 12 * U * xmax
    else:        # two bf16 roundings of values 12 * 2^-24 * max|x| apart: one bf16 ulp where a rounding boundary lies between them
        d = (new.float() - old.float()).abs().cpu().numpy()
        assert (d <= 12 * U * xmax + 2 * half_ulp).all()
    if not case[5]:
        assert torch.equal(new, old), "a shape the tiled form does not serve must take the same kernel with the hook on and off"


def test_tiled_form_is_the_one_that_runs():
    """the default path and the gather kernel are different kernels on a shape the tiled form serves: the launch census names what ran"""
    from fasterseg_amd import _lib, census
    lib = _lib.lib()
    case = CASES[0]
    _, buf, _ = _reference(case, torch.bfloat16)
    names = []
    try:
        for on in (1, 0):
            lib.fs_debug_logits_tiled(on)
            with census.recording(2) as rec:
                _run(buf, case, 1)
            names.append(sorted(rec.kernels))
    finally:
        lib.fs_debug_logits_tiled(1)
    assert any("bilinear_fwd_nchw_tiled_kernel" in k for k in names[0]), names
    assert not any("tiled" in k for k in names[1]) and any("bilinear_fwd_nchw_kernel" in k for k in names[1]), names
