"""Seeded cases of the bf16 matrix-core stem shared by tests/test_stem_pipelined_gpu.py and tools/make_stem_golden.py (which records
what the kernel of the commit before the multi-tile form wrote for them, tests/golden/stem_parent.npz)."""
import torch

COUTS = [32, 64, 24]
IMAGES = [(2, 34, 52), (2, 26, 264), (1, 17, 136),        # the geometries of tests/test_kernels_gpu.py::test_stem_conv
          (2, 70, 520)]                                    # Ho = 35, Wo = 260: 9 x 5 tiles per image, partial tiles at both edges
GOLDEN_FULL_BELOW = 16384                                  # outputs up to this many elements are recorded whole,
GOLDEN_STRIDE = 29                                         # larger ones as every 29th element of the flat (N, Ho, Wo, C) order


def case_id(cout, image):
    return "c%d_%dx3x%dx%d" % ((cout,) + tuple(image))


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def inputs(cout, image):
    """x (N,3,H,W), w (cout,3,3,3), scale, shift: fp32 CPU tensors, the same on every run"""
    n, h, w_ = image
    seed = 1000 * cout + h
    x = _rnd(n, 3, h, w_, seed=seed) * 2.0
    w = _rnd(cout, 3, 3, 3, seed=seed + 1, scale=0.3)
    return x, w, _rnd(cout, seed=seed + 2).abs() + 0.5, _rnd(cout, seed=seed + 3)


def run(cout, image):
    """the bf16 stem output for the case's inputs, as the uint16 bit patterns of the flat (N, Ho, Wo, cout) order (CPU tensor)"""
    from fasterseg_amd import kernels as k
    x, w, scale, shift = inputs(cout, image)
    wp = k.pack_weight(w.cuda(), torch.float32)
    y = k.conv_stem(x.cuda(), wp, cout, scale.cuda(), shift.cuda(), True, torch.bfloat16)       # NHWC view, channel stride = cout
    assert k.channel_stride(y) == cout
    return y.permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().reshape(-1)


def golden_sample(bits):
    return bits if bits.numel() <= GOLDEN_FULL_BELOW else bits[::GOLDEN_STRIDE]
