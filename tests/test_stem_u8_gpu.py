"""The stem on a uint8 frame (fs_conv_stem_u8_fwd, csrc/stem.hip: the fp32 stem's three kernel bodies behind another image loader).

Contract: byte u of channel c enters the convolution as ((float)u / 255.f - mean[c]) / std[c] in fp32 with IEEE division, padding is
0.0 after normalisation, and nothing behind the loader changes.  So every case asserts BIT equality with fs_conv_stem_fwd fed the
expected input (tests/_u8_cases.py: the same expression in numpy float32) with the same filter, scale, shift and relu - under the same
test hooks, since the hooks choose the kernel form for both entry points.

The 4 x 64 output tile sets the shapes: 2x18x264 gives Ho = 9, Wo = 132, i.e. 3 x 3 tiles per image whose last row tile has one row and
whose last column tile has four columns; 17x262 has W % 4 != 0 and an odd height (direct kernel); 2x4 is the smallest image."""
import pytest
import torch

from tests import _u8_cases as U

pytestmark = pytest.mark.gpu

TILED = (2, 18, 264)
_frames = {}


def _frame(shape, seed=5):
    """(uint8 NHWC frame, expected fp32 NCHW input) as host arrays: built once per shape, shared, never modified"""
    key = tuple(shape) + (seed,)
    if key not in _frames:
        img = U.frame(*shape, seed=seed)
        n, h, w = shape
        assert U.covers_every_byte(img) or h * w < 256
        assert (img[:, -1] == 255).all() and (img[:, :, -1] == 255).all()
        _frames[key] = (img, U.expected(img))
    return _frames[key]


def _weights(cout):
    g = torch.Generator().manual_seed(100 + cout)
    rnd = lambda *s: torch.randn(*s, generator=g)
    return (rnd(cout, 3, 3, 3) * 0.3).cuda(), (rnd(cout).abs() + 0.5).cuda(), rnd(cout).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _sentinel_out(n, ho, wo, cout, cs, dtype):
    raw_t, pattern = (torch.int16, 0x5A5A) if dtype == torch.bfloat16 else (torch.int32, 0x5A5A5A5A)
    buf = torch.full((n, ho, wo, cs), pattern, dtype=raw_t, device="cuda")
    return buf, pattern, buf.view(dtype).permute(0, 3, 1, 2)[:, :cout]


def _pair(shape, cout, dtype, relu=True, affine=True, cs=None, img_dev=None, x_dev=None):
    """(bits of fs_conv_stem_u8_fwd on the frame, bits of fs_conv_stem_fwd on the expected input): whole output buffers"""
    from fasterseg_amd import kernels as K
    img, x = _frame(shape)
    n, h, w = shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    wt, scale, shift = _weights(cout)
    wp = K.pack_weight(wt, torch.float32)
    if not affine:
        scale = shift = None
    if img_dev is None:
        img_dev = torch.from_numpy(img).cuda()
    if x_dev is None:
        x_dev = torch.from_numpy(x).cuda()
    cs = cs or K.round_up(cout, K.vec_of(dtype))
    outs = []
    for u8 in (True, False):
        buf, pattern, view = _sentinel_out(n, ho, wo, cout, cs, dtype)
        if u8:
            K.conv_stem_u8(img_dev, wp, cout, scale, shift, relu, dtype, U.MEAN, U.STD, out=view)
        else:
            K.conv_stem(x_dev, wp, cout, scale, shift, relu, dtype, out=view)
        torch.cuda.synchronize()
        if cs > cout:
            assert (buf[..., cout:] == pattern).all(), "channels %d..%d lost the sentinel (%s)" % (cout, cs - 1, "uint8" if u8 else "fp32")
        assert not (buf[..., :cout] == pattern).all()
        outs.append(buf)
    return outs


def _assert_same(got, want, what):
    diff = int((got != want).sum())
    assert torch.equal(got, want), "%s: %d of %d values differ from fs_conv_stem_fwd on the expected input" % (what, diff, want.numel())


@pytest.mark.parametrize("cout", [32, 40, 64])
def test_mfma_kernel_partial_tiles(cout):
    """bf16: the pipelined MFMA kernel, NT = 1 (32), a partial second n-tile (40) and NT = 2 (64)"""
    _assert_same(*_pair(TILED, cout, torch.bfloat16), "MFMA Cout=%d" % cout)


def test_lds_kernel_fp32():
    _assert_same(*_pair(TILED, 32, torch.float32), "LDS-tiled fp32")


def test_lds_kernel_bf16():
    from fasterseg_amd import _lib
    lib = _lib.lib()
    try:
        lib.fs_debug_stem_mfma(0)
        got, want = _pair(TILED, 32, torch.bfloat16)
    finally:
        lib.fs_debug_stem_mfma(1)
    _assert_same(got, want, "LDS-tiled bf16")
    mfma, _ = _pair(TILED, 32, torch.bfloat16)
    assert not torch.equal(got, mfma), "the hook did not change the kernel form"       # split-bf16 MFMA sums round differently


@pytest.mark.parametrize("blocks", [1, 3])
@pytest.mark.parametrize("cout", [32, 64])
def test_one_block_walks_every_tile(cout, blocks):
    """18 tiles on 1 or 3 blocks: every block alternates both window buffers; same bits as the fp32 source and as the default grid"""
    from fasterseg_amd import _lib
    lib = _lib.lib()
    try:
        lib.fs_debug_stem_blocks(blocks)
        got, want = _pair(TILED, cout, torch.bfloat16)
    finally:
        lib.fs_debug_stem_blocks(0)
    _assert_same(got, want, "%d block(s)" % blocks)
    default, _ = _pair(TILED, cout, torch.bfloat16)
    _assert_same(got, default, "%d block(s) against the default grid" % blocks)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_direct_kernel_odd_geometry(dtype):
    """H = 17, W = 262: W % 4 != 0 takes the direct kernel with byte loads"""
    _assert_same(*_pair((1, 17, 262), 32, dtype), "direct")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_image_base_offset_by_one_byte(dtype):
    """A frame that starts one byte into a larger buffer: the dispatch promises the direct kernel for a base that is not 4-byte aligned.
    The expected input starts one float into its buffer, so the fp32 side takes its direct kernel too (the bf16 MFMA form sums in
    another order: the comparison is between the same kernel body on both sides, as everywhere in this file)."""
    img, x = _frame(TILED)
    fbig = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    xv = fbig[1:1 + x.size].view(*x.shape)
    xv.copy_(torch.from_numpy(x))
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    big = torch.zeros(img.size + 64, dtype=torch.uint8, device="cuda")
    view = big[1:1 + img.size].view(*img.shape)
    view.copy_(torch.from_numpy(img))
    assert view.data_ptr() % 4 == 1 and view.is_contiguous()
    got, want = _pair(TILED, 32, dtype, img_dev=view, x_dev=xv)
    _assert_same(got, want, "unaligned base")
    if dtype == torch.float32:                # fp32 output: the tiled vector-ALU kernel sums in the direct kernel's order
        _assert_same(got, _pair(TILED, 32, dtype)[0], "unaligned base against the aligned frame")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_smallest_shape(dtype):
    _assert_same(*_pair((1, 2, 4), 8, dtype), "2x4")


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_output_slice_keeps_its_neighbours(dtype, relu, affine):
    """y_cs = 48 with Cout = 32: channels 32..47 of the sentinel-filled buffer stay as they were (asserted inside _pair)"""
    got, want = _pair(TILED, 32, dtype, relu=bool(relu), affine=affine, cs=48)
    _assert_same(got, want, "y_cs=48 relu=%d affine=%d" % (relu, affine))


def test_window_builder_normalises_the_same_way():
    """fs_eval_window_input on an identity window (rows = H, cols = W, no pad, taps of scale 1) writes the expected input bit for bit:
    the two device-side normalisations agree with each other and with numpy."""
    from fasterseg_amd import eval_plan as EP, kernels as K
    img, x = _frame(TILED)
    _, h, w = TILED
    frame0 = torch.from_numpy(img[0]).cuda()
    ytab, xtab = (torch.from_numpy(EP.pack_taps(*EP.linear_taps(n, n, 1.0))).cuda() for n in (h, w))
    d = K.eval_window_desc(h, w, h, w, 0, 0, 0, 0, h, w, EP.PAD_NORMALISED, False, U.MEAN, U.STD)
    out = torch.full((1, 3, h, w), float("nan"), dtype=torch.float32, device="cuda")
    K.eval_window_input(d, frame0, ytab, xtab, out)
    torch.cuda.synchronize()
    want = torch.from_numpy(x[:1]).cuda()
    assert torch.equal(_bits(out), _bits(want)), "%d values differ" % int((_bits(out) != _bits(want)).sum())
