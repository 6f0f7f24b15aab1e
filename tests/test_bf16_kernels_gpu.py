"""FS_BF16 through the inference kernels on a real MI355X, held to the bars of tests/test_f16_kernels_gpu.py: the same entry points,
geometries, flags and debug hooks, with bfloat16 storage.  Helpers and bound formulas: tests/_bounds.py, unit roundoff E = 2^-8.

1. Conversion on a fixed table of normal fp32 values: fs_nchw_to_nhwc into bf16 gives the bits of torch's fp32 -> bf16 conversion (round to
   nearest even; ties both ways around 1 + k 2^-8; a value at or beyond the midpoint above the largest finite bf16 becomes infinity -
   bf16 does not saturate, unlike fp16; +-0 keep their sign; NaN stays NaN and nothing else becomes one); bf16 -> fp32 is exact.  fp32
   subnormals are left out: what the hardware converter does with them is not measured.
2. Exact contractions.  x in {j / 256, |j| <= 256} needs all 8 significand bits (asserted), w in {j / 8, |j| <= 8}; with
   K = 9 * Cin <= 576 every partial sum is a multiple of 2^-11 below 2^10 - 21 bits, exact in fp32 in any order - so the output must be
   round-to-nearest-even of the exact sum, bit for bit.  A kernel that truncated the store, lost an operand bit, dropped a tap or a
   channel, or rounded twice cannot give those bits.  Two-stage kernels (fs_conv3x3_pw_fwd, fs_zoom_cell_fwd) round the first stage to
   bf16 where the separate launches store it; their second filter is in {-1, 0, 1} and sparse so that the second contraction is exactly
   summable too (asserted on the CPU for the operands used: every sum of |terms| is a multiple of 2^-12 below 2^12).  The zoom cell is
   exact with its 1/2 down-sample from 4 x 4 (taps land on pixels: scale 3) and without the x2 up-sample, whose weights are not exact;
   the up-sample is covered by the random cells.
3. Random operands, rounded to bf16 first, against an fp64 reference on the rounded operands, over the case tables of the fp16 file.
   Single-stage kernels, per element:
       |got - ref| <= 2^-8 |ref| + K 2^-23 sum|x w| + 2^-24
   (one output rounding + the fp32 accumulation bound; K = taps x channels, 4 for a resample).  Kernels that round an intermediate map
   to bf16 (a resample folded into the conv staging, the 3x3 -> 1x1 pair, the zoom cell) get the same bound PROPAGATED stage by stage
   (tests/_bounds.py `_stage`, `_resample`).  The stems: the existing fp32 bound 1e-4 + 1e-4 |ref| plus 2^-8 |ref|.
4. fs_bilinear_argmax equals the arg-max of the fp64 up-sample wherever the top-two margin exceeds twice the resample bound, takes the
   lowest index on exact ties, and at most 1 % of the pixels are excluded by the margin rule (asserted before the launch).
5. fs_refresh_weights into bf16 writes the bytes of fs_pack_weight / fs_pack_weight_frag.
6. fs_eval_score_accumulate on bf16 logits against the fp64 up-sample (canvas and class map, with and without the flipped image).

Where this is looser than a literal reading of the single formula: the multi-stage kernels use the propagated bound above; the arg-max
margin is twice the resample bound (both candidates carry it); the zoom table is cut to maps of at most 8192 pixels and the stem table
to its first three images plus one odd-width image, so that the fp64 references stay within seconds."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _bounds as B
from tests import _grouped_cases as G
from tests import _resize_ref as R
from tests import _stem_cases as S
from tests import _u8_cases as U8
from tests import test_conv3x3_pw_gpu as PW
from tests import test_halo_ksplit_gpu as HK
from tests import test_logits_upsample_tiled_gpu as LT
from tests import test_zoom_cell_gpu as ZC

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_B = B.For(BF)
EBF, E32, TINY = B.UNIT[BF], B.E32, B.TINY
grid, bits, conv64, assert_within, _second_stage_exact = B.grid, B.bits, B.conv64, B.assert_within, B._second_stage_exact
rnd16, rne16, dev16, single_bound, _stage, _resample, _argmax_inputs = (_B.rnd16, _B.rne16, _B.dev16, _B.single_bound, _B._stage, _B._resample,
                                                                         _B._argmax_inputs)


def K():
    from fasterseg_amd import kernels
    return kernels


# ---- 1. conversion -------------------------------------------------------------------------------------------------------------------
BF_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127                 # 0x7f7f, the largest finite bf16
BF_MID = (2.0 - 2.0 ** -8) * 2.0 ** 127                 # half-way to 2^128: the tie goes to the even neighbour, infinity
F32_MAX = (2.0 - 2.0 ** -23) * 2.0 ** 127


def conversion_table():
    u = 2.0 ** -8                                         # half a bf16 ulp at 1
    base = [1.0 + u, 1.0 + 3 * u, 1.0 + 2 * u, 1.0 + u + 2.0 ** -23, BF_MAX, BF_MID - 2.0 ** 104, BF_MID, F32_MAX, 0.0, 0.333251953125,
            1000.5, 2.0 ** -100]
    table = np.array(base + [-v for v in base] + [float("nan"), float("inf"), -float("inf"), 0.1, -0.1, 3.39e38, 1.0 + 3 * u - 2.0 ** -23, 65520.0])
    table = table.astype(np.float32)
    assert table.size == 32 and (np.abs(table[np.isfinite(table) & (table != 0)]) >= 2.0 ** -126).all(), "no fp32 subnormals"
    return table


def test_conversion_table_round_trip():
    k = K()
    table = conversion_table()
    x = torch.from_numpy(table).view(1, 8, 2, 2).clone()                     # (N, C, H, W): every value is one (pixel, channel)
    want = bits(x.to(BF))                                                     # torch's conversion on the CPU: round to nearest even
    wf = x.to(BF).float().view(-1)
    assert float(wf[0]) == 1.0 and float(wf[1]) == 1.0 + 2.0 ** -6 and float(wf[3]) == 1.0 + 2.0 ** -7, "the ties go to even, both ways"
    assert float(wf[4]) == BF_MAX and float(wf[5]) == BF_MAX and float(wf[29]) == BF_MAX
    assert bool(torch.isinf(wf[[6, 7, 18, 19, 25, 26]]).all()), "bf16 does not saturate: the midpoint and beyond round to infinity"
    y = k.to_nhwc(x.cuda(), BF)
    got = bits(y)
    nan = torch.isnan(x)
    gotf = got.view(BF).float()
    assert torch.equal(torch.isnan(gotf), nan), "NaN must stay NaN and nothing else may become one"
    assert torch.equal(got[~nan], want[~nan]), (gotf[~nan], want.view(BF).float()[~nan])
    flat = got.view(-1).numpy().view(np.uint16)
    assert flat[8] == 0x0000 and flat[20] == 0x8000                           # +0, -0 keep their sign
    back = k.to_nchw(y).cpu()
    assert torch.equal(back[~nan], gotf[~nan]) and bool(torch.isnan(back[nan]).all()), "bf16 -> fp32 must be exact"


# ---- 2. exact contractions -------------------------------------------------------------------------------------------------------------
def _exact_ops(N, cin, H, W, cout, ksize, seed):
    x = grid(N, cin, H, W, seed=seed, den=256, lim=256)
    w = grid(cout, cin, ksize, ksize, seed=seed + 1, den=8, lim=8)
    assert ksize * ksize * cin <= 576
    xb = x.float().to(BF)
    assert bool((xb.double() == x).all()) and bool((w.float().to(BF).double() == w).all()), "the operands must be bf16 numbers"
    cleared = (xb.view(torch.int16) & ~1).view(BF)
    assert bool((cleared != xb).any()), "some x must need all 8 significand bits"
    return x, w


@pytest.mark.parametrize("case", [(1, 40, 5, 7, 24, 1, 1, 0), (1, 8, 9, 11, 16, 3, 2, 1)], ids=["1x1_40-24", "3x3s2_8-16"])
def test_exact_conv2d(case):
    k = K()
    N, cin, H, W, cout, ks, stride, pad = case
    x, w = _exact_ops(N, cin, H, W, cout, ks, seed=11)
    want = rne16(conv64(x, w, stride, pad))
    y = k.conv2d(dev16(x), k.pack_weight(w.float().cuda(), BF), cout, ks, ks, stride, pad)
    assert torch.equal(bits(y), bits(want)), float((y.double().cpu() - want.double()).abs().max())


@pytest.mark.parametrize("form", ["rule_5x7", "ksplit", "ksplit16", "no_ksplit", "unaligned_slice"])
def test_exact_conv3x3_s1(form):
    k = K()
    if form == "rule_5x7":
        N, cin, H, W, cout, ks_flag = 1, 32, 5, 7, 32, None                   # partial tiles, one chunk
    else:
        N, cin, H, W, cout = 1, 64, 16, 32, 48
        ks_flag = {"ksplit": True, "ksplit16": 16, "no_ksplit": False, "unaligned_slice": None}[form]
    x, w = _exact_ops(N, cin, H, W, cout, 3, seed=21)
    want = rne16(conv64(x, w, 1, 1))
    xd, wf = dev16(x), k.pack_weight_frag(w.float().cuda(), BF)
    if form == "unaligned_slice":
        wide = k.empty_nhwc(N, cout + 8, H, W, BF, "cuda", zero=True)
        out = wide[:, 4:4 + cout]
        assert out.data_ptr() % 16 == 8
        k.conv3x3_halo(xd, wf, cout, out=out)
        assert float(wide[:, :4].abs().max()) == 0.0 and float(wide[:, 4 + cout:].abs().max()) == 0.0
        y = out
    else:
        y = k.conv3x3_halo(xd, wf, cout, ksplit=ks_flag)
    assert torch.equal(bits(y), bits(want)), float((y.double().cpu() - want.double()).abs().max())


@pytest.mark.parametrize("rows", [4, 8], ids=["rows4", "rows8"])
def test_exact_conv3x3_pw(rows):
    """Cin 32, C3 64, Cout 19 in a 20-channel pixel stride: the 3x3 (ReLU) rounded to bf16 as the separate launch stores it, then the 1x1"""
    k = K()
    N, cin, H, W, c3, cout = 1, 32, 9, 33, 64, 19
    x, w3 = _exact_ops(N, cin, H, W, c3, 3, seed=31)
    w2 = grid(cout, c3, 1, 1, seed=33, den=1, lim=1, density=0.25)
    t = rne16(F.relu(conv64(x, w3, 1, 1))).double()
    _second_stage_exact(t, w2, 0)
    want = rne16(conv64(t, w2, 1, 0))
    buf = torch.full((N, H, W, 20), 7.0, dtype=BF, device="cuda")
    out = buf.permute(0, 3, 1, 2)[:, :cout]
    assert k.channel_stride(out) == 20
    k.conv3x3_pw(dev16(x), k.pack_weight_frag(w3.float().cuda(), BF), c3, None, None, True, k.pack_weight(w2.float().cuda(), BF), cout,
                 None, None, False, out=out, rows=rows)
    assert torch.equal(bits(out), bits(want)), float((out.double().cpu() - want.double()).abs().max())
    assert bool((buf[..., cout:] == 7.0).all()), "the pad channel of the 20-channel stride was written"


@pytest.mark.parametrize("down", [1, 0], ids=["down", "plain"])
def test_exact_zoom_cell(down):
    """the smallest geometry of tests/test_zoom_cell_gpu.py (8 -> 8 -> 8 on 4 x 4), up-sample off (module docstring)"""
    k = K()
    N, cin, C, H, W = ZC.CASES[-1][:5]
    assert (N, cin, C, H, W) == (1, 8, 8, 4, 4)
    x, w1 = _exact_ops(N, cin, H, W, C, 3, seed=41)
    w2 = grid(C, C, 3, 3, seed=43, den=1, lim=1, density=0.5)
    v = x[:, :, ::3, ::3] if down else x                                      # 4 -> 2 at align_corners=True: source rows / columns 0 and 3
    if down:
        assert np.array_equal(R.upsample(x.numpy(), (2, 2)), v.numpy())
    t = rne16(F.relu(conv64(v, w1, 1, 1))).double()
    _second_stage_exact(t, w2, 1)
    want = rne16(F.relu(conv64(t, w2, 1, 1)))
    y = k.zoom_cell(dev16(x), k.pack_weight_frag(w1.float().cuda(), BF), None, None, k.pack_weight_frag(w2.float().cuda(), BF), None, None,
                    C, C, down=bool(down), up=False)
    assert torch.equal(bits(y), bits(want)), float((y.double().cpu() - want.double()).abs().max())


# ---- 3. random operands against fp64 ---------------------------------------------------------------------------------------------------
CONV_GEOMS = [s["geom"] for s in G.CONV_TABLE if s.get("kind", "plain") in ("plain", "affine")]


@pytest.mark.parametrize("geom", CONV_GEOMS, ids=lambda g: "%dx%dx%dx%d-%d_k%ds%dp%d" % g)
@pytest.mark.parametrize("cfg", [-1, -2], ids=["heuristic", "igemm_only"])
def test_random_conv2d(geom, cfg):
    from fasterseg_amd import _lib
    k = K()
    N, cin, H, W, cout, ks, stride, pad = geom
    x = rnd16(N, cin, H, W, seed=100 + cin)
    w = rnd16(cout, cin, ks, ks, seed=101 + cin, scale=(2.0 / (cin * ks * ks)) ** 0.5)
    ref, mag = conv64(x, w, stride, pad), conv64(x.abs(), w.abs(), stride, pad)
    try:
        _lib.lib().fs_debug_force_conv_cfg(cfg)
        ohw = G.out_hw(H, W, ks, stride, pad)                                 # (pad -1: FactorizedReduce's x[:, :, 1:, 1:] branch)
        y = k.conv2d(dev16(x), k.pack_weight(w.float().cuda(), BF), cout, ks, ks, stride, pad, out_hw=ohw)
        yr = k.conv2d(dev16(x), k.pack_weight(w.float().cuda(), BF), cout, ks, ks, stride, pad, relu=True, out_hw=ohw)
    finally:
        _lib.lib().fs_debug_force_conv_cfg(-1)
    assert_within(y, ref, single_bound(ref, mag, ks * ks * cin), "fs_conv2d_fwd")
    assert_within(yr, F.relu(ref), single_bound(ref, mag, ks * ks * cin), "fs_conv2d_fwd + ReLU")


def test_random_factorized_reduce():
    """FactorizedReduce's two 1x1 / stride-2 branches (pad 0 and pad -1) as one grouped launch into the halves of one map"""
    from fasterseg_amd import _lib
    k = K()
    N, cin, H, W, half = 2, 96, 8, 12, 48
    x = rnd16(N, cin, H, W, seed=140)
    ws = [rnd16(half, cin, 1, 1, seed=141 + j, scale=(2.0 / cin) ** 0.5) for j in range(2)]
    xd = dev16(x)
    out = k.empty_nhwc(N, 2 * half, H // 2, W // 2, BF, "cuda", zero=True)
    wp = [k.pack_weight(w.float().cuda(), BF) for w in ws]
    ds = [k.conv_desc(x.shape, k.channel_stride(xd), half, 1, 1, 2, -j, 2 * half, BF, out_hw=(H // 2, W // 2)) for j in range(2)]
    _lib.call("fs_factorized_reduce_fwd", k._stream(), ctypes.byref(ds[0]), k._p(xd), k._p(wp[0]), k._p(out[:, :half]), None,
              ctypes.byref(ds[1]), k._p(xd), k._p(wp[1]), k._p(out[:, half:]), None)
    for j in range(2):
        ref, mag = conv64(x, ws[j], 2, -j), conv64(x.abs(), ws[j].abs(), 2, -j)
        assert_within(out[:, j * half:(j + 1) * half], ref, single_bound(ref, mag, cin), "fs_factorized_reduce_fwd branch %d" % j)


HALO_CASES = ([(1, c * 32, 16, 32, 64, f) for c in (1, 2, 3, 4, 6, 8) for f in HK.FORMS if c > 1 or f is True] +      # test_ksplit_chunk_counts
              [(2, 5 * 32 + 8, 7, 21, 64, f) for f in HK.FORMS] + [(2, 2 * 32 - 8, 5, 35, 32, f) for f in HK.FORMS] +  # channel tail, ragged, N = 2
              [(1, 128, 9, 18, co, True) for co in (19, 40, 96, 144)] +                                              # test_ksplit_cout_tails
              [(1, 64, 9, 18, 144, False), (1, 32, 24, 40, 64, None), (2, 40, 9, 33, 128, False)])                     # plain form: tiles 32 / 64 / 128


@pytest.mark.parametrize("case", HALO_CASES, ids=lambda c: "%dx%dx%dx%d-%d_%s" % c)
def test_random_conv3x3_s1(case):
    k = K()
    N, cin, H, W, cout, form = case
    x = rnd16(N, cin, H, W, seed=200 + cin)
    w = rnd16(cout, cin, 3, 3, seed=201 + cin, scale=(2.0 / (cin * 9)) ** 0.5)
    ref, mag = conv64(x, w, 1, 1), conv64(x.abs(), w.abs(), 1, 1)
    xd, wf = dev16(x), k.pack_weight_frag(w.float().cuda(), BF)
    y = k.conv3x3_halo(xd, wf, cout, ksplit=form)
    assert_within(y, ref, single_bound(ref, mag, 9 * cin), "fs_conv3x3_s1_fwd")
    if form is False:                                                          # the forced output-channel tiles of the plain form, and stride 2
        for tile in (32, 64, 128):
            assert_within(k.conv3x3_halo(xd, wf, cout, tile=tile), ref, single_bound(ref, mag, 9 * cin), "tile %d" % tile)
        ref2, mag2 = conv64(x, w, 2, 1), conv64(x.abs(), w.abs(), 2, 1)
        assert_within(k.conv3x3_halo(xd, wf, cout, stride=2), ref2, single_bound(ref2, mag2, 9 * cin), "stride 2")


@pytest.mark.parametrize("ksplit", [True, 16, False], ids=["ks32", "ks16", "plain"])
@pytest.mark.parametrize("case", HK.VRES_CASES, ids=["%dx%dc-%dx%d-to-%dx%d-%d" % c for c in HK.VRES_CASES])
def test_random_resample_at_staging(case, ksplit):
    """conv(relu(resample(x))) in one launch: the staged sample is rounded to bf16 (first stage of the chain), then the convolution"""
    k = K()
    N, chunks, Hs, Ws, H, W, cout = case
    cin = chunks * 32
    x = rnd16(N, cin, Hs, Ws, seed=300 + cin)
    w = rnd16(cout, cin, 3, 3, seed=301 + cin, scale=(2.0 / (cin * 9)) ** 0.5)
    v, e = _resample(x, None, (H, W), relu=True)
    ref, bound = _stage(v, e, w, None, None, True)
    xd, wf = dev16(x), k.pack_weight_frag(w.float().cuda(), BF)
    assert_within(k.conv3x3_halo(xd, wf, cout, relu=True, ksplit=ksplit, vres=(H, W, True)), ref, bound, "resample-at-staging")
    if ksplit is False:                                                        # the implicit-GEMM kernel's virtual resize (fs_conv2d_fwd vr_*)
        assert_within(k.conv2d(xd, k.pack_weight(w.float().cuda(), BF), cout, 3, 3, 1, 1, relu=True, vres=(H, W, True)), ref, bound,
                      "fs_conv2d_fwd virtual resize")


@pytest.mark.parametrize("rows", PW.ROWS, ids=["rows4", "rows8"])
@pytest.mark.parametrize("ch", PW.CHANNELS, ids=lambda c: "%d-%d-%d" % c)
def test_random_conv3x3_pw(ch, rows):
    k = K()
    cin, c3, cout = ch
    for (N, H, W) in (PW.GEOMS[2], PW.GEOMS[5]):                               # 3 x 17 (partial tiles) and 2 images of 9 x 33
        x = rnd16(N, cin, H, W, seed=400 + cin)
        w3 = rnd16(c3, cin, 3, 3, seed=401, scale=(2.0 / (9 * cin)) ** 0.5)
        w2 = rnd16(cout, c3, 1, 1, seed=402, scale=(2.0 / c3) ** 0.5)
        g = torch.Generator().manual_seed(403)
        s3, b3 = (torch.rand(c3, generator=g) + 0.5).double(), (torch.randn(c3, generator=g) * 0.5).double()
        s2, b2 = (torch.rand(cout, generator=g) + 0.5).double(), (torch.randn(cout, generator=g) * 0.5).double()
        t, e = _stage(x, None, w3, s3, b3, True)
        ref, bound = _stage(t, e, w2, s2, b2, False, pad=0)
        out = k.empty_nhwc(N, cout, H, W, BF, "cuda", cs=k.round_up(cout, 32 if cout % 8 else 8))
        k.conv3x3_pw(dev16(x), k.pack_weight_frag(w3.float().cuda(), BF), c3, s3.float().cuda(), b3.float().cuda(), True,
                     k.pack_weight(w2.float().cuda(), BF), cout, s2.float().cuda(), b2.float().cuda(), False, out=out, rows=rows)
        assert_within(out, ref, bound, "fs_conv3x3_pw_fwd %s on %dx%dx%d" % (ch, N, H, W))


ZOOM_CASES = [c for c in ZC.CASES if c[0] * c[3] * c[4] <= 8192]              # the large maps only repeat tiles: fp64 references stay quick


@pytest.mark.parametrize("case", ZOOM_CASES, ids=[("%dx%d-%d-%dx%d-d%du%d" % c) for c in ZOOM_CASES])
def test_random_zoom_cell(case):
    k = K()
    N, cin, C, H, W, down, up = case
    x = rnd16(N, cin, H, W, seed=500 + cin)
    w1 = rnd16(C, cin, 3, 3, seed=501, scale=(2.0 / (9 * cin)) ** 0.5)
    w2 = rnd16(C, C, 3, 3, seed=502, scale=(2.0 / (9 * C)) ** 0.5)
    s1, b1 = ZC.rnd(C, seed=4).abs().double() * 0.5 + 0.75, ZC.rnd(C, seed=5, scale=0.2).double()
    s2, b2 = ZC.rnd(C, seed=6).abs().double() * 0.5 + 0.75, ZC.rnd(C, seed=7, scale=0.2).double()
    v, e = _resample(x, None, (H // 2, W // 2)) if down else (x, None)
    v, e = _stage(v, e, w1, s1, b1, True)
    if up:
        v, e = _stage(v, e, w2, s2, b2, False, store=False)                    # R2 stays fp32 in LDS
        ref, bound = _resample(v, e, (H, W), relu=True)
    else:
        ref, bound = _stage(v, e, w2, s2, b2, True)
    sc = [t.float().cuda() for t in (s1, b1, s2, b2)]
    y = k.zoom_cell(dev16(x), k.pack_weight_frag(w1.float().cuda(), BF), sc[0], sc[1], k.pack_weight_frag(w2.float().cuda(), BF), sc[2], sc[3],
                    C, C, down=bool(down), up=bool(up))
    assert_within(y, ref, bound, "fs_zoom_cell_fwd")


STEM_CASES = [(c, im) for c in S.COUTS for im in S.IMAGES[:3]] + [(32, (2, 33, 50))]                 # (33, 50): W % 4 != 0, the direct kernel


@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: S.case_id(*c))
@pytest.mark.parametrize("mfma", [1, 0], ids=["mfma", "direct"])
def test_random_stem(case, mfma):
    from fasterseg_amd import _lib
    k = K()
    cout, image = case
    x, w, scale, shift = S.inputs(cout, image)
    ref = F.relu(F.conv2d(x.double(), w.double(), None, 2, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    try:
        _lib.lib().fs_debug_stem_mfma(mfma)
        y = k.conv_stem(x.cuda(), k.pack_weight(w.cuda(), torch.float32), cout, scale.cuda(), shift.cuda(), True, BF)
    finally:
        _lib.lib().fs_debug_stem_mfma(1)
    assert y.dtype == BF
    assert_within(y, ref, 1e-4 + 1e-4 * ref.abs() + EBF * ref.abs(), "fs_conv_stem_fwd")


@pytest.mark.parametrize("geom", [(2, 34, 52, 32), (1, 26, 264, 64), (1, 17, 136, 24), (1, 33, 50, 32)], ids=lambda g: "%dx%dx%d-c%d" % g)
def test_random_stem_u8(geom):
    k = K()
    n, h, w_, cout = geom
    img = U8.frame(n, h, w_, seed=7)
    x = torch.from_numpy(U8.expected(img))
    _, w, scale, shift = S.inputs(cout, (n, h, w_))
    ref = F.relu(F.conv2d(x.double(), w.double(), None, 2, 1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1))
    y = k.conv_stem_u8(torch.from_numpy(img).cuda(), k.pack_weight(w.cuda(), torch.float32), cout, scale.cuda(), shift.cuda(), True, BF,
                       U8.MEAN, U8.STD)
    assert_within(y, ref, 1e-4 + 1e-4 * ref.abs() + EBF * ref.abs(), "fs_conv_stem_u8_fwd")


@pytest.mark.parametrize("spec", G.RESIZE_TABLE, ids=lambda s: "%dx%dx%dx%d_to_%dx%d_r%d" % (s[0] + s[1] + (s[2],)))
def test_random_bilinear_nhwc(spec):
    k = K()
    (N, C, Hi, Wi), size, relu = spec
    x = rnd16(N, C, Hi, Wi, seed=600 + C)
    ref, bound = _resample(x, None, size, relu=bool(relu))
    wide = k.empty_nhwc(N, C + 16, Hi, Wi, BF, "cuda", zero=True)            # a channel slice of a wider buffer, as in the grouped table
    wide[:, 8:8 + C] = dev16(x)
    assert_within(k.bilinear(wide[:, 8:8 + C], size, relu=bool(relu)), ref, bound, "fs_bilinear_fwd NHWC")


@pytest.mark.parametrize("mode", [1, 2], ids=["f32out", "bf16out"])
@pytest.mark.parametrize("case", LT.CASES, ids=lambda c: "%dx%dx%d_%dx%d_to_%dx%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4][0], c[4][1]))
def test_random_logits_upsample_nchw(case, mode):
    """tiled form, gather kernel and scalar kernel of the NCHW logits writer (the case table says which shape takes which)"""
    from fasterseg_amd import _lib
    n, c, cs, (hi, wi), size, _ = case
    x, buf = LT._input(case, BF)
    ref, bound = _resample(torch.from_numpy(x).double(), None, size, store=(mode == 2), exact_taps=True)
    try:
        for tiled in (1, 0):
            _lib.lib().fs_debug_logits_tiled(tiled)
            out = LT._run(buf, case, mode)
            assert out.dtype == (torch.float32 if mode == 1 else BF)
            assert_within(out, ref, bound + (TINY * ref.abs() if mode == 1 else 0.0), "fs_bilinear_fwd NCHW (tiled hook %d)" % tiled)
    finally:
        _lib.lib().fs_debug_logits_tiled(1)


ARGMAX_SEED = 77
ARGMAX_CASES = [(2, 19, 32, (8, 16), (64, 128)),        # x8: the strip kernel
                (1, 19, 20, (9, 13), (70, 100)),        # generic kernel, tight channel stride
                (1, 5, 8, (5, 7), (33, 52))]            # last channel group holds one class


@pytest.mark.parametrize("case", ARGMAX_CASES, ids=lambda c: "%dx%dx%d_%dx%d_to_%dx%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4][0], c[4][1]))
def test_bilinear_argmax(case):
    from fasterseg_amd import _lib
    k = K()
    n, c, cs, (hi, wi), size = case
    buf, want, use, ties = _argmax_inputs(case, seed=ARGMAX_SEED)
    assert float(use.double().mean()) >= 0.99
    view = buf.cuda().permute(0, 3, 1, 2)[:, :c]
    classes = torch.full((n,) + tuple(size), 255, dtype=torch.uint8, device="cuda")
    d = _lib.ResizeDesc(n, hi, wi, size[0], size[1], c, cs, 0, k.dtype_code(BF), 0, 0)
    _lib.call("fs_bilinear_argmax", k._stream(), ctypes.byref(d), k._p(view), k._p(classes))
    got = classes.cpu().long()
    assert bool((got[use] == want[use]).all()), "%d of %d decided pixels differ" % (int((got[use] != want[use]).sum()), int(use.sum()))
    assert bool((got[ties] == 0).all()), "an exact tie between classes 0 and 1 must go to class 0"
    assert int(got.max()) < c


def test_affine_act_and_copy_channels():
    k = K()
    N, C, H, W = 2, 40, 7, 9
    x = rnd16(N, C, H, W, seed=700)
    g = torch.Generator().manual_seed(701)
    s, b = (torch.rand(C, generator=g) + 0.5).double(), torch.randn(C, generator=g).double()
    xd = dev16(x)
    ref = F.relu(x * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1))
    mag = (x * s.view(1, -1, 1, 1)).abs() + b.abs().view(1, -1, 1, 1)
    assert_within(k.affine_act(xd, s.float().cuda(), b.float().cuda(), True), ref, single_bound(ref, mag, 2), "fs_affine_act")
    wide = k.empty_nhwc(N, C + 16, H, W, BF, "cuda", zero=True)
    k.copy_channels(xd, wide[:, 8:8 + C])
    assert torch.equal(bits(wide[:, 8:8 + C]), bits(xd)) and float(wide[:, :8].abs().max()) == 0.0 and float(wide[:, 8 + C:].abs().max()) == 0.0


def test_eval_score_accumulate_against_fp64():
    """fs_eval_score_accumulate on bf16 logits: exp(l0 (+ l1 mirrored)) of the x8 up-sampled logits added into the fp32 canvas, and the
    class map of the same sum.  Reference: the fp64 up-sample of tests/_resize_ref.py.  The up-sample's absolute error e (four taps, per
    image) goes through exp as a relative error; exp itself and the canvas addition keep the bar of the existing fp32 / bf16 test
    (tests/test_ms_eval_gpu.py: rtol 1e-5, atol 1e-6): |got - ref| <= ref (2 e + 1e-5) + 1e-6."""
    k = K()
    N, C, h, w, cs = 2, 19, 8, 12, 20
    H, W = 8 * h, 8 * w
    g = torch.Generator().manual_seed(901)
    x = (torch.randn(N, C, h, w, generator=g) * 2.0).to(BF)
    buf = torch.randn(N, h, w, cs, generator=g).to(BF)                                  # the pad channel holds junk
    buf[..., :C] = x.permute(0, 2, 3, 1)
    logits = buf.cuda().permute(0, 3, 1, 2)[:, :C]
    up, err = _resample(x.double(), None, (H, W), store=False)
    y0, x0, rows, cols, cy, cx = 3, 5, H - 7, W - 9, 2, 4
    for flip in (0, 1):
        l = up[0] + (up[1].flip(-1) if flip else 0.0)                                   # (C, H, W)
        e = err[0] + (err[1].flip(-1) if flip else 0.0)
        canvas = torch.full((H, W, cs), 0.5, device="cuda")
        k.eval_score_accumulate(logits, (H, W), flip, (y0, x0, rows, cols), canvas=canvas, at=(cy, cx), store=False)
        got = canvas[cy:cy + rows, cx:cx + cols, :C].permute(2, 0, 1).double().cpu() - 0.5
        want = torch.exp(l)[:, y0:y0 + rows, x0:x0 + cols]
        bound = want * (2 * e[:, y0:y0 + rows, x0:x0 + cols] + 1e-5) + 1e-6
        assert_within(got, want, bound, "fs_eval_score_accumulate flip=%d" % flip)
        assert float((canvas[:cy] - 0.5).abs().max()) == 0.0 and float((canvas[:, :cx] - 0.5).abs().max()) == 0.0
        assert float((canvas[..., C:] - 0.5).abs().max()) == 0.0, "the pad channel changed"
        classes = torch.full((rows * cols,), 255, dtype=torch.uint8, device="cuda")
        k.eval_score_accumulate(logits, (H, W), flip, (y0, x0, rows, cols), classes=classes)
        lw, ew = l[:, y0:y0 + rows, x0:x0 + cols], e[:, y0:y0 + rows, x0:x0 + cols]
        top = lw.topk(2, dim=0).values
        clear = (top[0] - top[1]) > 2 * ew.max(0).values
        assert float(clear.double().mean()) >= 0.99
        assert bool((classes.view(rows, cols).cpu().long()[clear] == lw.argmax(0)[clear]).all())


# ---- 5. refresh ------------------------------------------------------------------------------------------------------------------------
def test_refresh_weights_writes_the_pack_bytes():
    from fasterseg_amd import _lib
    k = K()
    L, h = _lib, _lib.lib()
    g = torch.Generator().manual_seed(800)
    specs = [(L.FS_REFRESH_PACK, 40, 24, 3), (L.FS_REFRESH_PACK, 19, 128, 1), (L.FS_REFRESH_PACK_FRAG, 40, 24, 3), (L.FS_REFRESH_PACK_FRAG, 72, 200, 3)]
    ws = [(torch.randn(co, ci, ks, ks, generator=g) * 300.0).cuda() for _, co, ci, ks in specs]
    want = [k.pack_weight(w, BF) if kind == L.FS_REFRESH_PACK else k.pack_weight_frag(w, BF) for (kind, *_), w in zip(specs, ws)]
    got = [torch.full_like(t, 3.0) for t in want]
    entries = (L.RefreshEntry * len(specs))()
    chunks = []
    for i, ((kind, co, ci, ks), w) in enumerate(zip(specs, ws)):
        e = entries[i]
        e.kind, e.dtype, e.Cout, e.Cin, e.R, e.S = kind, L.FS_BF16, co, ci, ks, ks
        e.o_stride, e.i_stride = w.stride(0), w.stride(1)
        e.src, e.dst = w.data_ptr(), got[i].data_ptr()
        n = h.fs_refresh_entry_chunks_infer(ctypes.byref(e))
        assert n > 0
        chunks += [[i, c] for c in range(n)]
    table = torch.frombuffer(bytearray(bytes(entries)), dtype=torch.uint8).cuda()
    ch = torch.tensor(chunks, dtype=torch.int32).cuda()
    L.call("fs_refresh_weights", k._stream(), k._p(table), len(specs), k._p(ch), len(chunks))
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), specs[i]
