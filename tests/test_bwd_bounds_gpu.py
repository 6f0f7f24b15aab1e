"""The training backward kernels on a real MI355X against fp64 references, held to the per-element bounds of tests/_bounds.py (second
half; tests/test_bwd_bounds_selfcheck.py shows on the CPU that these bounds pass an honest kernel and fail a subtly wrong one): the
weight gradient (slab split, ragged last slab and chunk, narrow tiles, strided banks, fused pairs, the bit-reproducible mode), the
stride-2 data gradient by parity classes, the bilinear backward (NHWC gather, both NCHW forms) and the BatchNorm backward (register-
resident, column and grid-wide bodies).  fp32 and bf16, every element checked.

The launch geometry is the library's own: the tests restate its rules (B.wgrad_slabs / B.wgrad_ksplits for wgrad_prepare and the narrow
tiles, bn_body for bn_small_ok and BN_COL_MAX_PIXELS) and assert for each case the branch it is there for.  Operands sit in channel
slices of wider buffers with NaN in the foreign channels; outputs start as NaN (overwritten) or a random base (accumulated), and what
lies around them must keep its bits."""
import ctypes

import pytest
import torch

from tests import _bounds as B
from tests.test_kernels_gpu import RESIZE_CASES, S2_DGRAD_CASES

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
IDS = ["f32", "bf16"]
NAN = float("nan")
SENTINEL = 7.25                      # exact in bf16 and fp32


def K():
    from fasterseg_amd import kernels
    return kernels


def vec_of(dtype):
    return 4 if dtype == F32 else 8


def pixels(v):
    """(N, C, H, W) -> (N H W, C), the NHWC pixel order of the kernels"""
    return v.permute(0, 2, 3, 1).reshape(-1, v.shape[1])


def sliced(v, dtype, extra=0, c0=0, fill=NAN):
    """(pixels, C) fp64 values as the channel slice [c0, c0 + C) of a (pixels, C + extra) device buffer of `dtype` filled with `fill`"""
    P, C = v.shape
    v_ = vec_of(dtype)
    assert extra % v_ == 0 and c0 % v_ == 0 and c0 <= extra
    buf = torch.full((P, C + extra), fill, dtype=dtype, device="cuda")
    view = buf[:, c0:c0 + C]
    if v is not None:
        view.copy_(v.to(dtype))
    assert view.data_ptr() % 16 == 0
    return buf, view


def untouched(buf, c0, C, fill, what):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[..., c0:c0 + C] = False
    rest = buf[keep]
    same = torch.isnan(rest) if fill != fill else rest == fill
    assert bool(same.all()), "%s: %d elements around the slice were overwritten" % (what, int((~same).sum()))


def recorded(fn):
    from tests._grouped_cases import recorded as rec
    return rec(fn)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------------
# forward geometry (N, Cin, H, W, Cout, k, stride, pad); what the case is there for, asserted from the restated launch rules
WGRAD_CASES = [
    dict(geom=(1, 64, 20, 30, 64, 3, 1, 1), slabs=3, last=88, ksplits={1}),                       # three slabs, ragged last one, border taps
    dict(geom=(2, 96, 9, 13, 96, 3, 1, 1), slabs=1, ksplits={1, 2, 4}),                           # one slab, ragged chunk, every narrow tile pair
    dict(geom=(1, 48, 17, 25, 80, 3, 2, 1), slabs=1, ksplits={1, 2}, x_extra=16, dy_extra=16, pair=True),  # stride 2, odd map, 16-channel tail, two banks
    dict(geom=(2, 64, 9, 12, 32, 1, 2, -1), slabs=1, ksplits={2}, bank=True),                              # FactorizedReduce conv_2 ...
    dict(geom=(2, 64, 9, 12, 32, 1, 2, 0), slabs=1, ksplits={2}, bank=True, dy_extra=32),                  # ... and conv_1
    dict(geom=(3, 32, 7, 11, 40, 3, 1, 1), slabs=1, ksplits={2}, x_extra=32),                     # HoWo = 77: images end inside chunks
]


class WgradCase:
    """operands on the device, fp64 reference and magnitudes on the CPU; built once per (case, dtype) and left unchanged"""

    def __init__(self, spec, dtype):
        from fasterseg_amd._lib import ConvDesc
        k = K()
        self.spec, self.dtype = spec, dtype
        N, cin, H, W, cout, ks, stride, pad = spec["geom"]
        Ho, Wo = B.conv_out_hw(H, W, ks, stride, pad)
        self.M, self.cout, self.cin, self.ks = N * Ho * Wo, cout, cin, ks
        x = B.rnd16(dtype, N, cin, H, W, seed=710)
        dy = B.rnd16(dtype, N, cout, Ho, Wo, seed=711, scale=1e-3)              # loss-scale-sized: nothing may hide under an absolute floor
        ref, mag, self.P = B.wgrad_ref(x, dy, ks, stride, pad)
        self.ref, self.mag = ref.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()      # [O][R][S][I]
        self.P = self.P.permute(0, 2, 3, 1)
        xe, ye = spec.get("x_extra", 0), spec.get("dy_extra", 0)
        self.xbuf, self.x = sliced(pixels(x), dtype, xe, xe // 2 // vec_of(dtype) * vec_of(dtype))
        self.ybuf, self.dy = sliced(pixels(dy), dtype, ye, ye)
        self.desc = ConvDesc(N, H, W, cin, cout, ks, ks, stride, pad, Ho, Wo, cin + xe, cout + ye, k.dtype_code(dtype), 0)
        # the branch the case exists for
        assert B.wgrad_slabs(self.M, cout, cin, ks * ks, dtype)[0] == spec["slabs"], B.wgrad_slabs(self.M, cout, cin, ks * ks, dtype)
        if "last" in spec:
            S, slab = B.wgrad_slabs(self.M, cout, cin, ks * ks, dtype)
            assert self.M - (S - 1) * slab == spec["last"]
        else:
            assert self.M % B.WGRAD_KC[dtype] != 0, "the last chunk must be ragged"
        assert B.wgrad_ksplits(cout, cin) == spec["ksplits"]

    def run(self, deterministic):
        """one launch onto a random base -> (the whole gradient tensor on the CPU, base, mask and index of the block written, a function that
        lays a [O][R][S][I] tensor out like the block, slab count)"""
        from fasterseg_amd import _lib
        k = K()
        spec, cout, cin, ks = self.spec, self.cout, self.cin, self.ks
        taps = ks * ks
        st = k._stream()
        d = self.desc
        d.n_seg = d.g_jump = 0
        if spec.get("pair"):
            rows, O, I = cout // 2, cout // 2 + 8, cin + 16
            shape, block = (2, O, ks, ks, I), (slice(None), slice(0, rows), slice(None), slice(None), slice(0, cin))
            d.n_seg, d.g_jump = rows, O - rows
            strides, off = (taps * I, 1, I), 0
            place = lambda t: torch.stack([t[:rows], t[rows:]])
        elif spec.get("bank") or deterministic:
            O, T, I = cout + 8, taps + 2, cin + 16                                 # the block starts at row 4, tap slot 1, channel 8
            shape, block = (O, T, I), (slice(4, 4 + cout), slice(1, 1 + taps), slice(8, 8 + cin))
            strides, off = (T * I, 1, I), (4 * T + 1) * I + 8
            place = lambda t: t.reshape(cout, taps, cin)
        else:
            shape, block, strides, off = (cout, ks, ks, cin), (slice(None),) * 4, None, 0
            place = lambda t: t
        base = B.rnd16(F32, *shape, seed=712)
        dw = base.float().cuda()
        ptr = dw.data_ptr() + 4 * off
        if deterministic:
            ws = torch.empty(k.WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
            ws[:-k.WS_COUNTER_BYTES].fill_(0x7f)                                    # garbage scratch, zero counters
            ws[-k.WS_COUNTER_BYTES:].zero_()
            with k.deterministic():
                _lib.call("fs_conv2d_wgrad_ws", st, ctypes.byref(d), k._p(self.x), k._p(self.dy), ptr, *strides, k._p(ws), k.WORKSPACE_BYTES)
                torch.cuda.synchronize()
            assert int(ws[-k.WS_COUNTER_BYTES:].view(torch.int32).abs().sum()) == 0, "arrival counters were not left at zero"
            S = B.wgrad_slabs(self.M, cout, cin, taps, self.dtype, ws_bytes=k.WORKSPACE_BYTES)[0]
        else:
            if strides is None:
                _lib.call("fs_conv2d_wgrad", st, ctypes.byref(d), k._p(self.x), k._p(self.dy), ptr)
            else:
                _lib.call("fs_conv2d_wgrad_strided", st, ctypes.byref(d), k._p(self.x), k._p(self.dy), ptr, *strides)
            torch.cuda.synchronize()
            S = B.wgrad_slabs(self.M, cout, cin, taps, self.dtype)[0]
        got = dw.cpu()
        mask = torch.zeros(shape, dtype=torch.bool)
        mask[block] = True
        return got, base, mask, block, place, S

    def check(self, deterministic, what):
        got, base, mask, block, place, S = self.run(deterministic)
        assert torch.equal(got[~mask], base.float()[~mask]), what + ": rows, channels or taps outside the block changed"
        b = base[block]
        bound = B.wgrad_bound(place(self.mag), place(self.P.expand_as(self.mag)), S, b)
        B.assert_within(got[block], b + place(self.ref), bound, what)
        untouched(self.xbuf, self.x.storage_offset() % self.xbuf.shape[1], self.cin, NAN, what + " (x)")
        untouched(self.ybuf, self.dy.storage_offset() % self.ybuf.shape[1], self.cout, NAN, what + " (dy)")


_cases = {}


def wgrad_case(i, dtype):
    if (i, dtype) not in _cases:
        _cases[i, dtype] = WgradCase(WGRAD_CASES[i], dtype)
    return _cases[i, dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("i", range(len(WGRAD_CASES)), ids=[str(c["geom"]) for c in WGRAD_CASES])
def test_wgrad_within_the_bound(i, dtype):
    """fs_conv2d_wgrad / fs_conv2d_wgrad_strided (fp32 atomics; narrow tiles split their pixels) and fs_conv2d_wgrad_ws in the
    bit-reproducible mode (ordered slab partials; no pixel split; into a strided bank), each against fp64: base + ref within
    (P + S + 1) 2^-23 sum|dy x| + S 2^-23 |base| + 2^-24 at every element.  fp32 with the fp32 MFMA and with the bf16 split form."""
    from fasterseg_amd import _lib
    lib = _lib.lib()
    case = wgrad_case(i, dtype)
    try:
        for split in ((0, 1) if dtype == F32 else (1,)):
            lib.fs_set_fp32_split(split)
            case.check(False, "wgrad %s %s split=%d atomics" % (case.spec["geom"], dtype, split))
            case.check(True, "wgrad %s %s split=%d ordered slabs" % (case.spec["geom"], dtype, split))
    finally:
        lib.fs_set_fp32_split(1)


# ---- stride-2 data gradient ------------------------------------------------------------------------------------------------------------
_dgrad = {}


def dgrad_case(case, dtype):
    if (case, dtype) not in _dgrad:
        N, cin, H, W, cout, ks, stride, pad = case
        Ho, Wo = B.conv_out_hw(H, W, ks, stride, pad)
        w = B.rnd16(dtype, cout, cin, ks, ks, seed=720, scale=0.2)
        dy = B.rnd16(dtype, N, cout, Ho, Wo, seed=721)
        ref, mag, Kc = B.dgrad_s2_ref((N, cin, H, W), w, dy, stride, pad)
        _dgrad[case, dtype] = (w, dy, ref, B.single_bound(dtype, ref, mag, Kc), Kc)
    return _dgrad[case, dtype]


@pytest.fixture
def force_cfg(request):
    from fasterseg_amd import _lib
    _lib.lib().fs_debug_force_conv_cfg(request.param)
    yield request.param
    _lib.lib().fs_debug_force_conv_cfg(-1)


@pytest.mark.parametrize("force_cfg", [-1, -2, 102, 105], indirect=True, ids=lambda c: "cfg%d" % c)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", S2_DGRAD_CASES[:6], ids=str)
def test_stride2_dgrad_within_the_bound(case, dtype, force_cfg):
    """FS_CONV_TRANSPOSED by parity classes (and the zero-insertion form, cfg -2): single_bound with K = the class's real taps x Cout;
    classes without any tap are exact zeros, and every pixel of the NaN-filled dx is written."""
    k = K()
    N, cin, H, W, cout, ks, stride, pad = case
    w, dy, ref, bound, Kc = dgrad_case(case, dtype)
    dyd = k.to_nhwc(dy.float().cuda(), dtype)
    wf = k.pack_weight(w.float().cuda(), dtype, flip=True)
    dx = k.empty_nhwc(N, cin, H, W, dtype, "cuda")
    dx.fill_(NAN)
    k.conv2d(dyd, wf, cin, ks, ks, 1, ks - 1 - pad, transposed=True, out_hw=(H, W), out=dx)
    got = dx.double().cpu()
    assert bool(torch.isfinite(got).all()), "some pixel of dx was not written"
    empty = (Kc == 0).expand_as(got)
    assert bool((got[empty] == 0).all()), "a class without any tap must be exact zeros"
    B.assert_within(got, ref, bound, "stride-2 dgrad %s %s cfg %d" % (case, dtype, force_cfg))


# ---- bilinear backward -----------------------------------------------------------------------------------------------------------------
RESIZE_ALL = RESIZE_CASES + [((1, 16, 3, 5), (7, 21))]                          # x2 (compacted), x8 (overflow), down, Ho = 1, same size, non-integer ratio
NCHW_CASES = [((2, 19, 5, 7), (40, 56)), ((2, 19, 5, 7), (33, 50))]


def resize_operands(shape, size, dtype, seed):
    N, C, Hi, Wi = shape
    dy = B.rnd16(dtype, N, C, size[0], size[1], seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    yo = B.rnd16(dtype, N, C, size[0], size[1], seed=seed + 2) * (torch.rand(N, C, size[0], size[1], generator=g) >= 0.25).double()
    return dy, yo


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case,extra", [(c, 0) for c in RESIZE_ALL] + [(RESIZE_ALL[0], 1), (RESIZE_ALL[-1], 1)],
                         ids=lambda v: "slices" if v == 1 else "dense" if v == 0 else str(v))
def test_bilinear_bwd_within_the_bound(case, extra, relu, dtype):
    """fs_bilinear_bwd, NHWC: the gather over cand_range with the 6-column compaction and its overflow path, against dx = sum_o w(o, i) g[o]
    with the fp32 tap weights of tests/_resize_ref.py.  y_out holds exact zeros at a quarter of the pixels (the mask is y_out > 0); dx starts
    as NaN, so inputs that receive exactly zero must be written.  `slices` (the x2 and the non-integer case): dy, y_out and dx in channel slices of wider buffers."""
    from fasterseg_amd import _lib
    from fasterseg_amd._lib import ResizeDesc
    k = K()
    shape, size = case
    N, C, Hi, Wi = shape
    v = vec_of(dtype)
    dy, yo = resize_operands(shape, size, dtype, 730)
    ref, bound = B.resample_bwd(dtype, dy, yo, (Hi, Wi), relu)
    e = 2 * v * extra
    dybuf, dyv = sliced(pixels(dy), dtype, e, v * extra)
    yobuf, yov = sliced(pixels(yo), dtype, e, e)                               # the entry point gives dy and y_out one channel stride
    dxbuf = torch.full((N * Hi * Wi, C + 3 * v * extra), SENTINEL, dtype=dtype, device="cuda")
    dxv = dxbuf[:, 2 * v * extra:2 * v * extra + C]
    dxv.fill_(NAN)
    d = ResizeDesc(N, Hi, Wi, size[0], size[1], C, dxbuf.shape[1], dybuf.shape[1], k.dtype_code(dtype), int(relu), 0)
    _lib.call("fs_bilinear_bwd", k._stream(), ctypes.byref(d), k._p(dyv), k._p(yov) if relu else None, k._p(dxv))
    got = dxv.double().cpu().view(N, Hi, Wi, C).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()), "some input pixel was not written"
    B.assert_within(got, ref, bound, "bilinear bwd %s -> %s relu=%d %s" % (shape, size, relu, dtype))
    untouched(dxbuf, 2 * v * extra, C, SENTINEL, "dx")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", ["gather", "separable"])
@pytest.mark.parametrize("case", NCHW_CASES, ids=str)
def test_bilinear_bwd_nchw_within_the_bound(case, form, dtype):
    """the logits gradient: dy contiguous NCHW fp32, dx NHWC with 19 of 32 channels; fs_bilinear_bwd with out_nchw = 1 (2-D gather) and
    the separable fs_bilinear_bwd_nchw (one more fp32 rounding, of the row pass's intermediate).  Channels 19..31 keep a sentinel."""
    from fasterseg_amd import _lib
    from fasterseg_amd._lib import ResizeDesc
    k = K()
    (N, C, Hi, Wi), (Ho, Wo) = case
    dy = B.rnd16(F32, N, C, Ho, Wo, seed=740)
    ref, bound = B.resample_bwd(dtype, dy, None, (Hi, Wi), False, extra=int(form == "separable"))
    dyd = dy.float().cuda().contiguous()
    dxbuf = torch.full((N * Hi * Wi, 32), SENTINEL, dtype=dtype, device="cuda")
    dxbuf[:, :C].fill_(NAN)
    d = ResizeDesc(N, Hi, Wi, Ho, Wo, C, 32, 0, k.dtype_code(dtype), 0, 1)
    if form == "separable":
        ws = torch.full((N, C, Ho, Wi), NAN, dtype=torch.float32, device="cuda")
        _lib.call("fs_bilinear_bwd_nchw", k._stream(), ctypes.byref(d), k._p(dyd), k._p(ws), k._p(dxbuf))
    else:
        _lib.call("fs_bilinear_bwd", k._stream(), ctypes.byref(d), k._p(dyd), None, k._p(dxbuf))
    got = dxbuf[:, :C].double().cpu().view(N, Hi, Wi, C).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()), "some input pixel was not written"
    B.assert_within(got, ref, bound, "logits gradient %s -> %s %s %s" % ((N, C, Hi, Wi), (Ho, Wo), form, dtype))
    untouched(dxbuf, 0, C, SENTINEL, "dx")


# ---- BatchNorm backward ----------------------------------------------------------------------------------------------------------------
BNS_MAX_PIXELS, BN_COL_MAX_PIXELS = 512, 512       # csrc/bn_bodies.h bn_small_ok (BNS_THREADS * BNS_UNROLL), csrc/units.hip


def bn_body(ppg, groups):
    """the body fs_bn_act_train_bwd takes (csrc/units.hip, csrc/bn_col.hip), by its kernels' names"""
    if ppg <= BN_COL_MAX_PIXELS:
        return ["bn_small_bwd_kernel"] if groups in (1, 2) and ppg <= BNS_MAX_PIXELS else ["bn_group_bwd_kernel"]
    return ["bn_bwd_apply_kernel", "chan_reduce_kernel"]


# (groups, pixels per group, workspace): register-resident with G = 1 / 2, three groups in the generic column, the grid-wide pair
BN_CASES = [(1, 96, False), (2, 96, False), (2, 250, False), (1, 512, False), (2, 512, False), (3, 85, False),
            (1, 513, False), (1, 513, True), (2, 640, False), (2, 640, True)]
BN_BODIES = {(1, 96): "small", (2, 96): "small", (2, 250): "small", (1, 512): "small", (2, 512): "small", (3, 85): "column", (1, 513): "grid",
             (2, 640): "grid"}


def bn_check(want, dzv, red, dgacc, dbacc, acc0, C, what):
    got = dzv.double().cpu().reshape(want["dz"].shape)
    assert bool(torch.isfinite(got).all()), what + ": dz holds unwritten elements"
    B.assert_within(got, want["dz"], want["dz_bound"], what + " dz")
    r = red.double().cpu()
    B.assert_within(r[:C], want["dbeta"], want["dbeta_bound"], what + " red: dbeta")
    B.assert_within(r[C:2 * C], want["dgamma"], want["dgamma_bound"], what + " red: dgamma")
    if dgacc is not None:
        B.assert_within(dgacc.double().cpu(), want["dgamma_acc"], want["dgamma_acc_bound"], what + " dgamma accumulated")
        B.assert_within(dbacc.double().cpu(), want["dbeta_acc"], want["dbeta_acc_bound"], what + " dbeta accumulated")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("case", BN_CASES, ids=lambda c: "%dx%d%s" % (c[0], c[1], "-ws" if c[2] else ""))
def test_bn_act_train_bwd_within_the_bound(case, relu, dtype):
    """fs_bn_act_train_bwd on its own inputs (the saved statistics are computed in fp64 and rounded once to fp32): dz, the `red` totals
    and the accumulated parameter gradients, C = 8 and 40, accumulators given and not.  With the workspace the grid-wide reduction runs
    inside k.deterministic(): ordered block partials instead of float atomics."""
    from fasterseg_amd import _lib
    k = K()
    G, n, use_ws = case
    body = bn_body(n, G)
    assert {"small": ["bn_small_bwd_kernel"], "column": ["bn_group_bwd_kernel"], "grid": ["bn_bwd_apply_kernel", "chan_reduce_kernel"]}[BN_BODIES[G, n]] == body
    v = vec_of(dtype)
    for C in (8, 40):
        for acc in (False, True):
            ops = B.bn_operands(dtype, G, n, C, relu, 750 + C)
            z, dy, yo, mean, invstd, gamma = ops
            g = torch.Generator().manual_seed(760)
            dg0, db0 = (torch.randn(C, generator=g).float().double(), torch.randn(C, generator=g).float().double()) if acc else (None, None)
            want = B.bn_bwd(dtype, *ops, relu, dg_acc=dg0, db_acc=db0)
            zbuf, zv = sliced(z.view(G * n, C), dtype, 2 * v, v)
            dybuf, dyv = sliced(dy.view(G * n, C), dtype, v, 0)
            yobuf, yov = sliced(yo.view(G * n, C), dtype, 3 * v, 2 * v)
            dzbuf = torch.full((G * n, C + v), SENTINEL, dtype=dtype, device="cuda")
            dzv = dzbuf[:, v:v + C]
            dzv.fill_(NAN)
            saved = torch.full((G, 4, C), NAN, dtype=torch.float32, device="cuda")          # [mean | invstd | scale | shift]: the backward reads two
            saved[:, 0], saved[:, 1] = mean.float().cuda(), invstd.float().cuda()
            gam = gamma.float().cuda()
            red = torch.zeros((G + 1 if G > 1 else 1) * 2 * C, dtype=torch.float32, device="cuda")
            dgacc, dbacc = (dg0.float().cuda(), db0.float().cuda()) if acc else (None, None)
            ws = k.stream_workspace("cuda") if use_ws else (None, 0)

            def launch():
                _lib.call("fs_bn_act_train_bwd", k._stream(), G * n, C, G, k._p(zv), zbuf.shape[1], k._p(dyv), dybuf.shape[1],
                          k._p(yov) if relu else None, yobuf.shape[1] if relu else 0, k._p(saved), k._p(gam), k._p(red), k.dtype_code(dtype),
                          int(relu), k._p(dzv), dzbuf.shape[1], k._p(dgacc), k._p(dbacc), *ws)
            if use_ws:
                with k.deterministic():
                    names = recorded(launch)
            else:
                names = recorded(launch)
            assert sorted(n_ for n_ in names if n_.startswith(("bn_", "chan_reduce"))) == body, names
            what = "BN bwd %d x %d C=%d relu=%d acc=%d ws=%d %s" % (G, n, C, relu, acc, use_ws, dtype)
            bn_check(want, dzv, red, dgacc, dbacc, acc, C, what)
            untouched(dzbuf, v, C, SENTINEL, what + " (dz)")
            for buf, c0 in ((zbuf, v), (dybuf, 0), (yobuf, 2 * v)):
                untouched(buf, c0, C, NAN, what + " (operands)")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
def test_bn_column_body_at_512_lanes(relu, dtype):
    """fs_bn_act_train_bwd hands the generic column body only maps of up to 512 pixels per group, 256 lanes; fs_bn_group_bwd itself takes
    any size and launches 512 lanes above 512 pixels per group: 3 x 600."""
    from fasterseg_amd import _lib
    k = K()
    G, n, C = 3, 600, 40
    ops = B.bn_operands(dtype, G, n, C, relu, 770)
    z, dy, yo, mean, invstd, gamma = ops
    want = B.bn_bwd(dtype, *ops, relu)
    zv, dyv, yov = (sliced(t.view(G * n, C), dtype)[1] for t in (z, dy, yo))
    dzv = torch.full((G * n, C), NAN, dtype=dtype, device="cuda")
    saved = torch.full((G, 4, C), NAN, dtype=torch.float32, device="cuda")
    saved[:, 0], saved[:, 1] = mean.float().cuda(), invstd.float().cuda()
    gam, red = gamma.float().cuda(), torch.zeros(2 * C, dtype=torch.float32, device="cuda")
    names = recorded(lambda: _lib.call("fs_bn_group_bwd", k._stream(), G * n, C, G, k._p(zv), C, k._p(dyv), C, k._p(yov) if relu else None,
                                       C if relu else 0, k._p(saved), k._p(gam), k.dtype_code(dtype), int(relu), k._p(dzv), C, k._p(red), None, None))
    assert [n_ for n_ in names if n_.startswith("bn_")] == ["bn_group_bwd_kernel"], names
    bn_check(want, dzv, red, None, None, False, C, "BN column body 3 x 600 relu=%d %s" % (relu, dtype))


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_backward_pair_on_a_small_map(dtype, relu):
    """k.bn_backward (fs_bn_bwd_reduce_ws + fs_bn_bwd_apply) on a 2 x 9 x 13 map: the bf16 path tests/test_kernels_gpu.py leaves out"""
    k = K()
    N, C, H, W = 2, 40, 9, 13
    ops = B.bn_operands(dtype, 1, N * H * W, C, relu, 780)
    z, dy, yo, mean, invstd, gamma = ops
    want = B.bn_bwd(dtype, *ops, relu)

    def nhwc(t):
        return k.to_nhwc(t.view(N, H, W, C).permute(0, 3, 1, 2).float().cuda(), dtype)
    dz, dg, db = k.bn_backward(nhwc(z), nhwc(dy), nhwc(yo), mean[0].float().cuda(), invstd[0].float().cuda(), gamma.float().cuda(), relu)
    got = dz.permute(0, 2, 3, 1).reshape(1, N * H * W, C)
    what = "k.bn_backward 2x9x13 relu=%d %s" % (relu, dtype)
    B.assert_within(got, want["dz"], want["dz_bound"], what + " dz")
    B.assert_within(db, want["dbeta"], want["dbeta_bound"], what + " dbeta")
    B.assert_within(dg, want["dgamma"], want["dgamma_bound"], what + " dgamma")
