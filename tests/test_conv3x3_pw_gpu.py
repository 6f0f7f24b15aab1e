"""fs_conv3x3_pw_fwd (conv3x3_pw.hip): a 3x3 / stride 1 / pad 1 LDS-halo conv and the 1x1 conv behind it in one launch.

Reference for "results stay what they were": the separate launches the engine issues without the fusion (fs_conv3x3_s1_fwd ->
fs_conv2d_fwd_ws on the same packed filters, scales and shifts).  Beside it an fp64 chain on the CPU that rounds to the storage type
where the separate launches store.

Exactly summable operands: inputs are integers in [-2, 2], filters are in {-1, 0, 1} (the 3x3 sparse), scales are in {0.5, 1, 2},
shifts are small integers.  Every product and every partial sum of both stages is then a multiple of 2^-3 whose magnitude, bounded by
the sum of the |terms|, stays below 2^21: exact in fp32 in ANY order of summation (test_exact_cases_are_exactly_summable checks that
on the CPU for every case used here).  The rounding to bf16 between the stages acts on identical fp32 values, so the fused launch
must give the bits of the separate launches - whole buffers are compared, pad channels and the neighbours of a slice included.

Random operands (bf16; the entry point refuses fp32 with FS_ERR_UNSUPPORTED and the engine keeps the separate launches there): error
of the fused launch and of the separate launches against the fp64 chain on the same inputs; fused max <= 2 x separate max, fused mean
<= 1.1 x separate mean.  Both paths carry one rounding per stage, a wrong tap / halo pixel / missing rounding shows as tens of times.
The separate 3x3 runs in its plain form there (FS_CONV_NO_KSPLIT), the form it takes on the >= 64 x 128 maps where the engine fuses; on
the test's 9 x 33 map the library's rule would pick the K-split form.  Measured on one MI355X: three of the four channel cases give the
bits of the separate launches (the 3x3 sums in the stand-alone kernel's order); in (128, 128, 19) one value of 11 286 differs, fused /
separate max 3.9e-3 / 3.9e-3 and mean 3.46e-7 / 3.57e-7 against the chain.

The form with a 1x1 in FRONT of the 3x3 is not built, so it has no cases here."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DT = torch.bfloat16

ROWS = [4, 8]
# N, H, W: a single pixel (a tile that is all border), partial tiles in both directions, exact tiles, two images
GEOMS = [(1, 1, 1), (1, 2, 16), (1, 3, 17), (1, 9, 33), (1, 16, 32), (2, 9, 33)]
# Cin (input of the 3x3: 72 ends inside a 32-channel chunk, 192 is six chunks), C3 (output of the 3x3), Cout (output of the 1x1)
CHANNELS = [(64, 128, 19), (72, 64, 64), (192, 128, 64), (128, 128, 19)]


def K():
    from fasterseg_amd import kernels
    return kernels


def make_case(seed, N, H, W, cin, c3, cout, exact):
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    c = dict(N=N, H=H, W=W, cin=cin, c3=c3, cout=cout)
    if exact:
        c["x"] = ri(-2, 2, N, cin, H, W)
        c["w3"] = ri(-1, 1, c3, cin, 3, 3) * (torch.rand((c3, cin, 3, 3), generator=g) < 0.25).float()
        c["w2"] = ri(-1, 1, cout, c3, 1, 1)
        for i, n in ((3, c3), (2, cout)):
            c["s%d" % i] = 2.0 ** ri(-1, 1, n)
            c["b%d" % i] = ri(-3, 3, n)
    else:
        c["x"] = torch.randn((N, cin, H, W), generator=g).to(DT).float()
        c["w3"] = (torch.randn((c3, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5).to(DT).float()
        c["w2"] = (torch.randn((cout, c3, 1, 1), generator=g) * (2.0 / c3) ** 0.5).to(DT).float()
        for i, n in ((3, c3), (2, cout)):
            c["s%d" % i] = torch.rand(n, generator=g) + 0.5
            c["b%d" % i] = torch.randn(n, generator=g) * 0.5
    return c


def stages(c):
    """[(filter, scale, shift, relu, pad)]: the 3x3 carries BN + ReLU, the 1x1 a bias only when it is the classifier (19 channels) and
    BN + ReLU otherwise (an arm)."""
    classifier = c["cout"] == 19
    return [(c["w3"], c["s3"], c["b3"], True, 1), (c["w2"], None if classifier else c["s2"], c["b2"], not classifier, 0)]


def chain64(c, magnitudes=False):
    """fp64 chain, rounded to bf16 where the separate launches store.  magnitudes=True: also the largest sum of |terms| of any stage
    (a bound on every partial sum in any order) and whether every stage's terms are multiples of 2^-3."""
    v = c["x"].double()
    worst, grid_ok = 0.0, True
    for w, s, b, relu, pad in stages(c):
        acc = F.conv2d(v, w.double(), None, 1, pad)
        if magnitudes:
            worst = max(worst, float(F.conv2d(v.abs(), w.double().abs(), None, 1, pad).max()))
            grid_ok = grid_ok and bool(((v * 8).round() == v * 8).all())
        o = acc * (s.double().view(1, -1, 1, 1) if s is not None else 1.0) + b.double().view(1, -1, 1, 1)
        if relu:
            o = F.relu(o)
        if magnitudes:
            worst = max(worst, float(o.abs().max()))
        v = o.to(torch.float32).to(DT).double()
    return (v, worst, grid_ok) if magnitudes else v


def device_ops(c):
    k = K()
    (w3, s3, b3, r3, _), (w2, s2, b2, r2, _) = stages(c)
    return dict(wf=k.pack_weight_frag(w3.cuda(), DT), s3=s3.cuda(), b3=b3.cuda(), r3=r3, w2=k.pack_weight(w2.cuda(), DT),
                s2=s2.cuda() if s2 is not None else None, b2=b2.cuda(), r2=r2)


def device_input(c, wide):
    """NHWC input; wide: a channel slice of a buffer with 16 more channels (x_cs > Cin)."""
    k = K()
    x = c["x"]
    xd = k.to_nhwc(x.cuda(), DT)
    if not wide:
        return xd
    buf = k.empty_nhwc(x.shape[0], x.shape[1] + 16, x.shape[2], x.shape[3], DT, "cuda", zero=True)
    buf[:, 8:8 + x.shape[1]] = xd
    buf[:, :8] = 5.0
    buf[:, 8 + x.shape[1]:] = -5.0
    return buf[:, 8:8 + x.shape[1]]


def out_buffer(c, lo, extra):
    """The output view and its whole buffer (filled with a sentinel): channels [lo, lo + Cout) of a pixel stride rounded up to 32 for the
    19-class logits (the engine's buffer) plus `extra`."""
    k = K()
    cout = c["cout"]
    cs = k.round_up(cout, 32 if cout % 8 else 8) + extra
    whole = k.empty_nhwc(c["N"], cs, c["H"], c["W"], DT, "cuda", cs=cs)
    whole.fill_(7.0)
    return whole[:, lo:lo + cout], whole


def run_separate(c, o, xd, out, ksplit=None):
    k = K()
    t = k.conv3x3_halo(xd, o["wf"], c["c3"], o["s3"], o["b3"], relu=o["r3"], ksplit=ksplit)
    return k.conv2d(t, o["w2"], c["cout"], 1, 1, 1, 0, o["s2"], o["b2"], relu=o["r2"], out=out)


def run_fused(c, o, xd, out, rows):
    return K().conv3x3_pw(xd, o["wf"], c["c3"], o["s3"], o["b3"], o["r3"], o["w2"], c["cout"], o["s2"], o["b2"], o["r2"], out=out, rows=rows)


def exact_cases():
    for gi, (N, H, W) in enumerate(GEOMS):
        for ci, ch in enumerate(CHANNELS):
            yield make_case(100 * gi + ci, N, H, W, *ch, exact=True)


def test_exact_cases_are_exactly_summable():
    """CPU: in every exact case every sum of |terms| (so every partial sum in any order) is a multiple of 2^-3 below 2^21, i.e. below
    2^24 units of the grid."""
    for c in list(exact_cases()) + [make_case(900 + ci, 2, 9, 33, *ch, exact=True) for ci, ch in enumerate(CHANNELS)]:
        _, worst, grid_ok = chain64(c, magnitudes=True)
        assert grid_ok and worst * 8 < 2 ** 24, (c["H"], c["W"], c["cin"], worst)


@gpu
@pytest.mark.parametrize("rows", ROWS, ids=["rows4", "rows8"])
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%dx%d" % g for g in GEOMS])
def test_fused_equals_separate_launches_bit_for_bit(geom, rows):
    gi = GEOMS.index(geom)
    for ci, ch in enumerate(CHANNELS):
        c = make_case(100 * gi + ci, *geom, *ch, exact=True)
        o = device_ops(c)
        xd = device_input(c, wide=(ci == 1))
        sep, sep_whole = out_buffer(c, 0, 0)
        fus, fus_whole = out_buffer(c, 0, 0)
        run_separate(c, o, xd, sep)
        run_fused(c, o, xd, fus, rows)
        assert torch.equal(sep_whole, fus_whole), (ch, float((sep_whole.float() - fus_whole.float()).abs().max()))
        want = chain64(c)
        assert torch.equal(fus.float().cpu().double(), want), (ch, "fp64 chain", float((fus.float().cpu().double() - want).abs().max()))
        again, again_whole = out_buffer(c, 0, 0)
        run_fused(c, o, xd, again, rows)
        assert torch.equal(again_whole, fus_whole), "two runs differ"


@gpu
@pytest.mark.parametrize("rows", ROWS, ids=["rows4", "rows8"])
@pytest.mark.parametrize("lo", [8, 4], ids=["aligned", "8_bytes_off"])
def test_output_into_channel_slice(lo, rows):
    """The output is channels [lo, lo + Cout) of a wider buffer: 16-byte stores when the slice is aligned, element stores 8 bytes off.  The
    neighbours of the slice and the pad channels hold what the separate launches leave there (the sentinel: nothing writes them)."""
    for ci, ch in enumerate(CHANNELS):
        c = make_case(900 + ci, 2, 9, 33, *ch, exact=True)
        o = device_ops(c)
        xd = device_input(c, wide=True)
        sep, sep_whole = out_buffer(c, lo, 16)
        fus, fus_whole = out_buffer(c, lo, 16)
        run_separate(c, o, xd, sep)
        run_fused(c, o, xd, fus, rows)
        assert torch.equal(sep_whole, fus_whole), ch
        cout = fus.shape[1]
        assert bool((fus_whole[:, :lo] == 7.0).all()) and bool((fus_whole[:, lo + cout:] == 7.0).all())


@gpu
@pytest.mark.parametrize("rows", ROWS, ids=["rows4", "rows8"])
def test_random_operands_error_against_fp64_chain(rows):
    ratios = []
    for ci, ch in enumerate(CHANNELS):
        c = make_case(500 + ci, 2, 9, 33, *ch, exact=False)
        o = device_ops(c)
        xd = device_input(c, wide=False)
        sep, _ = out_buffer(c, 0, 0)
        fus, _ = out_buffer(c, 0, 0)
        run_separate(c, o, xd, sep, ksplit=False)
        run_fused(c, o, xd, fus, rows)
        want = chain64(c)
        e_sep = (sep.float().cpu().double() - want).abs()
        e_fus = (fus.float().cpu().double() - want).abs()
        figures = (float(e_fus.max()), float(e_sep.max()), float(e_fus.mean()), float(e_sep.mean()))
        print("conv3x3_pw rows%d %s: fused max %.4e separate max %.4e fused mean %.4e separate mean %.4e; off the chain: fused %d separate %d "
              "of %d, fused != separate %d" % ((rows, ch) + figures + (int((e_fus > 0).sum()), int((e_sep > 0).sum()), e_fus.numel(),
                                                                       int((fus != sep).sum()))))
        ratios.append((ch, figures))
    for ch, (fmax, smax, fmean, smean) in ratios:
        assert fmax <= 2.0 * smax and fmean <= 1.1 * smean, (ch, fmax, smax, fmean, smean)


@gpu
def test_refused_descriptors_launch_nothing():
    from fasterseg_amd import _lib
    k = K()
    c = make_case(3, 1, 9, 33, 64, 128, 19, exact=True)
    o = device_ops(c)
    xd = device_input(c, wide=False)
    out, whole = out_buffer(c, 0, 0)
    handle = _lib.lib()

    def launch(d):
        return handle.fs_conv3x3_pw_fwd(k._stream(), ctypes.byref(d), k._p(xd), k._p(o["wf"]), k._p(o["s3"]), k._p(o["b3"]), k._p(o["w2"]), None,
                                        k._p(o["b2"]), k._p(out))

    def desc(**kw):
        d = k.conv_pw_desc(xd.shape, k.channel_stride(xd), 128, 19, k.channel_stride(out), DT, True, False)
        for n, v in kw.items():
            setattr(d, n, v)
        return d
    bad = [(desc(dtype=0), 2, "bf16 only"), (desc(C3=160), 2, "C3"), (desc(C3=100), 2, "C3"), (desc(Cout=160, y_cs=160), 2, "Cout"),
           (desc(flags=_lib.FS_PW_ROWS4 | _lib.FS_PW_ROWS8), 1, "exclude"), (desc(flags=0x1003), 1, "unknown flags"),
           (desc(x_cs=16), 1, "strides"), (desc(y_cs=8), 1, "strides"), (desc(Cin=12, x_cs=16), 1, "strides"), (desc(H=0), 1, "geometry"),
           (desc(dtype=7), 1, "dtype")]
    for d, status, word in bad:
        assert launch(d) == status, (word, handle.fs_last_error())
        assert word.encode() in handle.fs_last_error(), (word, handle.fs_last_error())
        assert handle.fs_conv3x3_pw_plan(ctypes.byref(d), None, None, None) == status
    assert handle.fs_conv3x3_pw_fwd(k._stream(), None, *([None] * 8)) == 1
    d = desc()
    assert handle.fs_conv3x3_pw_fwd(k._stream(), ctypes.byref(d), None, *([None] * 7)) == 1      # null operands
    torch.cuda.synchronize()
    assert bool((whole == 7.0).all()), "a refused descriptor wrote to the output"
    assert launch(desc()) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).all())


def test_plan_is_host_only():
    """Rows per block, workgroups and LDS bytes without a device: forced forms, the rule, and the LDS budget of two blocks per CU."""
    k = K()
    assert k.conv3x3_pw_plan(k.conv_pw_desc((1, 128, 128, 256), 128, 128, 19, 32, DT))[:2] == (8, 256)     # one 8-row block per CU
    assert k.conv3x3_pw_plan(k.conv_pw_desc((1, 128, 128, 256), 128, 128, 19, 32, DT, rows=4))[:2] == (4, 512)
    assert k.conv3x3_pw_plan(k.conv_pw_desc((1, 192, 64, 128), 192, 128, 64, 64, DT))[:2] == (4, 128)       # 64 blocks of 8 rows: 4 rows
    for rows in (4, 8):
        lds = k.conv3x3_pw_plan(k.conv_pw_desc((1, 128, 16, 32), 128, 128, 64, 64, DT, rows=rows))[2]
        assert 2 * lds <= 160 * 1024, (rows, lds)
