"""The per-element bounds of the training backward kernels (tests/_bounds.py, second half), checked on the CPU: they pass an honest
kernel and fail a subtly wrong one.  Companion of tests/test_bounds_selfcheck.py, for fp32 and bf16.

Every "kernel" is a small fp32 emulation that sums in an order that is not the fp64 reference's:
  * weight gradient: im2col by explicit index arithmetic (the kernel's pixel -> (n, oh, ow) decode and tap masks), 16 pixels at a time,
    the slabs of wgrad_prepare's rule added one after the other onto a random `base`;
  * stride-2 data gradient: one transposed convolution per filter tap, the taps added in fp32, one store;
  * bilinear backward: the gather in fp32 with the fp32 tap weights of tests/_resize_ref.py, wh * ww rounded, one store;
  * BatchNorm backward: A0, A1 as partial sums per 64 pixels, the dz expression in fp32, one store.
The honest emulation must lie within the bound at EVERY element.  Planted defects, each of which must put at least one element above it:
   1. wgrad: the last pixel of one slab is missing;
   2. wgrad: the pixels of the ragged last chunk beyond a multiple of 16 are missing;
   3. wgrad: a border tap with iw = -1 reads the last pixel of the previous row instead of zero;
   4. wgrad: the image index is taken one pixel late at an image boundary (HoWo = 77, no multiple of 16);
   5. wgrad: one slab's partial is added twice;
   6. dgrad: one tap of one parity class is missing;
   7. bilinear backward: the candidate range is one output short at the high end (`<` for `<=`: the widening by one hides it wherever
      the range is not clamped to the map; the last input column loses its last output);
   8. bilinear backward: the ReLU mask uses >= where the kernel uses > (y_out holds exact zeros);
   9. BN backward: A0 / (n - 1) instead of A0 / n;
  10. BN backward: the mask is ignored at one pixel;
  11. BN backward: group 1 uses group 0's saved statistics.
Each test prints how many elements the older bars flag - 2e-2 max|ref|, 2e-4 max|ref| + 1e-4, 1e-4 + 1e-4 |ref| - next to the count
above the bound (pytest -s); DESIGN.md records them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _bounds as B

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def store(v32, dtype):
    return v32.to(dtype).double()


def flagged(got, ref, bound, what, base=None):
    """elements above the per-element bound; prints the older bars' counts beside it (the older tests take the bars of an accumulated
    result from what was added, ref - base)"""
    err = (got - ref).abs()
    new = int((err > bound).sum())
    print("%-58s worst err / bound %10.3f   above the bound %6d   old bars (2e-2 max, 2e-4 max + 1e-4, 1e-4 + 1e-4|ref|) %s   of %d"
          % (what, float((err / bound).max()), new, B.old_bars(err, ref if base is None else ref - base), err.numel()))
    return new


_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


# ---- 1. weight gradient ----------------------------------------------------------------------------------------------------------------
WGRAD_CASES = {"slabs": (1, 16, 20, 30, 16, 3, 1, 1),         # M = 600: three slabs of 256, the last one 88 pixels = 5 * 16 + 8
               "images": (3, 8, 7, 11, 8, 3, 1, 1)}           # HoWo = 77: image boundaries inside 16-pixel chunks
WGRAD_DEFECTS = [("last_pixel_of_a_slab", "slabs"), ("ragged_chunk_tail", "slabs"), ("border_tap_wraps", "slabs"), ("image_index_late", "images"),
                 ("slab_added_twice", "slabs")]


def wgrad_case(name, dtype):
    def build():
        N, cin, H, W, cout, k, stride, pad = WGRAD_CASES[name]
        Ho, Wo = B.conv_out_hw(H, W, k, stride, pad)
        x = B.rnd16(dtype, N, cin, H, W, seed=610)
        dy = B.rnd16(dtype, N, cout, Ho, Wo, seed=611, scale=1e-3)                # loss-scale-sized gradients
        base = B.rnd16(torch.float32, cout, cin, k, k, seed=612)
        ref, mag, P = B.wgrad_ref(x, dy, k, stride, pad)
        S, slab = B.wgrad_slabs(N * Ho * Wo, cout, cin, k * k, dtype)
        return x, dy, base, base + ref, B.wgrad_bound(mag, P, S, base), (S, slab)
    return cached(("wgrad", name, dtype), build)


def emu_wgrad(x64, dy64, base64, geom, slabs, defect=None):
    """fp32: [pixel][tap][channel] operand rows gathered as the kernel decodes them, 16 pixels per step, slab after slab onto base"""
    N, cin, H, W, cout, k, stride, pad = geom
    S, slab = slabs
    Ho, Wo = B.conv_out_hw(H, W, k, stride, pad)
    M, howo = N * Ho * Wo, Ho * Wo
    m = torch.arange(M)
    n, rem = m // howo, m % howo
    if defect == "image_index_late":                                           # the first pixel of every later image still counts to the one before
        n = torch.where((rem == 0) & (n > 0), n - 1, n)
    oh, ow = rem // Wo, rem % Wo
    xp = x64.float().permute(0, 2, 3, 1).reshape(N * H * W, cin)               # NHWC pixels
    rows = []
    for r in range(k):
        for s in range(k):
            ih, iw = oh * stride - pad + r, ow * stride - pad + s
            ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
            pix = (n * H + ih) * W + iw
            if defect == "border_tap_wraps":                                   # iw = -1 is not masked: the address is the previous row's last pixel
                ok = ok | ((iw == -1) & (ih >= 0) & (ih < H) & (pix >= 0))
            rows.append(xp[pix.clamp(0, N * H * W - 1)] * ok[:, None].float())
    Bm = torch.stack(rows, 1).reshape(M, k * k * cin)                          # [pixel][tap][ci]
    A = dy64.float().permute(0, 2, 3, 1).reshape(M, cout)
    out = base64.float().permute(0, 2, 3, 1).reshape(cout, k * k * cin).clone()
    for sl in range(S):
        m0, m1 = sl * slab, min((sl + 1) * slab, M)
        if defect == "last_pixel_of_a_slab" and sl == 0:
            m1 -= 1
        if defect == "ragged_chunk_tail" and sl == S - 1:
            assert (m1 - m0) % 16 != 0
            m1 = m0 + (m1 - m0) // 16 * 16
        part = torch.zeros(cout, k * k * cin)
        for c0 in range(m0, m1, 16):
            part = part + A[c0:min(c0 + 16, m1)].t() @ Bm[c0:min(c0 + 16, m1)]
        out = out + part
        if defect == "slab_added_twice" and sl == 1:
            out = out + part
    return out.view(cout, k, k, cin).permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("name", list(WGRAD_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_honest_wgrad_is_within_the_bound(dtype, name):
    x, dy, base, ref, bound, slabs = wgrad_case(name, dtype)
    if name == "slabs":
        assert slabs == (3, 256)
    got = emu_wgrad(x, dy, base, WGRAD_CASES[name], slabs)
    B.assert_within(got, ref, bound, "honest wgrad %s, %s" % (name, dtype))
    assert flagged(got, ref, bound, "honest wgrad %s %s" % (name, dtype), base) == 0


@pytest.mark.parametrize("defect,name", WGRAD_DEFECTS, ids=[d for d, _ in WGRAD_DEFECTS])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_wgrad_defect_is_above_the_bound(dtype, defect, name):
    x, dy, base, ref, bound, slabs = wgrad_case(name, dtype)
    got = emu_wgrad(x, dy, base, WGRAD_CASES[name], slabs, defect=defect)
    assert flagged(got, ref, bound, "wgrad %s %s" % (defect, dtype), base) >= 1


def test_wgrad_bound_refuses_contractions_it_cannot_resolve():
    with pytest.raises(AssertionError):
        B.wgrad_bound(torch.ones(1, 1, 1, 1), torch.full((1, 1, 1, 1), 2049.0), 1)


# ---- 2. stride-2 data gradient ---------------------------------------------------------------------------------------------------------
DGRAD_GEOM = (1, 24, 9, 13, 16, 3, 2, 1)                                       # odd map: four parity classes of different sizes


def dgrad_case(dtype):
    def build():
        N, cin, H, W, cout, k, stride, pad = DGRAD_GEOM
        Ho, Wo = B.conv_out_hw(H, W, k, stride, pad)
        w = B.rnd16(dtype, cout, cin, k, k, seed=620, scale=0.2)
        dy = B.rnd16(dtype, N, cout, Ho, Wo, seed=621)
        ref, mag, K = B.dgrad_s2_ref((N, cin, H, W), w, dy, stride, pad)
        assert sorted(set(K.flatten().tolist())) == [cout, 2 * cout, 4 * cout]
        return w, dy, ref, B.single_bound(dtype, ref, mag, K)
    return cached(("dgrad", dtype), build)


def emu_dgrad(w64, dy64, dtype, drop=None):
    N, cin, H, W, cout, k, stride, pad = DGRAD_GEOM
    acc = torch.zeros(N, cin, H, W)
    for r in reversed(range(k)):
        for s in reversed(range(k)):
            w1 = torch.zeros_like(w64).float()
            w1[:, :, r, s] = w64[:, :, r, s].float()
            x0 = torch.zeros(N, cin, H, W, requires_grad=True)
            F.conv2d(x0, w1, None, stride, pad).backward(dy64.float())
            t = x0.grad
            if drop == (r, s):                                                 # the tap is missing for the pixels of one parity class
                t[:, :, 1::2, 1::2] = 0.0
            acc = acc + t
    return store(acc, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dgrad_honest_and_dropped_tap(dtype):
    w, dy, ref, bound = dgrad_case(dtype)
    got = emu_dgrad(w, dy, dtype)
    B.assert_within(got, ref, bound, "honest stride-2 dgrad, %s" % dtype)
    assert flagged(got, ref, bound, "honest stride-2 dgrad %s" % dtype) == 0
    assert flagged(emu_dgrad(w, dy, dtype, drop=(0, 0)), ref, bound, "dgrad: one tap of the odd-odd class missing, %s" % dtype) >= 1


# ---- 3. bilinear backward --------------------------------------------------------------------------------------------------------------
RESAMPLE_CASE = ((2, 8, 9, 12), (18, 24))


def resample_case(dtype, relu):
    def build():
        (N, C, Hi, Wi), (Ho, Wo) = RESAMPLE_CASE
        dy = B.rnd16(dtype, N, C, Ho, Wo, seed=630)
        yo = B.rnd16(dtype, N, C, Ho, Wo, seed=631)
        g = torch.Generator().manual_seed(632)
        yo = yo * (torch.rand(N, C, Ho, Wo, generator=g) >= 0.25).double()       # exact zeros at about a quarter of the pixels
        assert int((yo == 0).sum()) > 0
        ref, bound = B.resample_bwd(dtype, dy, yo, (Hi, Wi), relu)
        return dy, yo, ref, bound
    return cached(("resample", dtype, relu), build)


def emu_resample_bwd(dy64, yo64, dtype, relu, short_range=False, mask_ge=False):
    (N, C, Hi, Wi), (Ho, Wo) = RESAMPLE_CASE
    g = dy64.float()
    if relu:
        g = g * ((yo64 >= 0) if mask_ge else (yo64 > 0)).float()
    wh, ww = B.tap_matrix(Hi, Ho).float(), B.tap_matrix(Wi, Wo).float()
    if short_range:                                                            # `ow < whi` for `ow <= whi`: the widening hides it except where the
        _, hi = B.cand_range(Wi, Wo)                                           # range is clamped to the map - the last input column loses an output
        for i in range(Wi):
            ww[int(hi[i]), i] = 0.0
    w2 = (wh[:, None, :, None] * ww[None, :, None, :]).reshape(Ho * Wo, Hi * Wi)         # wh * ww rounded to fp32, as the kernel forms it
    return store((g.reshape(N * C, Ho * Wo) @ w2).view(N, C, Hi, Wi), dtype)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_resample_bwd_honest_and_defects(dtype, relu):
    dy, yo, ref, bound = resample_case(dtype, relu)
    got = emu_resample_bwd(dy, yo, dtype, relu)
    B.assert_within(got, ref, bound, "honest bilinear backward, %s relu=%d" % (dtype, relu))
    assert flagged(got, ref, bound, "honest bilinear backward %s relu=%d" % (dtype, relu)) == 0
    assert flagged(emu_resample_bwd(dy, yo, dtype, relu, short_range=True), ref, bound, "candidate range one short, %s relu=%d" % (dtype, relu)) >= 1
    if relu:
        assert flagged(emu_resample_bwd(dy, yo, dtype, relu, mask_ge=True), ref, bound, "ReLU mask >= instead of >, %s" % dtype) >= 1


def test_candidate_range_covers_every_contributing_output():
    """the restated cand_range (fp32, widened by one) contains every output with a non-zero reference weight, at the geometries of the
    GPU tests: what the kernel's gather rests on"""
    from tests.test_bwd_bounds_gpu import NCHW_CASES, RESIZE_ALL
    pairs = set()
    for (_, _, hi, wi), (ho, wo) in RESIZE_ALL + NCHW_CASES:
        pairs.update(((hi, ho), (wi, wo)))
    for i_, o_ in sorted(pairs):
        w, near = B.tap_matrix(i_, o_), B.near_matrix(i_, o_)
        assert bool(((w > 0).double() <= near).all()), (i_, o_)
        assert np.isclose(float(w.sum()), o_), (i_, o_)


# ---- 4. BatchNorm backward -------------------------------------------------------------------------------------------------------------
BN_CASE = (2, 96, 16)                                                           # groups, pixels per group, channels


def bn_case(dtype, relu):
    def build():
        G, n, C = BN_CASE
        ops = B.bn_operands(dtype, G, n, C, relu, 640)
        return ops, B.bn_bwd(dtype, *ops, relu)
    return cached(("bn", dtype, relu), build)


def emu_bn_bwd(ops, dtype, relu, defect=None):
    z, dy, yo, mean, invstd, gamma = (t.float() for t in ops)
    G, n, C = z.shape
    g = dy * (yo > 0).float() if relu else dy.clone()
    if defect == "mask_ignored_at_one_pixel":
        p = int(torch.nonzero((yo[1, :, 0] <= 0))[0]) if relu else 0
        g[1, p] = dy[1, p]
    if defect == "wrong_group_statistics":
        mean, invstd = mean[[0, 0]], invstd[[0, 0]]
    xh = (z - mean[:, None]) * invstd[:, None]
    a0, a1 = torch.zeros(G, 1, C), torch.zeros(G, 1, C)
    for p0 in range(0, n, 64):
        a0 = a0 + g[:, p0:p0 + 64].sum(1, keepdim=True)
        a1 = a1 + (g[:, p0:p0 + 64] * xh[:, p0:p0 + 64]).sum(1, keepdim=True)
    inv = torch.tensor(1.0 / n, dtype=torch.float32)
    t0 = a0 / (n - 1) if defect == "n_minus_one" else a0 * inv
    dz = gamma * invstd[:, None] * (g - t0 - xh * a1 * inv)
    return store(dz, dtype), a0.sum(0).view(C).double(), a1.sum(0).view(C).double()


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bn_bwd_honest_and_defects(dtype, relu):
    ops, want = bn_case(dtype, relu)
    dz, db, dg = emu_bn_bwd(ops, dtype, relu)
    B.assert_within(dz, want["dz"], want["dz_bound"], "honest BN backward dz, %s relu=%d" % (dtype, relu))
    B.assert_within(db, want["dbeta"], want["dbeta_bound"], "honest BN backward dbeta")
    B.assert_within(dg, want["dgamma"], want["dgamma_bound"], "honest BN backward dgamma")
    assert flagged(dz, want["dz"], want["dz_bound"], "honest BN backward %s relu=%d" % (dtype, relu)) == 0
    defects = ["n_minus_one", "wrong_group_statistics"] + (["mask_ignored_at_one_pixel"] if relu else [])
    for defect in defects:
        dz, _, _ = emu_bn_bwd(ops, dtype, relu, defect=defect)
        assert flagged(dz, want["dz"], want["dz_bound"], "BN %s, %s relu=%d" % (defect, dtype, relu)) >= 1, defect
