"""The loss heads through the C ABI against the fp64 reference of tests/_loss_ref.py, per pixel and per gradient element:
fs_ohem_ce_up_{fwd,bwd,bwd_coef} and fs_kl_distill_up_{fwd,bwd} (csrc/loss_up.hip) at the geometries where the cell partition
(first_dst), the per-cell sweep and the gather change path, fs_ohem_ce_{fwd,bwd,bwd_coef} and fs_kl_distill_{fwd,bwd} (csrc/loss.hip)
at odd full-resolution shapes, and the label rule of the criteria built on them (a label outside [0, C) counts as ignored).

Inputs: logits rounded to their storage dtype, at randn * 2, randn * 30 (probabilities underflow, nll in the hundreds) and
randn * 2 + 100 (exp without the max subtraction overflows); pad channels [C, cs) of every input map hold NaN; labels carry ~5 %
ignore and a handful of -1, C, 254 and 2**32 + 3; every output lives inside a sentinel-filled buffer; every backward runs once on a
NaN-filled and once on a zeroed workspace and must give the same bits.

Tolerance (fp32 outputs): with e32 the error of the torch fp32 CPU chain (interpolate, log_softmax, gather; autograd for gradients)
against fp64 on the same inputs, the kernel's maximum error is at most max(8 * e32, 16 * eps_fp32 * max|ref|) and every element is
inside 1e-4 + 1e-4 * |ref|.  bf16 gradients: 2^-8 * |ref| per element (half an ulp of 8 significant bits plus one bit for an fp32
error that crosses a rounding boundary) plus the fp32 bound.  Each check prints `ratio` = (kernel error) / e32 before it asserts.

Not covered: the grid-stride tails of the pixel loops - the launches cap at 65 536 blocks of 256 lanes, so reaching them needs more
than 16.7 M pixels.

Observed (kernel error) / e32 on an MI355X, worst case per family (fp32 outputs; n2 / n30 / p100 are the three distributions):
  ohem_up fwd 6.2 / 1.9 / 2.2    ohem_up bwd 3.1 / 1.2 / 2.4    kl_up fwd 1.8 / 2.6 / 2.9    kl_up bwd 1.5 / 1.6 / 1.5
  ohem (full) fwd 1.4 / 1.0 / 1.4    ohem (full) bwd 1.1 / 1.0 / 1.8    kl (full) fwd 1.4 / 1.0 / 1.5    kl (full) bwd 1.0 / 0.7 / 1.0
Every family is below the factor of 8.  Before the kernels were mended these tests measured: ohem (full) bwd 44 and kl (full) bwd 30
at n30 / p100 and true_prob 47 at p100 (exp(x - lse) with one fp32 lse rounded at |lse| ~ 100; the kernels now form
exp((x - max) - log(sum))), kl_up bwd 18 at n30 (make_tap's `scale * dst - i0` fused into an fma in one of forward / backward only:
loss_up.hip's up_tap keeps the operations apart), and a C = 1 gradient of 4.7e-8 instead of 0 (the blend contracted differently in
forward and backward: common.h's bilerp).
"""
import ctypes
import functools

import pytest
import torch

from tests import _loss_ref as R

pytestmark = pytest.mark.gpu

IGNORE = 255
EPS32 = float(torch.finfo(torch.float32).eps)
SENT = -123.0                 # exact in bf16 and fp32
GUARD = 64                    # elements before and after every output (keeps 16-byte alignment)
FS_ERR_INVALID = 1

# N, C, cs, (h, w), (H, W): the path each row exists for
ROWS = {
    1: (2, 19, 32, (8, 12), (64, 96)),      # x8, one wave per cell: the baseline
    2: (1, 19, 20, (5, 7), (37, 53)),       # ratio not an integer, one wave per cell
    3: (1, 19, 24, (3, 4), (40, 56)),       # ratio not an integer, cell area > 100: one block per cell
    4: (2, 20, 20, (1, 6), (17, 40)),       # h == 1 (rh == 0), C = LU_MAXC = cs
    5: (1, 5, 8, (6, 1), (11, 4)),          # w == 1, a partial last quad
    6: (2, 4, 4, (9, 7), (9, 7)),           # identity, smallest stride
    7: (1, 3, 64, (9, 10), (4, 5)),         # down-sample: cells with no pixel, largest stride
    8: (1, 1, 4, (4, 4), (12, 12)),         # C = 1: nll == 0, true_prob == 1, gradient 0
    9: (1, 19, 32, (2, 2), (1, 1)),         # H == W == 1 (both scales 0)
    10: (1, 17, 20, (4, 4), (64, 64)),      # x16, C = 17
}
DISTS = ("n2", "n30", "p100")
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
OHEM_CASES = [(r, dist) for r in ROWS for dist in (DISTS if r <= 3 else DISTS[:1])]


class Guarded:
    """`n` elements inside a sentinel-filled buffer."""

    def __init__(self, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def _draw(shape, dist, gen):
    v = torch.randn(shape, generator=gen)
    return {"n2": v * 2.0, "n30": v * 30.0, "p100": v * 2.0 + 100.0}[dist]


@functools.lru_cache(maxsize=None)
def _lowres(N, C, cs, hw, dtype, dist, seed):
    """Low-resolution logits: the (N, h, w, cs) device buffer (pad channels NaN) and the storage-rounded CPU value (N, C, h, w)."""
    val = _draw((N, C) + hw, dist, torch.Generator().manual_seed(seed)).to(dtype)
    buf = torch.full((N,) + hw + (cs,), float("nan"), dtype=dtype, device="cuda")
    buf[..., :C] = val.permute(0, 2, 3, 1).cuda()
    return buf, val


@functools.lru_cache(maxsize=None)
def _labels(N, H, W, C, seed, all_ignored=False):
    """~5 % ignore and up to three each of -1, C, 254 and 2**32 + 3 (never more than half of the pixels)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (N, H, W), generator=g)
    t[torch.rand(N, H, W, generator=g) < 0.05] = IGNORE
    if all_ignored:
        t[:] = IGNORE
    flat = t.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:min(12, flat.numel() // 2)]
    for k, p in enumerate(where.tolist()):
        flat[p] = (-1, C, 254, 2 ** 32 + 3)[k % 4]
    return t


def _desc(N, C, cs, hw, HW, dtype):
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    return _lib.LogitsDesc(N, hw[0], hw[1], C, cs, HW[0], HW[1], K.dtype_code(dtype))


def _ws_floats(d):
    from fasterseg_amd import _lib
    n = int(_lib.lib().fs_loss_up_workspace_bytes(ctypes.byref(d)))
    assert n == d.N * d.h * d.w * 80 * 4
    return n // 4


def _bound32(ref, ref32):
    e32 = float((ref32.double() - ref).abs().max())
    return max(8.0 * e32, 16.0 * EPS32 * float(ref.abs().max())), e32


def _check(got, ref, ref32, what, bf16_out=False):
    """got: the kernel's output; ref: fp64; ref32: the torch fp32 CPU chain.  Prints the error ratio, then asserts."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.double().reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound, e32 = _bound32(ref, ref32.reshape(-1))
    err = (got - ref).abs()
    worst = float(err.max()) if bool(torch.isfinite(err).all()) else float("nan")
    print("ratio %-40s err %.3e e32 %.3e ratio %.2f max|ref| %.3e" % (what, worst, e32, worst / e32 if e32 > 0 else (0.0 if worst == 0 else float("inf")),
                                                                     float(ref.abs().max())))
    if bf16_out:
        assert bool((err <= 2.0 ** -8 * ref.abs() + bound).all()), (what, worst, bound)
        return
    assert worst <= bound, (what, worst, bound, e32)
    assert bool((err <= 1e-4 + 1e-4 * ref.abs()).all()), (what, worst)


def _grad_out(d, dtype):
    g = Guarded(d.N * d.h * d.w * d.cs, dtype)
    return g, g.view.view(d.N, d.h, d.w, d.cs)


def _check_grad(gbuf, view, d, ref, ref32, what):
    assert gbuf.intact(), what + ": wrote outside the gradient"
    assert bool((view[..., d.C:] == 0).all()), what + ": pad channels of the gradient must be exactly 0"
    _check(view[..., :d.C].permute(0, 3, 1, 2), ref, ref32, what, bf16_out=view.dtype == torch.bfloat16)


def _twice(run, d, gbuf, what):
    """A backward on a NaN-filled and on a zeroed workspace: the same bits (fixed summation order, every slot read was written)."""
    ws = Guarded(_ws_floats(d))
    outs = []
    for fill in (float("nan"), 0.0):
        ws.view.fill_(fill)
        gbuf.view.fill_(SENT)
        run(ws)
        torch.cuda.synchronize()
        assert ws.intact(), what + ": wrote outside the workspace"
        outs.append(gbuf.view.clone())
    assert torch.equal(outs[0], outs[1]), what + ": the gradient depends on what the workspace held"


# ---- OHEM cross-entropy from low-resolution logits -------------------------------------------------------------------------------
def _ohem_up_case(row, dist, dtype, all_ignored=False):
    from fasterseg_amd import kernels as K
    N, C, cs, hw, HW = ROWS[row]
    P = N * HW[0] * HW[1]
    x_dev, x = _lowres(N, C, cs, hw, dtype, dist, 100 + row)
    target = _labels(N, HW[0], HW[1], C, 200 + row, all_ignored)
    tgt = target.cuda()
    d = _desc(N, C, cs, hw, HW, dtype)
    what = "ohem_up row%d %s %s" % (row, dist, "bf16" if dtype == torch.bfloat16 else "fp32")
    tp, nll, lse = Guarded(P), Guarded(P), Guarded(P)
    K.call("fs_ohem_ce_up_fwd", K._stream(), ctypes.byref(d), K._p(x_dev), K._p(tgt), IGNORE, K._p(tp.view), K._p(nll.view), K._p(lse.view))
    torch.cuda.synchronize()
    assert tp.intact() and nll.intact() and lse.intact(), what + ": wrote outside a per-pixel vector"
    ref = R.ohem_vectors(R.upsample(x, HW), target, IGNORE)
    ref32 = R.ohem_vectors(R.upsample(x, HW, torch.float32), target, IGNORE)
    for name, got, k in (("true_prob", tp, 0), ("nll", nll, 1), ("lse", lse, 2)):
        _check(got.view, ref[k], ref32[k], "%s fwd %s" % (what, name))
    dead = ~ref[3].cuda()
    assert bool((tp.view[dead] == 1).all()) and bool((nll.view[dead] == 0).all()), what + ": a label outside [0, C) or ignore must give true_prob 1, nll 0"

    g = torch.Generator().manual_seed(300 + row)
    keep = torch.rand(P, generator=g) < 0.6
    if all_ignored:
        keep[:] = True
    kept = keep.to(torch.uint8)
    odd = keep & (torch.rand(P, generator=g) < 0.3)
    kept[odd] = torch.randint(2, 256, (int(odd.sum()),), generator=g).to(torch.uint8)          # any non-zero byte keeps
    coef = torch.where(keep, torch.rand(P, generator=g) * 1.5 + 0.5, torch.zeros(P))
    scale = torch.tensor([0.37], device="cuda")
    kept_d, coef_d = kept.cuda(), coef.cuda()
    gbuf, gview = _grad_out(d, dtype)
    for entry, sel_d, sel in (("fs_ohem_ce_up_bwd", kept_d, keep.double()), ("fs_ohem_ce_up_bwd_coef", coef_d, coef.double())):
        _twice(lambda ws: K.call(entry, K._stream(), ctypes.byref(d), K._p(x_dev), K._p(tgt), K._p(lse.view), K._p(sel_d), K._p(scale),
                                 K._p(gbuf.view), K._p(ws.view), ws.n * 4), d, gbuf, what + " " + entry)
        gref = R.ohem_grad(x, HW, target, sel, 0.37, IGNORE)
        gref32 = R.ohem_grad(x.float(), HW, target, sel, 0.37, IGNORE, torch.float32)
        _check_grad(gbuf, gview, d, gref, gref32, "%s %s" % (what, entry[len("fs_ohem_ce_up_"):]))
    return tp.view, nll.view, gview, d


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("row,dist", OHEM_CASES, ids=["row%d-%s" % c for c in OHEM_CASES])
def test_ohem_up_matches_fp64(row, dist, dtype):
    _ohem_up_case(row, dist, DTYPES[dtype])


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_ohem_up_every_pixel_ignored(dtype):
    """No valid pixel: true_prob 1, nll 0 everywhere and a gradient of exact zeros although every kept byte / coefficient is set."""
    tp, nll, gview, d = _ohem_up_case(2, "n2", DTYPES[dtype], all_ignored=True)
    assert bool((tp == 1).all()) and bool((nll == 0).all()) and bool((gview == 0).all())


# ---- KL distillation from low-resolution logits -------------------------------------------------------------------------------
def _teacher_like(row):
    N, C, cs, hw, HW = ROWS[row]
    return dict(hw=hw, cs=cs)


KL_PAIRS = {   # student row or (N, C, cs, hw, HW), teacher (hw, cs), (student dtype, teacher dtype) combinations
    "same1": (1, _teacher_like(1), [("fp32", "fp32"), ("bf16", "bf16"), ("fp32", "bf16")]),
    "same3": (3, _teacher_like(3), [("fp32", "fp32"), ("bf16", "bf16"), ("fp32", "bf16")]),
    "same5": (5, _teacher_like(5), [("fp32", "fp32"), ("bf16", "bf16"), ("fp32", "bf16")]),
    "row1_coarser_teacher": (1, dict(hw=(4, 6), cs=20), [("fp32", "bf16"), ("bf16", "bf16")]),
    "row3_teacher_5x7": (3, dict(hw=(5, 7), cs=32), [("fp32", "fp32"), ("bf16", "fp32")]),
    "finer_teacher": ((2, 19, 32, (4, 6), (64, 96)), dict(hw=(8, 12), cs=32), [("fp32", "fp32"), ("bf16", "bf16")]),
    "row2_teacher_1x1": (2, dict(hw=(1, 1), cs=20), [("fp32", "fp32"), ("bf16", "fp32")]),
}
KL_CASES = [(name, dts, dist) for name, (s, _, combos) in KL_PAIRS.items() for dts in combos
            for dist in (DISTS[:1] if name == "same5" else DISTS)]


@pytest.mark.parametrize("name,dts,dist", KL_CASES, ids=["%s-s_%s-t_%s-%s" % (n, a, b, di) for n, (a, b), di in KL_CASES])
def test_kl_up_matches_fp64(name, dts, dist):
    from fasterseg_amd import kernels as K
    student, teacher, _ = KL_PAIRS[name]
    N, C, cs, hw, HW = ROWS[student] if isinstance(student, int) else student
    sdt, tdt = DTYPES[dts[0]], DTYPES[dts[1]]
    P = N * HW[0] * HW[1]
    s_dev, s = _lowres(N, C, cs, hw, sdt, dist, 400 + hw[0])
    t_dev, t = _lowres(N, C, teacher["cs"], teacher["hw"], tdt, dist, 500 + teacher["hw"][0])
    ds, dt = _desc(N, C, cs, hw, HW, sdt), _desc(N, C, teacher["cs"], teacher["hw"], HW, tdt)
    what = "kl_up %s %s s_%s t_%s" % (name, dist, dts[0], dts[1])
    kl, ls, lt = Guarded(P), Guarded(P), Guarded(P)
    K.call("fs_kl_distill_up_fwd", K._stream(), ctypes.byref(ds), K._p(s_dev), ctypes.byref(dt), K._p(t_dev), K._p(kl.view), K._p(ls.view),
           K._p(lt.view))
    torch.cuda.synchronize()
    assert kl.intact() and ls.intact() and lt.intact(), what + ": wrote outside a per-pixel vector"
    ref = R.kl_vectors(R.upsample(s, HW), R.upsample(t, HW))
    ref32 = R.kl_vectors(R.upsample(s, HW, torch.float32), R.upsample(t, HW, torch.float32))
    for name_, got, k in (("kl", kl, 0), ("lse_s", ls, 1), ("lse_t", lt, 2)):
        _check(got.view, ref[k], ref32[k], "%s fwd %s" % (what, name_))
    scale = torch.tensor([1.7], device="cuda")
    gbuf, gview = _grad_out(ds, sdt)
    _twice(lambda ws: K.call("fs_kl_distill_up_bwd", K._stream(), ctypes.byref(ds), K._p(s_dev), ctypes.byref(dt), K._p(t_dev), K._p(ls.view),
                             K._p(lt.view), K._p(scale), K._p(gbuf.view), K._p(ws.view), ws.n * 4), ds, gbuf, what + " bwd")
    gref = R.kl_grad(s, t, HW, 1.7)
    gref32 = R.kl_grad(s.float(), t.float(), HW, 1.7, torch.float32)
    _check_grad(gbuf, gview, ds, gref, gref32, what + " bwd")


# ---- refused calls ---------------------------------------------------------------------------------------------------------------
def test_loss_up_refuses_bad_descriptors_and_writes_nothing():
    """Refused on the host before any launch: FS_ERR_INVALID and not one output element changed.  Every buffer is large enough
    for the call had it been accepted."""
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    lib = _lib.lib()
    big = 1 << 16
    x = torch.zeros(big, device="cuda")
    tgt = torch.zeros(big, dtype=torch.long, device="cuda")
    kept = torch.ones(big, dtype=torch.uint8, device="cuda")
    coef = torch.ones(big, device="cuda")
    lse_in = torch.zeros(big, device="cuda")
    scale = torch.ones(1, device="cuda")
    outs = [Guarded(big) for _ in range(5)]            # three vectors, the gradient, the workspace
    v0, v1, v2, grad, ws = outs
    good = dict(N=1, h=2, w=3, C=19, cs=20, H=4, W=6, dtype=_lib.FS_F32)

    def desc(**kw):
        f = dict(good)
        f.update(kw)
        return _lib.LogitsDesc(f["N"], f["h"], f["w"], f["C"], f["cs"], f["H"], f["W"], f["dtype"])

    def ws_bytes(d):
        return max(int(lib.fs_loss_up_workspace_bytes(ctypes.byref(d))), 0)

    def ohem(d, short=0):
        st, r, n = K._stream(), ctypes.byref(d), ws_bytes(d) - short
        fwd = [] if short else [lib.fs_ohem_ce_up_fwd(st, r, K._p(x), K._p(tgt), IGNORE, K._p(v0.view), K._p(v1.view), K._p(v2.view))]
        return fwd + [lib.fs_ohem_ce_up_bwd(st, r, K._p(x), K._p(tgt), K._p(lse_in), K._p(kept), K._p(scale), K._p(grad.view), K._p(ws.view), n),
                      lib.fs_ohem_ce_up_bwd_coef(st, r, K._p(x), K._p(tgt), K._p(lse_in), K._p(coef), K._p(scale), K._p(grad.view), K._p(ws.view), n)]

    def kl(d_s, d_t, short=0):
        st, rs, rt, n = K._stream(), ctypes.byref(d_s), ctypes.byref(d_t), ws_bytes(d_s) - short
        fwd = [] if short else [lib.fs_kl_distill_up_fwd(st, rs, K._p(x), rt, K._p(x), K._p(v0.view), K._p(v1.view), K._p(v2.view))]
        return fwd + [lib.fs_kl_distill_up_bwd(st, rs, K._p(x), rt, K._p(x), K._p(lse_in), K._p(lse_in), K._p(scale), K._p(grad.view), K._p(ws.view), n)]

    bad = dict(C21=desc(C=21, cs=24), cs68=desc(cs=68), cs_not_mult4=desc(C=16, cs=18), cs_below_C=desc(cs=16), dtype=desc(dtype=5))
    for name, d in bad.items():
        assert ohem(d) == [FS_ERR_INVALID] * 3, name
        assert kl(d, desc()) == [FS_ERR_INVALID] * 2 and kl(desc(), d) == [FS_ERR_INVALID] * 2, name
    assert ohem(desc(), short=1) == [FS_ERR_INVALID] * 2 and kl(desc(), desc(), short=1) == [FS_ERR_INVALID], "workspace one byte short (the backwards)"
    for name, d in dict(N=desc(N=2), C=desc(C=18), H=desc(H=5), W=desc(W=7)).items():
        assert kl(desc(), d) == [FS_ERR_INVALID] * 2 and kl(d, desc()) == [FS_ERR_INVALID] * 2, "student / teacher differ in " + name
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused call wrote something"
    assert ohem(desc()) == [0, 0, 0] and kl(desc(), desc(h=1, w=1, cs=32, dtype=_lib.FS_F32)) == [0, 0]       # the good descriptor is accepted
    torch.cuda.synchronize()
    assert all(o.intact() for o in outs) and not grad.untouched()


# ---- csrc/loss.hip: the same criteria on full-resolution NCHW fp32 logits ---------------------------------------------------------
FULL_SHAPES = [(3, 19, 7, 9), (1, 1, 1, 1), (2, 20, 1, 257), (2, 33, 5, 5), (1, 2, 16, 16)]


@functools.lru_cache(maxsize=None)
def _full(shape, dist, seed):
    return _draw(shape, dist, torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=["x".join(map(str, s)) for s in FULL_SHAPES])
def test_ohem_full_resolution_matches_fp64(shape, dist):
    from fasterseg_amd import kernels as K
    B, C, H, W = shape
    P = B * H * W
    x = _full(shape, dist, 600 + C)
    x_dev = x.cuda()
    target = _labels(B, H, W, C, 700 + C)
    tgt = target.cuda()
    what = "ohem_full %s %s" % ("x".join(map(str, shape)), dist)
    tp, nll, lse = Guarded(P), Guarded(P), Guarded(P)
    K.call("fs_ohem_ce_fwd", K._stream(), K._p(x_dev), K._p(tgt), B, C, H * W, IGNORE, K._p(tp.view), K._p(nll.view), K._p(lse.view))
    torch.cuda.synchronize()
    assert tp.intact() and nll.intact() and lse.intact()
    ref, ref32 = R.ohem_vectors(x.double(), target, IGNORE), R.ohem_vectors(x, target, IGNORE)
    for name, got, k in (("true_prob", tp, 0), ("nll", nll, 1), ("lse", lse, 2)):
        _check(got.view, ref[k], ref32[k], "%s fwd %s" % (what, name))
    dead = ~ref[3].cuda()
    assert bool((tp.view[dead] == 1).all()) and bool((nll.view[dead] == 0).all())
    g = torch.Generator().manual_seed(800 + C)
    keep = torch.rand(P, generator=g) < 0.6
    kept = keep.to(torch.uint8)
    odd = keep & (torch.rand(P, generator=g) < 0.3)
    kept[odd] = torch.randint(2, 256, (int(odd.sum()),), generator=g).to(torch.uint8)
    coef = torch.where(keep, torch.rand(P, generator=g) * 1.5 + 0.5, torch.zeros(P))
    scale = torch.tensor([0.37], device="cuda")
    kept_d, coef_d = kept.cuda(), coef.cuda()
    for entry, sel_d, sel in (("fs_ohem_ce_bwd", kept_d, keep.double()), ("fs_ohem_ce_bwd_coef", coef_d, coef.double())):
        gbuf = Guarded(x.numel())
        K.call(entry, K._stream(), K._p(x_dev), K._p(tgt), K._p(lse.view), K._p(sel_d), K._p(scale), B, C, H * W, K._p(gbuf.view))
        torch.cuda.synchronize()
        assert gbuf.intact()
        _check(gbuf.view, R.ohem_grad(x, None, target, sel, 0.37, IGNORE), R.ohem_grad(x, None, target, sel, 0.37, IGNORE, torch.float32),
               "%s %s" % (what, entry[len("fs_ohem_ce_"):]))


def _kl_full(s, t, what):
    from fasterseg_amd import kernels as K
    B, C, H, W = s.shape
    P = B * H * W
    s_dev, t_dev = s.cuda(), t.cuda()
    kl, ls, lt = Guarded(P), Guarded(P), Guarded(P)
    K.call("fs_kl_distill_fwd", K._stream(), K._p(s_dev), K._p(t_dev), B, C, H * W, K._p(kl.view), K._p(ls.view), K._p(lt.view))
    torch.cuda.synchronize()
    assert kl.intact() and ls.intact() and lt.intact()
    ref, ref32 = R.kl_vectors(s.double(), t.double()), R.kl_vectors(s, t)
    for name, got, k in (("kl", kl, 0), ("lse_s", ls, 1), ("lse_t", lt, 2)):
        _check(got.view, ref[k], ref32[k], "%s fwd %s" % (what, name))
    scale = torch.tensor([1.7], device="cuda")
    gbuf = Guarded(s.numel())
    K.call("fs_kl_distill_bwd", K._stream(), K._p(s_dev), K._p(t_dev), K._p(ls.view), K._p(lt.view), K._p(scale), B, C, H * W, K._p(gbuf.view))
    torch.cuda.synchronize()
    assert gbuf.intact()
    gref = R.kl_grad(s, t, None, 1.7)
    assert bool(torch.isfinite(gref).all()) and bool(torch.isfinite(ref[0]).all())
    _check(gbuf.view, gref, R.kl_grad(s, t, None, 1.7, torch.float32), what + " bwd")


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("shape", FULL_SHAPES, ids=["x".join(map(str, s)) for s in FULL_SHAPES])
def test_kl_full_resolution_matches_fp64(shape, dist):
    _kl_full(_full(shape, dist, 900 + shape[1]), _full(shape, dist, 950 + shape[1]), "kl_full %s %s" % ("x".join(map(str, shape)), dist))


def test_kl_full_resolution_teacher_with_minus_infinity():
    """A teacher class at -inf on some pixels: p_t = 0 there, the xlogy guard gives the finite fp64 value and a finite gradient."""
    s = _full((3, 19, 7, 9), "n2", 960)
    t = _full((3, 19, 7, 9), "n2", 961).clone()
    t[:, 4, ::2, 1::3] = float("-inf")
    t[1, 0, 3, :] = float("-inf")
    _kl_full(s, t, "kl_full -inf teacher")


# ---- one rule for labels outside [0, C) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_kept", [0, "P/16"])
@pytest.mark.parametrize("where", ["full", "lowres-fp32", "lowres-bf16"])
def test_unweighted_and_unit_weighted_criteria_ignore_out_of_range_labels(where, min_kept):
    """ProbOhemCrossEntropy2d without weights and with all weights 1 on labels that include -1, C, 254 and 2**32 + 3: the same loss
    and gradient, both equal to the fp64 criterion that ignores those pixels (fs_ohem_select's documented rule)."""
    from fasterseg_amd import kernels as K
    from fasterseg_amd.losses import ProbOhemCrossEntropy2d, ohem_ce_lowres
    N, C, cs, hw, HW = ROWS[1]
    P = N * HW[0] * HW[1]
    mk = 0 if min_kept == 0 else P // 16
    target = _labels(N, HW[0], HW[1], C, 201)
    assert int((~R.valid_mask(target, C, IGNORE) & target.ne(IGNORE)).sum()) == 12
    crits = [ProbOhemCrossEntropy2d(IGNORE, thresh=0.7, min_kept=mk), ProbOhemCrossEntropy2d(IGNORE, thresh=0.7, min_kept=mk, weight=torch.ones(C))]
    if where == "full":
        x = _full((N, C) + HW, "n2", 970)
        size, dtype = None, torch.float32
        run = lambda crit: (lambda v: (crit(v, target.cuda()), v))(x.cuda().requires_grad_(True))
        ref_logits = x.double()
    else:
        dtype = torch.float32 if where.endswith("fp32") else torch.bfloat16
        x_dev, x = _lowres(N, C, cs, hw, dtype, "n2", 101)
        size = HW
        x_clean = K.empty_nhwc(N, C, hw[0], hw[1], dtype, "cuda", cs=cs, zero=True)
        x_clean.copy_(x.cuda())
        run = lambda crit: (lambda v: (ohem_ce_lowres(crit, v, target.cuda()), v))(x_clean.detach().requires_grad_(True))
        ref_logits = R.upsample(x, HW)
    want, coef = R.ohem_criterion(ref_logits, target, 0.7, mk, IGNORE)
    assert int((coef > 0).sum()) > 0 and bool((coef[~R.valid_mask(target, C, IGNORE).reshape(-1)] == 0).all())
    gref = R.ohem_grad(x, size, target, coef, 1.0 / float(coef.sum()), IGNORE)
    gref32 = R.ohem_grad(x.float(), size, target, coef, 1.0 / float(coef.sum()), IGNORE, torch.float32)
    got = []
    for crit, kind in zip(crits, ("unweighted", "weights=1")):
        loss, v = run(crit)
        loss.backward()
        assert abs(float(loss.detach()) - float(want)) <= 2e-5 * max(1.0, abs(float(want))), (kind, float(loss.detach()), float(want))
        _check(v.grad, gref, gref32, "label rule %s %s min_kept=%d" % (where, kind, mk), bf16_out=dtype == torch.bfloat16)
        got.append((float(loss.detach()), v.grad.float().cpu()))
    assert abs(got[0][0] - got[1][0]) <= 1e-6 * max(1.0, abs(got[1][0])), (got[0][0], got[1][0])
    assert float((got[0][1] - got[1][1]).abs().max()) <= 8 * EPS32 * float(gref.abs().max())
