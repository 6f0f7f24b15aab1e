"""Class maps against an independent reference: fs_bilinear_argmax (the x8 strip kernel and the generic kernel of csrc/eval.hip) and
fs_heads_confusion (csrc/eval_heads.hip) against the arg-max of the fp64 up-sample of the storage-rounded logits (tests/_loss_ref.py).

Pass rule (the one of tests/test_ms_eval_gpu.py): a pixel is clear when the two largest fp64 values are more than 1e-4 apart - fp32
interpolation of unit-normal logits errs by about 1e-6, two orders of magnitude less.  On a clear pixel the class must be the fp64
arg-max, on every other pixel a class whose fp64 value is within 1e-4 of the maximum; no pixel goes unchecked, and at least 99.9 %
of the pixels of every case are clear (asserted; the seeds below were fixed on the CPU so that it holds: the clear share is
0.9996 .. 1.0 for fs_bilinear_argmax and exactly 1 for every fs_heads_confusion case, where the counts must match numpy exactly).
Pad channels [C, cs) hold NaN: they are loaded with the last quad and must never win.  Ties: the lowest class index wins."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _loss_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
SENT = 0xEE
GUARD = 64

ARGMAX_CASES = {   # N, C, (h, w), (H, W), cs
    "x8_strip": (2, 19, (9, 13), (72, 104), 32),
    "generic": (1, 19, (7, 11), (29, 44), 20),
    "down_in_H": (2, 7, (5, 3), (3, 8), 8),
    "x8_five_full_quads_Wi2": (1, 20, (2, 2), (16, 16), 20),
    "Wi1": (1, 19, (6, 1), (11, 4), 24),
    "x8_geometry_C25_generic": (1, 25, (8, 16), (64, 128), 28),
    "generic_5x5": (1, 19, (5, 5), (5, 8), 32),
}

HEADS_CASES = {    # N, C, (h, w), (H, W), channel strides (K = their number)
    "K1_x8": (1, 20, (2, 2), (16, 16), [20]),
    "K1_generic": (1, 19, (5, 5), (5, 8), [32]),
    "K3_generic_down": (2, 7, (5, 3), (3, 8), [8, 12, 16]),
    "K3_x8": (1, 19, (3, 5), (20, 40), [20, 32, 24]),
    "K5_x8": (1, 19, (3, 5), (20, 40), [32, 20, 24, 32, 28]),
    "K5_generic": (1, 19, (6, 1), (11, 4), [24, 20, 32, 28, 64]),
}
# (case, dtype) -> seed index, 0 where not listed: the first for which every pixel of every head is clear
HEADS_SEEDS = {("K3_x8", "fp32"): 1, ("K3_x8", "bf16"): 1, ("K5_x8", "fp32"): 1, ("K5_x8", "bf16"): 5}


def _logits(N, C, hw, dtype, seed):
    """Unit-normal logits rounded to the storage dtype (CPU, (N, C, h, w))."""
    return torch.randn((N, C) + tuple(hw), generator=torch.Generator().manual_seed(seed)).to(dtype)


def _to_device(val, cs):
    """NHWC view (N, C, h, w) over an (N, h, w, cs) device buffer whose pad channels hold NaN."""
    N, C, h, w = val.shape
    buf = torch.full((N, h, w, cs), float("nan"), dtype=val.dtype, device="cuda")
    buf[..., :C] = val.permute(0, 2, 3, 1).cuda()
    return buf.permute(0, 3, 1, 2)[:, :C]


def _argmax(head, HW):
    """fs_bilinear_argmax into a sentinel-guarded class map."""
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    N, C, h, w = head.shape
    n = N * HW[0] * HW[1]
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.uint8, device="cuda")
    d = _lib.ResizeDesc(N, h, w, HW[0], HW[1], C, K.channel_stride(head), 0, K.dtype_code(head.dtype), 0, 0)
    K.call("fs_bilinear_argmax", K._stream(), ctypes.byref(d), K._p(head), K._p(buf[GUARD:]))
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()), "wrote outside the class map"
    return buf[GUARD:GUARD + n].view(N, HW[0], HW[1]).cpu()


def heads_seed(case, dtype):
    return HEADS_SEEDS.get((case, dtype), 0)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", list(ARGMAX_CASES))
def test_bilinear_argmax_matches_fp64_class_map(case, dtype):
    N, C, hw, HW, cs = ARGMAX_CASES[case]
    val = _logits(N, C, hw, DTYPES[dtype], 1000)
    up, arg, gap = R.class_map(val, HW)
    got = _argmax(_to_device(val, cs), HW)
    assert int(got.max()) < C
    share = R.check_class_map(got, up, arg, gap)
    print("clear share %s %s: %.4f" % (case, dtype, share))
    assert share >= 0.999, share


def _tie_inputs(N, C, hw, dtype, a, b):
    """Classes a < b bit-identical and at least 1 above every other class; and a map whose every class is the same constant."""
    x = torch.randn((N, C) + tuple(hw), generator=torch.Generator().manual_seed(5))
    top = x.amax(1) + 1.5 + torch.rand((N,) + tuple(hw), generator=torch.Generator().manual_seed(6))
    x[:, a] = top
    x[:, b] = top
    x = x.to(dtype)
    assert torch.equal(x[:, a], x[:, b])
    others = [c for c in range(C) if c not in (a, b)]
    assert float((x[:, a].float() - x[:, others].float().amax(1)).min()) >= 1.0
    return x, torch.full((N, C) + tuple(hw), 0.75).to(dtype)


TIE_GEOMETRIES = {"x8_strip": (2, 19, (9, 13), (72, 104), 32), "generic": (1, 19, (7, 11), (29, 44), 20)}


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("geometry", list(TIE_GEOMETRIES))
def test_first_maximum_wins(geometry, dtype):
    """Exact ties (random normals never tie): class a of two bit-identical winning maps a < b, class 0 of an all-equal map, at every
    pixel, through fs_bilinear_argmax and - counted in column a / 0 - through fs_heads_confusion."""
    from fasterseg_amd import kernels as K
    N, C, hw, HW, cs = TIE_GEOMETRIES[geometry]
    a, b = 6, 17
    tied, flat = _tie_inputs(N, C, hw, DTYPES[dtype], a, b)
    gt = torch.randint(0, C, (N,) + HW, generator=torch.Generator().manual_seed(7))
    gt[torch.rand((N,) + HW, generator=torch.Generator().manual_seed(8)) < 0.1] = 255
    for val, winner in ((tied, a), (flat, 0)):
        head = _to_device(val, cs)
        got = _argmax(head, HW)
        assert bool((got == winner).all()), "%d pixels are not class %d" % (int((got != winner).sum()), winner)
        hist = torch.zeros(C * C, dtype=torch.int64, device="cuda")
        counts = torch.zeros(2, dtype=torch.int64, device="cuda")
        K.heads_confusion([head], gt.to(torch.uint8).cuda(), hist, counts)
        want, labeled, correct = R.hist_info(C, np.full(gt.numel(), winner), gt.reshape(-1).numpy())
        assert np.array_equal(hist.cpu().numpy().reshape(C, C), want) and int(want[:, winner].sum()) == labeled
        assert counts.tolist() == [labeled, correct]


def _gt(N, HW, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, C, (N,) + tuple(HW), generator=g)
    drop = torch.rand((N,) + tuple(HW), generator=g)
    t[drop < 0.06] = 255
    if kind == "u8":
        return t.to(torch.uint8)
    t[(drop >= 0.06) & (drop < 0.1)] = -1
    t[(drop >= 0.1) & (drop < 0.13)] = C + 1
    return t.to(torch.int64 if kind == "i64" else torch.int32)


@pytest.mark.parametrize("kind", ["u8", "i32", "i64"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("case", list(HEADS_CASES))
def test_heads_confusion_matches_fp64_class_map(case, dtype, kind):
    """Every pixel of every head is clear (asserted), so hist, labeled and correct equal numpy's hist_info of the fp64 arg-max exactly."""
    from fasterseg_amd import kernels as K
    N, C, hw, HW, strides = HEADS_CASES[case]
    Kh = len(strides)
    vals = [_logits(N, C, hw, DTYPES[dtype], 2000 + 16 * heads_seed(case, dtype) + k) for k in range(Kh)]
    gt = _gt(N, HW, C, kind, 3000 + Kh)
    hist = torch.zeros(Kh * C * C, dtype=torch.int64, device="cuda")
    counts = torch.zeros(2 * Kh, dtype=torch.int64, device="cuda")
    K.heads_confusion([_to_device(v, cs) for v, cs in zip(vals, strides)], gt.cuda(), hist, counts)
    g = gt.reshape(-1).numpy().astype(np.int64)
    assert int(((g >= 0) & (g < C)).sum()) > 0
    for k, v in enumerate(vals):
        _, arg, gap = R.class_map(v, HW)
        assert bool((gap > 1e-4).all()), "head %d: not every pixel is clear - pick another seed" % k
        want, labeled, correct = R.hist_info(C, arg.reshape(-1).numpy(), g)
        assert np.array_equal(hist[k * C * C:(k + 1) * C * C].cpu().numpy().reshape(C, C), want), k
        assert counts[2 * k:2 * k + 2].tolist() == [labeled, correct], k
