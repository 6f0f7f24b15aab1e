"""fs_ohem_select (losses.ohem_select): exact k-th-smallest radix select + kept set + class-weighted reduction, against the formula
of losses._OhemCE.forward written in torch (torch.sort for the k-th value), with the weighted mean taken in float64.

Required in every case: result[2] bit-equal to the torch threshold, coef != 0 identical to torch's kept mask, equal counts, result[0]
within 1e-6 relative of the float64 weighted mean, and two calls bit-identical."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

IGNORE = 255


def _vectors(P, C, ignore_frac, seed, quant=None):
    """(true_prob, nll, target) as fs_ohem_ce_fwd leaves them: ignored pixels carry true_prob = 1, nll = 0."""
    g = torch.Generator().manual_seed(seed)
    tp = torch.rand(P, generator=g) * 0.999 + 0.0005
    if quant:
        tp = torch.floor(tp * quant) / quant
    tgt = torch.randint(0, C, (P,), generator=g)
    tgt[torch.rand(P, generator=g) < ignore_frac] = IGNORE
    nll = -torch.log(tp.clamp_min(1e-30))
    tp[tgt == IGNORE] = 1.0
    nll[tgt == IGNORE] = 0.0
    return tp.cuda(), nll.cuda(), tgt.cuda()


def _weight(C, seed=3):
    return (torch.rand(C, generator=torch.Generator().manual_seed(seed)) + 0.5).cuda()


def _torch_chain(tp, nll, tgt, C, thresh, min_kept, w):
    P = tp.numel()
    valid = tgt.ne(IGNORE)
    num_valid = valid.sum()
    kept = valid
    threshold = torch.full((), float(thresh), dtype=torch.float32, device=tp.device)
    apply = torch.zeros((), dtype=torch.bool, device=tp.device)
    if min_kept > 0:
        kth = torch.sort(tp).values[min(P, min_kept) - 1]
        threshold = torch.maximum(threshold, kth)
        apply = (num_valid >= min_kept) & (num_valid > 0)
        kept = valid & (tp.le(threshold) | ~apply)
    wt = torch.ones(P, dtype=torch.float64, device=tp.device) if w is None else w.double()[tgt.clamp(0, C - 1)]
    coef = wt * kept
    mean = (coef * nll.double()).sum() / coef.sum()
    return threshold, bool(apply), kept, int(num_valid), int(kept.sum()), float(mean), coef


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _check(tp, nll, tgt, C, thresh, min_kept, w=None):
    from fasterseg_amd.losses import ohem_select
    threshold, apply, kept, n_valid, n_kept, mean, coef_ref = _torch_chain(tp, nll, tgt, C, thresh, min_kept, w)
    coef, result, counts = ohem_select(tp, nll, tgt, C, IGNORE, thresh, min_kept, weight=w)
    coef2, result2, counts2 = ohem_select(tp, nll, tgt, C, IGNORE, thresh, min_kept, weight=w)
    torch.cuda.synchronize()
    got = result.cpu()
    print("ohem_select P=%d C=%d k=%d: threshold %r (torch %r) counts %s (torch %s) loss %r (fp64 %r)" % (
        tp.numel(), C, min_kept, float(got[2]), float(threshold), counts.tolist(), [n_valid, n_kept], float(got[0]), mean))
    assert int(_bits(result[2:3])) == int(_bits(threshold.reshape(1))), (float(got[2]), float(threshold))
    assert torch.equal(coef.ne(0), kept)
    assert counts.tolist() == [n_valid, n_kept]
    assert float(got[3]) == (1.0 if apply else 0.0)
    assert float((coef.double() - coef_ref).abs().max()) == 0.0              # the kept pixel's own class weight, exactly
    if math.isnan(mean):
        assert math.isnan(float(got[0]))
    else:
        assert abs(float(got[0]) - mean) <= 1e-6 * abs(mean), (float(got[0]), mean)
        assert abs(float(got[1]) - float(coef_ref.sum())) <= 1e-6 * float(coef_ref.sum())
    assert torch.equal(_bits(result), _bits(result2)) and torch.equal(counts, counts2) and torch.equal(_bits(coef), _bits(coef2))
    return got


@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_ties_k_inside_a_run_of_equal_values(weighted):
    P = 3 * 17 * 23
    tp, nll, tgt = _vectors(P, 19, 0.1, 1, quant=8)
    values, runs = torch.unique(tp, return_counts=True)
    assert int(runs.max()) > 50                                             # eight distinct values: long runs
    below = int((tp < values[2]).sum())
    k = below + int(runs[2]) // 2                                           # strictly inside the run of the third value
    got = _check(tp, nll, tgt, 19, 0.05, k, _weight(19) if weighted else None)
    assert float(got[2]) == float(values[2])


@pytest.mark.parametrize("which", ["k1", "kP", "beyond_P"])
def test_boundaries_of_k(which):
    P = 1000
    tp, nll, tgt = _vectors(P, 19, 0.0, 2)
    min_kept = {"k1": 1, "kP": P, "beyond_P": P + 5}[which]
    got = _check(tp, nll, tgt, 19, 0.0, min_kept, _weight(19))
    assert float(got[2]) == float(tp.min() if which == "k1" else tp.max())
    assert float(got[3]) == (0.0 if which == "beyond_P" else 1.0)


@pytest.mark.parametrize("which", ["min_kept_zero", "too_few_valid"])
def test_disabled_selection_keeps_every_valid_pixel(which):
    tp, nll, tgt = _vectors(2000, 19, 0.6, 4)
    min_kept = 0 if which == "min_kept_zero" else 1500                      # ~800 valid
    got = _check(tp, nll, tgt, 19, 0.3, min_kept, _weight(19))
    assert float(got[3]) == 0.0


def test_nothing_valid_gives_nan_and_zero_counts():
    tp, nll, tgt = _vectors(777, 19, 1.1, 5)
    got = _check(tp, nll, tgt, 19, 0.7, 100, _weight(19))
    assert math.isnan(float(got[0])) and float(got[1]) == 0.0 and float(got[2]) == 1.0


def test_extreme_values_force_every_radix_pass_to_decide():
    """Exact 0, the smallest subnormal, neighbours in the last mantissa bit and 1.0: k walks over all of them."""
    sub = float(torch.tensor(1, dtype=torch.int32).view(torch.float32))      # 2^-149
    a = torch.tensor(0.3, dtype=torch.float32)
    ulp = lambda x, n: (x.view(torch.int32) + n).view(torch.float32)
    vals = torch.stack([torch.tensor(0.0), torch.tensor(sub), torch.tensor(2 * sub), a, ulp(a, 1), ulp(a, 2), ulp(a, 1), a,
                        ulp(torch.tensor(1.0), -1), torch.tensor(1.0), torch.tensor(0.5), ulp(torch.tensor(0.5), -1),
                        ulp(torch.tensor(0.3), 1024), ulp(torch.tensor(0.3), 2048), torch.tensor(0.0), torch.tensor(1.0)])
    g = torch.Generator().manual_seed(6)
    tp = vals[torch.randperm(vals.numel(), generator=g)].cuda()
    nll = torch.rand(vals.numel(), generator=g).cuda()
    tgt = torch.randint(0, 19, (vals.numel(),), generator=g).cuda()
    order = torch.sort(tp).values.cpu()
    for k in range(1, vals.numel() + 1):
        got = _check(tp, nll, tgt, 19, 0.0, k)
        assert int(_bits(got[2:3])) == int(_bits(order[k - 1:k]))


@pytest.mark.parametrize("P", [4 * 128 * 160, 4 * 128 * 160 - 3, 2 * 2048 * 1024 + 1029], ids=["blocks", "odd", "grid_stride"])
def test_sizes_several_blocks_tail_and_grid_stride(P):
    """81 920 pixels: 80 blocks; an odd P leaves a scalar tail; past 2048 x 1024 pixels the capped grid strides."""
    tp, nll, tgt = _vectors(P, 19, 0.05, 7)
    _check(tp, nll, tgt, 19, 0.7, P // 16, _weight(19))
    _check(tp, nll, tgt, 19, 0.01, P // 16)


def test_unaligned_base_pointer():
    P = 4 * 128 * 160 - 3
    tp, nll, tgt = _vectors(P + 1, 19, 0.05, 8)
    view = tp[1:]
    assert view.data_ptr() % 16 == 4
    _check(view, nll[:P], tgt[:P], 19, 0.2, P // 16, _weight(19))
    _check(view, nll[1:], tgt[1:], 19, 0.2, P // 16, _weight(19))           # every vector off the 16-byte grid by one element


@pytest.mark.parametrize("C", [19, 7])
@pytest.mark.parametrize("weighted", [False, True], ids=["none", "random"])
def test_weights_and_class_counts(C, weighted):
    tp, nll, tgt = _vectors(5000, C, 0.1, 9 + C)
    _check(tp, nll, tgt, C, 0.4, 700, _weight(C, seed=C) if weighted else None)


def test_bad_arguments_return_a_status_and_a_message():
    import ctypes
    from fasterseg_amd import _lib
    from fasterseg_amd import kernels as K
    from fasterseg_amd.losses import ohem_select
    tp, nll, tgt = _vectors(300, 19, 0.1, 10)
    with pytest.raises(_lib.FasterSegHipError, match="C = 21"):
        ohem_select(tp, nll, tgt, 21, IGNORE, 0.7, 10)
    short = torch.empty(16, dtype=torch.long, device="cuda")
    with pytest.raises(_lib.FasterSegHipError, match="workspace"):
        ohem_select(tp, nll, tgt, 19, IGNORE, 0.7, 10, workspace=short)
    h = _lib.lib()
    need = int(h.fs_ohem_select_workspace_bytes(300))
    assert need > 128 and int(h.fs_ohem_select_workspace_bytes(0)) == 0
    out = torch.empty(300, device="cuda")
    res, cnt = torch.empty(4, device="cuda"), torch.empty(2, dtype=torch.long, device="cuda")
    status = h.fs_ohem_select(K._stream(), K._p(tp), K._p(nll), K._p(tgt), 300, 19, IGNORE, None, ctypes.c_float(0.7), 10, K._p(out),
                              K._p(res), K._p(cnt), K._p(short), need - 8)
    assert status != 0 and b"workspace" in h.fs_last_error()
    assert h.fs_ohem_select(K._stream(), None, K._p(nll), K._p(tgt), 300, 19, IGNORE, None, ctypes.c_float(0.7), 10, K._p(out), K._p(res),
                            K._p(cnt), K._p(short), need) != 0
    assert h.fs_ohem_select(K._stream(), K._p(tp), K._p(nll), K._p(tgt), 0, 19, IGNORE, None, ctypes.c_float(0.7), 10, K._p(out), K._p(res),
                            K._p(cnt), K._p(short), need) != 0
    torch.cuda.synchronize()
