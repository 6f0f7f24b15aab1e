"""The reference and bound of the multi-tensor SGD kernel (tests/_sgd_ref.py), checked on the CPU: they pass an honest update and fail a
subtly wrong one.  Companion of tests/test_bwd_bounds_selfcheck.py; tests/test_flat_sgd_gpu.py holds the kernel to the same bound.

Honest: the update on the zoo's operands with every operation rounded to fp32, in three operation orders, and two contracted forms that
round once from fp64 where the compiler may emit an fma.  Every element of every tensor must lie inside the bound; the worst
err / bound is printed (pytest -s) and must be below 1.

Mutants, each of which must put AT LEAST ONE ELEMENT OF EVERY TENSOR IT APPLIES TO outside the bound (exact fp64 arithmetic of the wrong
formula: what is caught is the formula, not its rounding):
   1. wd_after_blend   weight decay added after the momentum blend (the momentum buffer does not carry it);
   2. clip_on_decay    the clip factor applied to the decay term too;
   3. nesterov         p -= lr (g' + mu b);
   4. dampening        b = mu m + (1 - mu) g';
   5. no_momentum      p -= lr g', the buffer is overwritten with g';
   6. grad_param_order the gradient slice of a filter read in parameter order [O][I][taps] (filters with taps > 1 and I > 1);
   7. flip_one_axis    the rotated pack flipped along R only (3x3 packs);
   8. flip_none        the rotated pack not rotated (3x3 packs);
   9. fwd_oihw         the forward pack in OIHW order (3x3 packs: for a 1x1 filter the two orders coincide);
  10. bf16_truncated   a bf16 pack truncated where it should be rounded (every pack, bf16).
A mutant that survives on some tensor means the operands are too tame: the zoo's values change, not this list."""
import numpy as np
import pytest
import torch

from tests import _sgd_ref as R

LR, MU, WD, C = R.f32(0.05), R.f32(0.9), R.f32(5e-4), R.f32(0.37)
V = R.Values()
f = np.float32


def r32(x64):
    """one rounding of an fp64 expression to fp32 (the products of two fp32 values are exact in fp64)"""
    return x64.astype(np.float32)


def honest(order, p, m, g):
    """fp32 emulations -> (m', p') widened"""
    lr, mu, wd, c = f(LR), f(MU), f(WD), f(C)
    pd, md, gd = p.astype(np.float64), m.astype(np.float64), g.astype(np.float64)
    if order == "kernel":                                   # (g c + wd p), then mu m + that: the order the source is written in
        b = mu * m + (g * c + wd * p)
        return b.astype(np.float64), (p - lr * b).astype(np.float64)
    if order == "blend_first":                              # (mu m + c g) + wd p
        b = (mu * m + c * g) + wd * p
        return b.astype(np.float64), (p - lr * b).astype(np.float64)
    if order == "decay_first":                              # (wd p + mu m) + c g
        b = (wd * p + mu * m) + c * g
        return b.astype(np.float64), (p - lr * b).astype(np.float64)
    if order == "fma":                                      # fma(g, c, wd p), fma(mu, m, g'), fma(-lr, b, p)
        gp = r32(gd * C + (wd * p).astype(np.float64))
        b = r32(MU * md + gp.astype(np.float64))
        return b.astype(np.float64), r32(pd - LR * b.astype(np.float64)).astype(np.float64)
    assert order == "fma_other"                             # fma(wd, p, g c), the blend and the step as two operations each
    gp = r32(WD * pd + (g * c).astype(np.float64))
    b = mu * m + gp
    return b.astype(np.float64), (p - lr * b).astype(np.float64)


ORDERS = ["kernel", "blend_first", "decay_first", "fma", "fma_other"]


def test_numpy_keeps_float32_arithmetic_in_float32():
    """the emulations rely on it: float32 scalar (op) float32 array stays float32"""
    assert (f(0.9) * V.m[3] + V.g[3]).dtype == np.float32


@pytest.mark.parametrize("order", ORDERS)
def test_honest_updates_stay_inside_the_bound(order):
    worst = 0.0
    for k, shape in enumerate(R.SHAPES):
        p, m, g = V.p[k], V.m[k], V.g[k]
        pd, md, gd = (a.astype(np.float64) for a in (p, m, g))
        m64, p64 = R.step64(pd, md, gd, C, LR, MU, WD)
        bm, bp = R.bound(pd, md, gd, C, LR, MU, WD)
        me, pe = honest(order, p, m, g)
        rm, rp = float((np.abs(me - m64) / bm).max()), float((np.abs(pe - p64) / bp).max())
        worst = max(worst, rm, rp)
        assert rm <= 1 and rp <= 1, (order, shape, rm, rp)
    print("honest %-12s worst err / bound over the zoo %.3f" % (order, worst))
    assert worst < 1


def _perm_param_order(g):
    """what a walk in gradient order reads when it indexes the slice in PARAMETER order: the flat [O][R][S][I] slice reinterpreted as
    [O][I][R][S]"""
    return R.to_grad_order(g).reshape(g.shape)


def mutant(name, p, m, g):
    """exact fp64 -> (m', p')"""
    gp = C * g + WD * p
    if name == "wd_after_blend":
        b = MU * m + C * g
        return b, p - LR * (b + WD * p)
    if name == "clip_on_decay":
        b = MU * m + C * (g + WD * p)
        return b, p - LR * b
    if name == "nesterov":
        b = MU * m + gp
        return b, p - LR * (gp + MU * b)
    if name == "dampening":
        b = MU * m + (1 - MU) * gp
        return b, p - LR * b
    if name == "no_momentum":
        return gp, p - LR * gp
    assert name == "grad_param_order"
    return R.step64(p, m, _perm_param_order(g), C, LR, MU, WD)


UPDATE_MUTANTS = ["wd_after_blend", "clip_on_decay", "nesterov", "dampening", "no_momentum", "grad_param_order"]


@pytest.mark.parametrize("name", UPDATE_MUTANTS)
def test_update_mutants_are_caught_on_every_tensor(name):
    applied = 0
    for k, shape in enumerate(R.SHAPES):
        if name == "grad_param_order" and not (len(shape) == 4 and shape[2] * shape[3] > 1 and shape[1] > 1):
            continue
        pd, md, gd = (a.astype(np.float64) for a in (V.p[k], V.m[k], V.g[k]))
        m64, p64 = R.step64(pd, md, gd, C, LR, MU, WD)
        bm, bp = R.bound(pd, md, gd, C, LR, MU, WD)
        mm, pm = mutant(name, pd, md, gd)
        out = int((np.abs(mm - m64) > bm).sum()) + int((np.abs(pm - p64) > bp).sum())
        print("%-18s %-18s outside the bound: %7d of %d" % (name, shape, out, 2 * pd.size))
        assert out >= 1, "%s survives on %s: the operands are too tame" % (name, shape)
        applied += 1
    assert applied >= (10 if name == "grad_param_order" else len(R.SHAPES))


def pack_mutant(name, p, dtype):
    """-> (fwd, flip) bit patterns"""
    if name == "flip_one_axis":
        return R.packs64(p, dtype)[0], R.pack_bits(p[:, :, ::-1, :].transpose(1, 2, 3, 0), dtype)
    if name == "flip_none":
        return R.packs64(p, dtype)[0], R.pack_bits(p.transpose(1, 2, 3, 0), dtype)
    if name == "fwd_oihw":
        return R.pack_bits(p, dtype).reshape(p.shape[0], p.shape[2], p.shape[3], p.shape[1]), R.packs64(p, dtype)[1]
    assert name == "bf16_truncated" and dtype == torch.bfloat16
    trunc = lambda a: (np.ascontiguousarray(a.astype(np.float32)).view(np.int32) >> 16).astype(np.int16)
    return trunc(p.transpose(0, 2, 3, 1)), trunc(p[:, :, ::-1, ::-1].transpose(1, 2, 3, 0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["flip_one_axis", "flip_none", "fwd_oihw", "bf16_truncated"])
def test_pack_mutants_are_caught_on_every_pack(name, dtype):
    if name == "bf16_truncated" and dtype != torch.bfloat16:
        return                                              # truncation is the identity on an fp32 pack: the mutant does not exist there
    applied = 0
    for k, shape in enumerate(R.SHAPES):
        if not R.packable(shape):
            continue
        if name != "bf16_truncated" and shape[2] == 1:
            continue                                        # a 1x1 filter has nothing to rotate, and its OIHW order IS [O][R][S][I]
        p = V.p[k].astype(np.float64)
        want, got = R.packs64(p, dtype), pack_mutant(name, p, dtype)
        diff = sum(int((a != b).sum()) for a, b in zip(want, got))
        print("%-14s %-18s %-8s differing pack elements: %7d of %d" % (name, shape, str(dtype)[6:], diff, 2 * p.size))
        assert diff >= 1, (name, shape)
        applied += 1
    assert applied == (5 if name == "bf16_truncated" else 2)


def test_packs64_is_the_transpose_it_says():
    """element by element on a small filter: fwd[o,r,s,i] = p[o,i,r,s], flip[i,r,s,o] = p[o,i,R-1-r,S-1-s]; bf16 rounds to nearest EVEN"""
    p = np.arange(8 * 8 * 3 * 3, dtype=np.float64).reshape(8, 8, 3, 3)
    fwd, flip = R.packs64(p, torch.float32)
    fwd, flip = fwd.view(np.float32), flip.view(np.float32)
    for o, i, r, s in [(0, 0, 0, 0), (1, 2, 0, 2), (7, 5, 2, 1), (3, 7, 1, 1)]:
        assert fwd[o, r, s, i] == p[o, i, r, s] and flip[i, r, s, o] == p[o, i, 2 - r, 2 - s]
    ties = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20]).reshape(1, 3, 1, 1)      # down to even, up to even, up
    bits = R.packs64(ties, torch.bfloat16)[0].reshape(-1)
    assert [int(b) for b in bits] == [0x3F80, 0x3F82, 0x3F81]


def test_zoo_values_are_what_the_tests_rely_on():
    """not N(0, 1): all four scales occur for each operand, zeros in the gradients, and tensors whose decay term carries the update"""
    for col in (1, 2, 3):
        assert {z[col] for z in R.ZOO} == {0, 1, 2, 3}
    carried = 0
    for k, shape in enumerate(R.SHAPES):
        p, g = V.p[k].astype(np.float64), V.g[k].astype(np.float64)
        if p.size >= 8:
            assert (g == 0).any() and (g != 0).any(), shape
        carried += bool(np.median(np.abs(WD * p)) > 30 * np.median(np.abs(C * g[g != 0])))
    assert carried >= 2, carried
