"""The per-element bounds of the train-mode BatchNorm forward (tests/_bounds.py, third section), checked on the CPU: they pass an honest
kernel and fail a subtly wrong one.  Companion of tests/test_bwd_bounds_selfcheck.py, for fp32 and bf16.

The "kernel" is an fp32 emulation of the arithmetic of csrc/bn_bodies.h in torch: s1 = sum z and s2 = sum z * z (the product rounded
before it is added) in a summation order that is not the fp64 reference's, m = s1 / n, var = max(s2 / n - m * m, 0),
invstd = 1 / sqrt(var + eps), scale = gamma * invstd, shift = beta - m * gamma * invstd, y = z * scale + shift, ReLU from a first
channel on, one store in the storage type, and the running statistics updated group after group.  Two orders: serial, and a random
permutation of the pixels dealt to 64 lanes whose partial sums meet in a halving tree.

Shapes G x n = 1x105, 2x512, 3x96, 2x1536, 1x2048 (C = 16, ReLU from channel 8 on), both operand families of B.bn_fwd_operands.
The honest emulation must lie within every bound at every element, in both families (the grid family with exact_sums=True, where the
bound has no term in n).  Planted defects, each of which must put at least one element above some bound at every shape of the grid
family:
   1. the last pixel of every group is missing from the sums;
   2. the last pixel of group g is counted in group g + 1 (shapes with more than one group);
   3. no eps under the square root (the constant channel: inf);
   4. running_var without count / (count - 1);
   5. the bf16 store truncates (bf16 only);
   6. ReLU applied to the channels below relu_from too;
   7. shift without beta;
   8. the running statistics take one update for all the groups (shapes with more than one group);
   9. no eps where y is formed, the saved statistics right (the per-element form of the normalisation pass derives its own invstd).
Defects 2 and 8 do not exist with one group, so the one-group shapes have no case for them.  Each defect test also prints (pytest -s)
what the older bars of tests/test_bn_group_gpu.py make of the defect on the operands they were set for, the normal family: which
outputs they flag, NONE where the defect passes them.  DESIGN.md records the outcome."""
import pytest
import torch

from tests import _bounds as B

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SHAPES = [(1, 105), (2, 512), (3, 96), (2, 1536), (1, 2048)]
C, RELU_FROM = 16, 8
ORDERS = ["serial", "lanes"]
DEFECTS = ["lost_last_pixel", "pixel_in_next_group", "no_eps", "no_unbiased", "truncating_store", "relu_below_first", "shift_without_beta",
           "one_running_update", "no_eps_in_y"]
NEEDS_GROUPS = ("pixel_in_next_group", "one_running_update")

_cache = {}


def case(dtype, shape, family):
    key = (dtype, shape, family)
    if key not in _cache:
        G, n = shape
        ops = B.bn_fwd_operands(dtype, G, n, C, 800 + n, family)
        _cache[key] = (ops, B.bn_fwd(dtype, *ops, RELU_FROM, family == "grid"))
    return _cache[key]


def sums(v, order, seed):
    """fp32 sum over dim 1 of (G, n, C) in the given order"""
    G, n, _ = v.shape
    if order == "serial":
        s = torch.zeros(G, v.shape[2])
        for p in range(n):
            s = s + v[:, p]
        return s
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    v = v[:, perm]
    pad = -n % 64
    v = torch.cat([v, torch.zeros(G, pad, v.shape[2])], 1).view(G, -1, 64, v.shape[2])     # [step][lane]
    lanes = torch.zeros(G, 64, v.shape[3])
    for t in range(v.shape[1]):
        lanes = lanes + v[:, t]
    w = 64
    while w > 1:
        w //= 2
        lanes = lanes[:, :w] + lanes[:, w:2 * w]
    return lanes[:, 0]


def truncate_bf16(v32):
    return (v32.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def emulate(dtype, ops, order, defect=None):
    z, gamma, beta, rm, rv = (t.float() for t in ops)
    G, n, _ = z.shape
    eps, mom = torch.tensor(B.BN_EPS, dtype=torch.float32), torch.tensor(B.BN_MOMENTUM, dtype=torch.float32)
    zs = z
    if defect == "lost_last_pixel":
        zs = z[:, :n - 1]
    if defect == "pixel_in_next_group":
        assert G > 1
        zs = z.clone()
        zs[1, 0] = z[0, n - 1]
        zs[0, n - 1] = z[1, 0]
    s1, s2 = sums(zs, order, 1), sums(zs * zs, order, 2)
    count = torch.tensor(float(n), dtype=torch.float32)
    m = s1 / count
    var = (s2 / count - m * m).clamp(min=0.0)
    is_ = 1.0 / torch.sqrt(var if defect == "no_eps" else var + eps)
    scale = gamma * is_
    shift = -(m * gamma * is_) if defect == "shift_without_beta" else beta - m * gamma * is_
    if defect == "no_eps_in_y":
        sc = gamma * (1.0 / torch.sqrt(var))
        y = z * sc[:, None] + (beta - m * sc)[:, None]
    else:
        y = z * scale[:, None] + shift[:, None]
    first = 0 if defect == "relu_below_first" else RELU_FROM
    y = torch.cat([y[..., :first], torch.fmax(y[..., first:], torch.zeros(()))], -1)          # fmaxf: a NaN comes out as 0
    y = truncate_bf16(y) if defect == "truncating_store" else y.to(dtype)
    one = torch.tensor(1.0, dtype=torch.float32)
    for g in range(1 if defect == "one_running_update" else G):
        rm = (one - mom) * rm + mom * m[g]
        unbiased = var[g] if defect == "no_unbiased" or n == 1 else var[g] * (count / (count - one))
        rv = (one - mom) * rv + mom * unbiased
    return dict(mean=m, invstd=is_, scale=scale, shift=shift, y=y, rm=rm, rv=rv)


def above(want, got):
    """outputs with at least one element above the bound (or not finite)"""
    out = []
    for k in B.BN_FWD_OUTPUTS:
        err = (got[k].double().reshape(want[k].shape) - want[k]).abs()
        if not bool((err <= want[k + "_bound"]).all()):
            out.append("%s (worst err / bound %.3g)" % (k, float((err / want[k + "_bound"]).nan_to_num(nan=float("inf")).max())))
    return out


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("family", ["grid", "normal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_honest_forward_is_within_every_bound(dtype, shape, family, order):
    ops, want = case(dtype, shape, family)
    got = emulate(dtype, ops, order)
    B.bn_fwd_check(want, got, "honest BN forward %dx%d %s %s %s" % (shape + (family, order, dtype)))
    if family == "grid":                         # what the family is for: the sums are exact whatever the order
        z = ops[0].float()
        assert torch.equal(torch.cat([sums(z, order, 1), sums(z * z, order, 2)], 1).double(), want["stats"])
    else:                                        # the older bars were set on this family; on the grid family the cancellation in
        assert B.bn_old_bars(dtype, got, want) == []          # E[z^2] - m^2 of channel 1 is beyond them, and inside the bound


def test_grid_sums_are_exact_only_while_the_assertion_holds():
    """4400 pixels at |j| <= 64 let sum j^2 of channel 1 (j = 63 or 64) pass 2^24: refused; at |j| <= 32 they are accepted"""
    with pytest.raises(AssertionError):
        B.bn_fwd_operands(torch.float32, 1, 4400, 8, 1, "grid")
    B.bn_fwd_operands(torch.float32, 1, 4400, 8, 1, "grid", jmax=32)
    with pytest.raises(AssertionError):
        B.bn_fwd_operands(torch.float32, 1, 2049, 8, 1, "normal")


# a defect between groups does not exist with one group (module docstring); an fp32 value is stored as it is
DEFECT_CASES = [(dt, s, d) for dt in DTYPES for s in SHAPES for d in DEFECTS
                if not (d in NEEDS_GROUPS and s[0] == 1) and not (d == "truncating_store" and dt != torch.bfloat16)]


@pytest.mark.parametrize("dtype,shape,defect", DEFECT_CASES, ids=["%s-%dx%d-%s" % (IDS[DTYPES.index(dt)], s[0], s[1], d) for dt, s, d in DEFECT_CASES])
def test_defect_is_above_some_bound(dtype, shape, defect):
    """asserted on the grid family; printed for the record: what the older bars make of the same defect on THEIR operands, the normal
    family (on the grid family the honest cancellation of channel 1 already trips them), and whether the n-rounding bound sees it there"""
    name = "%-20s %dx%-5d %-5s" % (defect, shape[0], shape[1], IDS[DTYPES.index(dtype)])
    ops, want = case(dtype, shape, "grid")
    for order in ORDERS:
        out = above(want, emulate(dtype, ops, order, defect))
        print("%s %-6s grid:   above the bound: %s" % (name, order, ", ".join(out) or "-"))
        assert out, defect
    ops, want = case(dtype, shape, "normal")
    got = emulate(dtype, ops, "lanes", defect)
    print("%s lanes  normal: above the bound: %s | flagged by the old bars: %s"
          % (name, ", ".join(above(want, got)) or "-", ", ".join(B.bn_old_bars(dtype, got, want)) or "NONE"))
