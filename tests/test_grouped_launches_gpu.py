"""Every grouped launch (csrc/group.h: up to FS_MAX_GROUP = 12 problems of one kernel in one launch) against fp64 references, problem by
problem and element by element.

The grouped kernels are reached through the public ABI with hand-built command lists (tests/_grouped_cases.py): JOIN runs through
fs_exec_program (program.hip run_pool) and k one-command programs through fs_exec_program_group (run_same_op, the deferred weight-gradient
sink).  Every group is heterogeneous - map sizes, channel tails, strides, dtypes, kernel routes - so a wrong block prefix, local grid
size or problem order shows up in the one problem it hits.  Tolerances are those of the single-launch test of the same kernel
(tests/test_kernels_gpu.py, test_bn_group_gpu.py, test_conv_unit_gpu.py).  Every output is a channel slice of a wider buffer between
pixel margins: the slice starts as NaN (or, for accumulated outputs, a random base) and must come back finite, the surroundings must
come back untouched.  The launch census (level 2) proves which kernels ran: the grouped one with the expected launch count, the
single-problem one only for a lone 13th problem or a bucket of one.

The library reads the grouped convolution's tile choice, problem order and cost model (FS_IGEMM2_GROUP_CFG / _LPT / _MODEL) and the grouped
weight gradient's block budget (FS_WGRAD_GROUP_BLOCKS) once, at load, and FS_GROUP_BN_MIXED at first use: those run in a fresh child process
per setting."""
import os
import subprocess
import sys

import pytest
import torch

from tests import _grouped_cases as G

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", G.DTYPES, ids=["f32", "bf16"])
SIZE = pytest.mark.parametrize("n", G.SIZES)
ROUTE = pytest.mark.parametrize("route", ["join", "programs"])


def P():
    from fasterseg_amd import program
    return program


def group_and_single(kernels, family, n, what):
    """n problems of one dtype: one grouped launch of min(n, 12) problems, and a single-problem launch for the 13th"""
    want = {family + "_group_kernel": 1}
    if n > 12:
        want[family + "_kernel"] = 1
    assert G.only(kernels, [family]) == want, (what, kernels)


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------
@DT
@SIZE
@ROUTE
def test_grouped_convolutions(dtype, n, route):
    """OP_CONV_FWD (conv_igemm2_group_kernel): 3x3 / 1x1, stride 1 / 2, pad -1, stride-2 data gradients by parity class, channel tails, a
    BatchNorm-statistics epilogue with scale / shift / ReLU, a two-segment filter bank; K from 16 to 3456 in one launch."""
    ps = G.conv_problems(dtype, n)
    kernels = G.recorded(lambda: G.run(route, P().OP_CONV_FWD, [p.args() for p in ps]))
    G.conv_census_ok(kernels, n)
    for i, p in enumerate(ps):
        p.verify("conv problem %d of %d (%s %s)" % (i, n, p.kind, p.spec["geom"]))


def test_grouped_convolutions_in_bit_reproducible_mode():
    """kernels.deterministic() promises per-problem launches for the weight gradients only: conv_igemm2.hip never consults the mode, so
    a JOIN run of convolutions stays ONE grouped launch with the same results.  The accumulators are plain stores except the affine
    problem's BatchNorm-statistics epilogue, which adds (sum, sumsq) with float atomics in either mode - within the bars below, not
    bit-reproducible; the conv -> BatchNorm units keep their promise by taking the separate statistics pass in this mode (units.hip)."""
    from fasterseg_amd import kernels as K
    ps = G.conv_problems(torch.float32, 12)
    with K.deterministic():
        kernels = G.recorded(lambda: G.run_joined(P().OP_CONV_FWD, [p.args() for p in ps]))
    G.conv_census_ok(kernels, 12)
    for i, p in enumerate(ps):
        p.verify("deterministic conv problem %d (%s %s)" % (i, p.kind, p.spec["geom"]))


# ---- weight gradients ----------------------------------------------------------------------------------------------------------------------
WGRAD_MODES = [(torch.float32, 1), (torch.float32, 0), (torch.bfloat16, 1)]


@pytest.fixture
def fp32_split(request):
    from fasterseg_amd import _lib
    _lib.lib().fs_set_fp32_split(request.param)
    yield request.param
    _lib.lib().fs_set_fp32_split(1)


@pytest.mark.parametrize("dtype,fp32_split", WGRAD_MODES, ids=["f32-split", "f32-mfma", "bf16"], indirect=["fp32_split"])
@SIZE
def test_grouped_weight_gradients(dtype, fp32_split, n):
    """OP_WGRAD_STRIDED JOIN runs (wgrad_group_kernel): taps 1 / 9, stride 1 / 2, pad -1, full and narrow tiles, 96 .. 6039 pixels (ragged
    last slabs), strided operands, [O][R][S][I] and [O][I][R][S] gradient views, a fused pair (n_seg / g_jump), two problems accumulating
    into one gradient tensor; every gradient starts from a random base."""
    s = G.wgrad_set(dtype, n)
    kernels = G.recorded(lambda: G.run_joined(P().OP_WGRAD_STRIDED, [p.args() for p in s.problems]))
    group_and_single(kernels, "wgrad", n, "wgrad")
    s.verify("wgrad group of %d" % n)


@pytest.mark.parametrize("dtype,fp32_split", WGRAD_MODES, ids=["f32-split", "f32-mfma", "bf16"], indirect=["fp32_split"])
def test_deferred_weight_gradient_sink(dtype, fp32_split):
    """25 weight gradients in 5 programs through fs_exec_program_group: collected in the sink, sorted by work, issued as 12 + 12 + 1."""
    s = G.WgradSet(dtype, [i % len(G.WGRAD_TABLE) for i in range(25)], seed0=3000)
    args = [p.args() for p in s.problems]
    kernels = G.recorded(lambda: G.run_programs(P().OP_WGRAD_STRIDED, [args[5 * k:5 * k + 5] for k in range(5)]))
    assert G.only(kernels, ["wgrad"]) == {"wgrad_group_kernel": 2, "wgrad_kernel": 1}, kernels
    s.verify("deferred wgrad sink")


@pytest.mark.parametrize("route", ["join", "programs"])
def test_weight_gradients_in_bit_reproducible_mode(route):
    """kernels.deterministic(): no grouped weight gradient and no deferral - one ordered-slab launch per problem, same results."""
    from fasterseg_amd import kernels as K
    s = G.wgrad_set(torch.float32, 12)
    with K.deterministic():
        kernels = G.recorded(lambda: G.run(route, P().OP_WGRAD_STRIDED, [p.args() for p in s.problems]))
    assert G.only(kernels, ["wgrad"]) == {"wgrad_kernel": 12}, kernels
    s.verify("deterministic wgrad (%s)" % route)


# ---- BatchNorm units -------------------------------------------------------------------------------------------------------------------------
@SIZE
def test_grouped_batchnorm_units(n):
    """OP_BN_UNIT_FWD / _BWD over k programs: column kernels (96 .. 512 pixels per group; 4 groups through the generic kernel), grid-wide
    passes (513, 3072), 1 / 2 / 4 batch groups, ReLU on / off, fp32 and bf16 problems in ONE call, with and without dgamma / dbeta
    accumulators; running statistics after the groups' sequential updates.  The forward runs twice: on exactly summable operands, held per
    element to tests/_bounds.bn_fwd (y, the four blocks of `saved`, the running statistics), and on the normal operands at the older bars,
    whose y and `saved` the backward then reads."""
    ps = G.bn_problems(n)
    op = P()
    if n == 13:          # the expectation itself: the full table must reach every grouped BatchNorm kernel of the default routing
        assert G.bn_expected(ps, False) == {"bn_group_fwd_group_kernel": 2, "bn_fwd_mixed_group_kernel": 2, "bn_train_apply_group_kernel": 2,
                                            "chan_reduce_kernel": 1, "bn_train_apply_kernel": 1}
        assert G.bn_expected(ps, True) == {"bn_group_bwd_group_kernel": 2, "bn_bwd_mixed_group_kernel": 2, "bn_bwd_apply_group_kernel": 2,
                                           "chan_reduce_kernel": 1, "bn_bwd_apply_kernel": 1}
    grid = G.bn_problems(n, "grid")          # the same table on exactly summable operands: the forward per element (tests/_bounds.bn_fwd)
    kernels = G.recorded(lambda: G.run_programs(op.OP_BN_UNIT_FWD, [[p.fwd_args()] for p in grid]))
    assert G.only(kernels, G.BN_KERNELS) == G.bn_expected(grid, False), kernels
    for i, p in enumerate(grid):
        p.verify_fwd("bn fwd problem %d of %d %s" % (i, n, G.BN_TABLE[i]))
    kernels = G.recorded(lambda: G.run_programs(op.OP_BN_UNIT_FWD, [[p.fwd_args()] for p in ps]))
    assert G.only(kernels, G.BN_KERNELS) == G.bn_expected(ps, False), kernels
    for i, p in enumerate(ps):
        p.verify_fwd("bn fwd problem %d of %d %s" % (i, n, G.BN_TABLE[i]))
    kernels = G.recorded(lambda: G.run_programs(op.OP_BN_UNIT_BWD, [[p.bwd_args()] for p in ps]))
    assert G.only(kernels, G.BN_KERNELS) == G.bn_expected(ps, True), kernels
    for i, p in enumerate(ps):
        p.verify_bwd("bn bwd problem %d of %d %s" % (i, n, G.BN_TABLE[i]))


# ---- conv -> BatchNorm -> ReLU units -----------------------------------------------------------------------------------------------------------
@DT
@pytest.mark.parametrize("n", G.UNIT_SIZES)
def test_grouped_conv_bn_units(dtype, n):
    """OP_UNIT_FWD / _BWD over k programs: units on both sides of units.hip's stats_in_epilogue, stride 1 / 2, with and without dx - one
    call mixes `stats_ready` normalisations, statistics passes and column kernels in the mixed BatchNorm launches; the weight gradients
    leave through the deferred sink, the data gradients as one grouped convolution."""
    ps = G.unit_problems(dtype, n)
    assert {p.mode for p in ps} == ({0, 2} if n == 2 else {0, 1, 2})
    op = P()
    names = list(G.BN_KERNELS) + ["wgrad", "conv_igemm2", "conv_igemm"]
    kernels = G.recorded(lambda: G.run_programs(op.OP_UNIT_FWD, [[p.fwd_args()] for p in ps]))
    assert G.only(kernels, names) == G.unit_expected(ps, False), kernels
    for i, p in enumerate(ps):
        p.verify_fwd("unit fwd problem %d of %d %s" % (i, n, G.UNIT_TABLE[i]))
    kernels = G.recorded(lambda: G.run_programs(op.OP_UNIT_BWD, [[p.bwd_args()] for p in ps]))
    assert G.only(kernels, names) == G.unit_expected(ps, True), kernels
    for i, p in enumerate(ps):
        p.verify_bwd("unit bwd problem %d of %d %s" % (i, n, G.UNIT_TABLE[i]))


# ---- bilinear resamples -----------------------------------------------------------------------------------------------------------------------
@DT
@SIZE
@ROUTE
def test_grouped_bilinear(dtype, n, route):
    """OP_BILINEAR_FWD / _BWD: x2 up, 1/2 down, odd sizes (15x21 <-> 29x41), identity, ReLU on / off, strided maps."""
    ps = G.resize_problems(dtype, n)
    op = P()
    kernels = G.recorded(lambda: G.run(route, op.OP_BILINEAR_FWD, [p.fwd_args() for p in ps]))
    group_and_single(kernels, "bilinear_fwd", n, "bilinear fwd")
    for i, p in enumerate(ps):
        p.verify_fwd("bilinear fwd problem %d of %d %s" % (i, n, G.RESIZE_TABLE[i]))
    kernels = G.recorded(lambda: G.run(route, op.OP_BILINEAR_BWD, [p.bwd_args() for p in ps]))
    group_and_single(kernels, "bilinear_bwd", n, "bilinear bwd")
    for i, p in enumerate(ps):
        p.verify_bwd("bilinear bwd problem %d of %d %s" % (i, n, G.RESIZE_TABLE[i]))


# ---- weighted sums, axpy -------------------------------------------------------------------------------------------------------------------------
@DT
@SIZE
@ROUTE
def test_grouped_weighted_sums(dtype, n, route):
    """OP_WSUM / OP_WSUM_BWD / OP_WSUM_DOTS: 1, 2, 5 and 8 operands of different channel strides, 35 .. 3072 pixels, 8 .. 384 channels; null
    operands of the backward stay unwritten, the dot products accumulate onto a random base."""
    ps = G.wsum_problems(dtype, n)
    op = P()
    for opcode, family, args, verify in ((op.OP_WSUM, "wsum", "wsum_args", "verify_wsum"), (op.OP_WSUM_BWD, "wsum_bwd", "bwd_args", "verify_bwd"),
                                         (op.OP_WSUM_DOTS, "wsum_dot", "dots_args", "verify_dots")):
        kernels = G.recorded(lambda: G.run(route, opcode, [getattr(p, args)() for p in ps]))
        group_and_single(kernels, family, n, family)
        for i, p in enumerate(ps):
            getattr(p, verify)("%s problem %d of %d %s" % (family, i, n, G.WSUM_TABLE[i]))


@ROUTE
def test_grouped_axpy_buckets(route):
    """OP_AXPY, 12 calls at once: overwrite / accumulate and fp32 / bf16 mixed - four buckets (for_each_bucket), one grouped launch each."""
    ps = [G.AxpyProblem(s, 2500 + 10 * i) for i, s in enumerate(G.AXPY_TABLE)]
    kernels = G.recorded(lambda: G.run(route, P().OP_AXPY, [p.args() for p in ps]))
    assert G.only(kernels, ["ew"]) == {"ew_group_kernel": 4}, kernels
    for i, p in enumerate(ps):
        p.verify("axpy problem %d %s" % (i, G.AXPY_TABLE[i]))


# ---- settings the library reads at load: one fresh child process per setting -----------------------------------------------------------------
def run_child(table, env):
    full = dict(os.environ)
    full.update(env)
    r = subprocess.run([sys.executable, "-m", "tests._grouped_cases", table], env=full, cwd=G.ROOT, timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "%s under %s: exit status %d\n%s" % (table, env, r.returncode, r.stdout[-6000:])
    assert r.stdout.rstrip().endswith("ok"), r.stdout[-2000:]


@pytest.mark.parametrize("env", [{"FS_IGEMM2_GROUP_CFG": "0"}, {"FS_IGEMM2_GROUP_CFG": "4"}, {"FS_IGEMM2_GROUP_CFG": "5"},
                                 {"FS_IGEMM2_GROUP_CFG": "6"}, {"FS_IGEMM2_GROUP_LPT": "0"}, {"FS_IGEMM2_GROUP_MODEL": "0"}],
                         ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_grouped_convolutions_forced_configurations(env):
    """every tile configuration of the grouped convolution (64x64, 32x32 K4, 64x32 K2, 32x64 K2), caller order instead of longest-first,
    and the fewest-staged-bytes choice: the whole convolution table, both dtypes, groups of 2 / 12 / 13"""
    run_child("conv", env)


@pytest.mark.parametrize("blocks", ["64", "4096"])
def test_grouped_weight_gradients_block_budget(blocks):
    """FS_WGRAD_GROUP_BLOCKS 64 (every problem at the 64-block floor: long slabs) and 4096 (short slabs down to the 256-pixel minimum)"""
    run_child("wgrad", {"FS_WGRAD_GROUP_BLOCKS": blocks})


def test_grouped_batchnorm_units_without_mixed_launches():
    """FS_GROUP_BN_MIXED=0: the BatchNorm table through chan_reduce_group_kernel, the grouped register-resident column kernels and the
    grouped normalisation / input-gradient passes (the default routing folds the first two into the mixed launches)"""
    run_child("bn", {"FS_GROUP_BN_MIXED": "0"})
