"""The train-mode BatchNorm forward on a real MI355X against fp64 references, held to the per-element bounds of tests/_bounds.py (third
section; tests/test_bn_fwd_bounds_selfcheck.py shows on the CPU that these bounds pass an honest kernel and fail a subtly wrong one):
the register-resident body, the generic column body at 256 / 512 / 1024 lanes, the split-K slab sum, the grid-wide pair with float
atomics and with ordered block partials, the ordered reduction's edges, the apply pass with its LDS table and in its per-element form,
the three-launch form, the ReLU tail of a fused pair with its two counters, and the conv -> BatchNorm unit's three routes on a
selection filter.  fp32 and bf16; y, all four blocks of `saved`, both running statistics and num_batches_tracked in every case.

Two operand families (B.bn_fwd_operands): "grid" - z = j / 16, whose sums are exact in fp32 in any order, so the bound has no term in
the pixel count and `stats`, where a route leaves it behind, must EQUAL the fp64 sums - and "normal", the older tests' 1.5 N(0, 1) +
0.3 (at most 2048 pixels per group: the cases beyond run the grid family only).  z and y are channel slices of wider buffers (NaN
around z, a sentinel around y); y and `saved` start as NaN; num_batches_tracked starts at 5 with a second counter and a sentinel word
after it.  Every case asserts by kernel name the body it is there for (fwd_body: the forward twin of test_bwd_bounds_gpu.bn_body).

Worst err / bound observed on one MI355X as B.assert_within printed it, per body, over both families, "statistics" being the four
blocks of `saved` and the running statistics (recorded observations, not thresholds; the bf16 y figure is the store's own half-ulp,
at most 1 by construction; the statistics' 0.3 to 0.5 is the one division in m = s1 / n against its 2^-23 |m|):
    register-resident              fp32: statistics 0.389, y 0.134    bf16: statistics 0.389, y 0.992
    column                         fp32: statistics 0.335, y 0.136    bf16: statistics 0.335, y 0.991
    split-K slabs                  fp32: statistics 0.343, y 0.134    bf16: statistics 0.343, y 0.992
    grid-wide pair, atomics        fp32: statistics 0.348, y 0.111    bf16: statistics 0.334, y 0.956
    grid-wide pair, ordered        fp32: statistics 0.348, y 0.111    bf16: statistics 0.334, y 0.956
    ordered reduction edges        fp32: sums exact on the grid family, 0.022 of the n-rounding bound on the normal one
    apply pass alone               fp32: statistics 0.479, y 0.128    bf16: statistics 0.479, y 0.992
    three launches                 fp32: statistics 0.327, y 0.091    bf16: statistics 0.327, y 0.988
    ReLU tail, two counters        fp32: statistics 0.343, y 0.140    bf16: statistics 0.343, y 0.992
    conv unit, selection filter    fp32: statistics 0.270, y 0.132    bf16: statistics 0.270, y 0.970
    mixed grouped launch, "rest" route and second pass (tests/test_grouped_launches_gpu.py, grid family)
                                   fp32: statistics 0.345, y 0.144    bf16: statistics 0.344, y 0.993
The convolution's z was the exact selection, bit for bit, on every route and in both types; no kernel needed a fix."""
import ctypes

import pytest
import torch

from tests import _bounds as B
from tests.test_bwd_bounds_gpu import BF16, BN_COL_MAX_PIXELS, BNS_MAX_PIXELS, DTYPES, F32, IDS, NAN, SENTINEL, K, recorded, sliced, untouched, vec_of

pytestmark = pytest.mark.gpu

FAMILIES = ["grid", "normal"]
EPS, MOMENTUM = B.BN_EPS, B.BN_MOMENTUM
NBT0, NBT_SENTINEL = 5, 7777
SMALL, COLUMN, GRID = ["bn_small_fwd_kernel"], ["bn_group_fwd_kernel"], ["bn_train_apply_kernel", "chan_reduce_kernel"]
BN_NAMES = ("bn_", "chan_reduce")


def fwd_body(ppg, groups, unit):
    """the kernels fs_bn_act_train_fwd (unit=True) and fs_bn_group_fwd (unit=False) launch (csrc/units.hip, csrc/bn_col.hip)"""
    if unit and ppg > BN_COL_MAX_PIXELS:
        return GRID
    return SMALL if groups in (1, 2) and ppg <= BNS_MAX_PIXELS else COLUMN


def col_lanes(ppg):
    """csrc/bn_col.hip bnc_threads"""
    return 1024 if ppg > 2048 else 512 if ppg > 512 else 256


def reduce_blocks(mg, rpb):
    """csrc/elementwise.hip reduce_blocks: (blocks, pixels per block) of a statistics pass over mg pixels, rpb pixel rows per iteration"""
    iters = -(-mg // rpb)
    blocks = max(1, min(2048, (iters + 3) // 4))
    per = -(-(-(-mg // blocks)) // rpb) * rpb
    return -(-mg // per), per


def reduce_ws_blocks(mg, rpb, C, groups, ws_bytes):
    """csrc/elementwise.hip reduce_ws: the block count after the workspace's cap (room for `room` partial slots, 1024 at most)"""
    blocks, per = reduce_blocks(mg, rpb)
    room = (ws_bytes - K().WS_COUNTER_BYTES) // (4 * 2 * C * groups)
    assert room >= 1
    cap = min(room, 1024)
    if blocks > cap:
        per = -(-(-(-mg // cap)) // rpb) * rpb
        blocks = -(-mg // per)
    return blocks, per


def fvec(n, data=None, fill=None):
    """n floats between two 4-float sentinel margins -> (buffer, view)"""
    buf = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[4:4 + n]
    if data is not None:
        view.copy_(data.reshape(-1).float())
    else:
        view.fill_(fill)
    return buf, view


def margins_ok(buf, what):
    assert bool((buf[:4] == SENTINEL).all()) and bool((buf[-4:] == SENTINEL).all()), what + ": the floats around the vector were overwritten"


def bit_view(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16).cpu()


_refs = {}


def reference(dtype, G, n, C, family, relu, jmax=B.BN_GRID_JMAX, z=None, exact=None, key=None):
    """operands and fp64 reference of a case, computed once.  relu: the kernels' argument (bit 0, first channel from bit 8 on)"""
    k = (dtype, G, n, C, family, relu & ~2, jmax, key)
    if k not in _refs:
        ops = B.bn_fwd_operands(dtype, G, n, C, 1000 + 7 * n + C, family, jmax=jmax)
        if z is not None:
            ops = (z,) + ops[1:]
        relu_from = (relu >> 8) if relu & 1 else None
        _refs[k] = (ops, B.bn_fwd(dtype, *ops, relu_from, family == "grid" if exact is None else exact))
    return _refs[k]


class Case:
    """device buffers of one launch; operands and reference are shared (reference) and never written"""

    def __init__(self, dtype, G, n, C, family, relu=0, jmax=B.BN_GRID_JMAX, z=None, exact=None, key=None, z_garbage=False):
        self.dtype, self.G, self.n, self.C, self.family, self.relu = dtype, G, n, C, family, relu
        self.ops, self.want = reference(dtype, G, n, C, family, relu, jmax, z, exact, key)
        z64, gamma, beta, rm0, rv0 = self.ops
        v = vec_of(dtype)
        self.v = v
        self.zbuf, self.zv = sliced(z64.reshape(G * n, C), dtype, 2 * v, v)
        self.z_bits = bit_view(self.zv)
        if z_garbage:
            self.zv.fill_(123.0)
        self.ybuf = torch.full((G * n, C + 3 * v), SENTINEL, dtype=dtype, device="cuda")
        self.yv = self.ybuf[:, 2 * v:2 * v + C]
        self.yv.fill_(NAN)
        self.gamma, self.beta = gamma.float().cuda(), beta.float().cuda()
        self.saved_buf, self.saved = fvec(G * 4 * C, fill=NAN)
        self.stats_buf, self.stats = fvec(G * 2 * C, fill=0.0)
        self.rm_buf, self.rm = fvec(C, data=rm0)
        self.rv_buf, self.rv = fvec(C, data=rv0)
        self.nbt = torch.tensor([NBT0, NBT0, NBT_SENTINEL], dtype=torch.int64, device="cuda")
        self.what = "BN fwd %d x %d C=%d %s relu=%#x %s" % (G, n, C, family, relu, IDS[DTYPES.index(dtype)])

    def group_fwd(self, partials=None, splits=1):
        """fs_bn_group_fwd, the column kernels called directly"""
        from fasterseg_amd import _lib
        k = K()
        _lib.call("fs_bn_group_fwd", k._stream(), self.G * self.n, self.C, self.G, k._p(self.zv), self.zbuf.shape[1], k._p(partials), splits,
                  k._p(self.gamma), k._p(self.beta), EPS, MOMENTUM, k._p(self.rm), k._p(self.rv), k._p(self.nbt), k._p(self.saved), k._p(self.yv),
                  self.ybuf.shape[1], k.dtype_code(self.dtype), self.relu)

    def act_train_fwd(self, ws):
        """fs_bn_act_train_fwd, the launch sequence chosen by the map size"""
        from fasterseg_amd import _lib
        k = K()
        _lib.call("fs_bn_act_train_fwd", k._stream(), self.G * self.n, self.C, self.G, k._p(self.zv), self.zbuf.shape[1], k._p(self.gamma),
                  k._p(self.beta), EPS, MOMENTUM, k._p(self.rm), k._p(self.rv), k._p(self.nbt), k._p(self.stats), k._p(self.saved), k._p(self.yv),
                  self.ybuf.shape[1], k.dtype_code(self.dtype), self.relu, *ws)

    def check(self, names, body, stats=False, z_kept=True, tag=""):
        what = self.what + tag
        assert sorted(n_ for n_ in names if n_.startswith(BN_NAMES)) == body, (what, names)
        G, n, C, v = self.G, self.n, self.C, self.v
        got = dict(saved=self.saved, y=self.yv.double().cpu().view(G, n, C), rm=self.rm, rv=self.rv)
        B.bn_fwd_check(self.want, got, what)
        if stats and self.family == "grid":
            assert torch.equal(self.stats.double().cpu().view(G, 2 * C), self.want["stats"]), what + ": stats are not the exact sums"
        two = bool(self.relu & 2)
        assert self.nbt.tolist() == [NBT0 + G, NBT0 + G * two, NBT_SENTINEL], (what, self.nbt.tolist())
        if z_kept:
            assert torch.equal(bit_view(self.zv), self.z_bits), what + ": z was written"
        untouched(self.zbuf, v, C, NAN, what + " (z)")
        untouched(self.ybuf, 2 * v, C, SENTINEL, what + " (y)")
        for buf in (self.saved_buf, self.stats_buf, self.rm_buf, self.rv_buf):
            margins_ok(buf, what)
        if self.relu >> 8:                        # the ReLU tail: channels below the first rectified one keep their negative outputs
            first = self.relu >> 8
            lo = self.want["y"][..., :first]
            sure = lo < -self.want["y_bound"][..., :first]
            assert int(sure.sum()) > 0 and bool((got["y"][..., :first][sure] < 0).all()), what + ": outputs below the first rectified channel were rectified"
            assert bool((got["y"][..., first:] >= 0).all()), what


def relu_for(C):
    """C = 8 without ReLU, C = 40 with it on every channel"""
    return 1 if C == 40 else 0


# ---- the register-resident body ----------------------------------------------------------------------------------------------------------
SMALL_CASES = [(1, 2), (1, 105), (1, 256), (2, 257), (1, 512), (2, 512)]          # 105: fewer pixels than lanes; 257: one live lane in slot 2
COLUMN_CASES = [(3, 96, 64), (3, 512, 64), (1, 513, 64), (2, 2049, 64), (1, 4097, 32)]       # 256, 256, 512, 1024 lanes; a second strided trip
COLUMN_LANES = {96: 256, 512: 256, 513: 512, 2049: 1024, 4097: 1024}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", SMALL_CASES, ids=lambda c: "%dx%d" % c)
def test_register_resident_body(case, dtype):
    """bn_small_fwd_body<T, 1 | 2> through fs_bn_group_fwd"""
    G, n = case
    assert fwd_body(n, G, False) == SMALL
    for family in FAMILIES:
        for C in (8, 40):
            c = Case(dtype, G, n, C, family, relu_for(C))
            c.check(recorded(c.group_fwd), SMALL)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", COLUMN_CASES, ids=lambda c: "%dx%d" % c[:2])
def test_column_body(case, dtype):
    """bn_group_fwd_body<T> through fs_bn_group_fwd at 256, 512 and 1024 lanes; 4097 pixels give lane 0 a second trip of the strided loop
    (4 x 1024 pixels per trip) and need |j| <= 32 for exact sums.  Beyond 2048 pixels per group only the grid family runs."""
    G, n, jmax = case
    assert fwd_body(n, G, False) == COLUMN and col_lanes(n) == COLUMN_LANES[n]
    for family in FAMILIES:
        if family == "normal" and n > B.BN_NORMAL_N_MAX:
            continue
        for C in (8, 40):
            c = Case(dtype, G, n, C, family, relu_for(C), jmax=jmax)
            c.check(recorded(c.group_fwd), COLUMN)


# ---- split-K slabs -----------------------------------------------------------------------------------------------------------------------
def slab_sum(parts):
    """fp32 sum in slab order from 0.f, as the kernels add the slabs"""
    acc = torch.zeros(parts.shape[1:], dtype=torch.float32)
    for s in range(parts.shape[0]):
        acc = acc + parts[s]
    return acc


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("slabs", ["random", "grid"])
@pytest.mark.parametrize("case", [(2, 257), (3, 96)], ids=lambda c: "%dx%d" % c)
def test_split_k_slabs(case, slabs, dtype):
    """fs_bn_group_fwd with splits = 3: z starts as garbage and must come back as the round-to-nearest-even of the fp32 sum of the slabs
    taken in slab order from 0.f, bit for bit; the statistics are those of that stored z.  Random fp32 slabs, and grid-valued slabs that
    sum to a grid z (exact sums)."""
    G, n = case
    body = fwd_body(n, G, False)
    assert body == (SMALL if G == 2 else COLUMN)
    S = 3
    for C in (8, 40):
        g = torch.Generator().manual_seed(4000 + n + C)
        if slabs == "grid":
            zg = B.bn_fwd_operands(dtype, G, n, C, 1000 + 7 * n + C, "grid")[0].reshape(G * n, C)
            a = torch.randint(-64, 65, (2, G * n, C), generator=g).double() / B.BN_GRID_DEN
            parts = torch.cat([a, (zg - a[0] - a[1])[None]], 0).float()
            assert bool((parts.double().sum(0) == zg).all())
        else:
            parts = torch.randn(S, G * n, C, generator=g) * 1.5 + 0.1
        acc = slab_sum(parts)
        stored = acc.to(dtype)
        if slabs == "grid":
            assert bool((stored.double() == zg).all())
        c = Case(dtype, G, n, C, "grid" if slabs == "grid" else "normal", relu_for(C), z=stored.double().view(G, n, C), key="slabs", z_garbage=True)
        pd = parts.contiguous().cuda()
        names = recorded(lambda: c.group_fwd(pd, S))
        assert torch.equal(bit_view(c.zv), bit_view(stored)), c.what + ": z is not the rounded slab sum"
        c.check(names, body, z_kept=False, tag=" slabs")


# ---- the grid-wide pair ------------------------------------------------------------------------------------------------------------------
WIDE_CASES = [(F32, 384, 1, 513), (BF16, 40, 2, 600)]


@pytest.mark.parametrize("dtype,C,G,n", WIDE_CASES, ids=["f32-C384-1x513", "bf16-C40-2x600"])
def test_grid_wide_pair(dtype, C, G, n):
    """chan_reduce_body<T, 0> + bn_train_apply_body<T> through fs_bn_act_train_fwd, with float atomics and, inside k.deterministic(), with
    ordered block partials.  fp32 C = 384: 2 pixel rows per iteration, 65 blocks of 8 pixels, the last with one; bf16 C = 40: 51 rows per
    iteration, lane 255 idle, 3 blocks of 204 with a ragged last one.  On the grid family both modes leave the exact sums in `stats`."""
    k = K()
    rpb = 256 // (C // vec_of(dtype))
    assert reduce_blocks(n, rpb) == ((65, 8) if dtype == F32 else (3, 204)) and 256 % (C // vec_of(dtype)) == (64 if dtype == F32 else 1)
    assert fwd_body(n, G, True) == GRID
    for family in FAMILIES:
        a = Case(dtype, G, n, C, family, 1)
        a.check(recorded(lambda: a.act_train_fwd(k.stream_workspace("cuda"))), GRID, stats=True, tag=" atomics")
        d = Case(dtype, G, n, C, family, 1)
        with k.deterministic():
            names = recorded(lambda: d.act_train_fwd(k.stream_workspace("cuda")))
        d.check(names, GRID, stats=True, tag=" ordered")
        if family == "grid":
            assert torch.equal(bit_view(a.stats), bit_view(d.stats))


def stats_bounds(z64):
    """[s1 | s2] of (n, C) and the any-order bounds e1, e2 of B.bn_fwd"""
    n = z64.shape[0]
    ref = torch.cat([z64.sum(0), (z64 * z64).sum(0)])
    return ref, torch.cat([n * B.E32 * z64.abs().sum(0), (n + 1) * B.E32 * (z64 * z64).sum(0)]) + B.TINY


@pytest.mark.parametrize("n,room", [(51, None), (67, None), (131, None), (51, 3)], ids=["7-blocks", "9-blocks", "17-blocks", "room-3"])
def test_ordered_reduction_edges(n, room):
    """fs_channel_stats_ws inside k.deterministic(), fp32 C = 384 (2 pixel rows per iteration, 8 pixels per block): 7, 9 and 17 blocks -
    the finishing block adds eight interleaved row groups, so 7 leaves one empty, 9 and 17 give the first one a second and third slot -
    and a workspace with room for 3 partial slots, which lowers the block count from 7 to 3.  Grid family: the exact sums; normal: n
    roundings.  The arrival counters come back zero, the workspace beyond the slots in use keeps its bytes."""
    from fasterseg_amd import _lib
    k = K()
    C, dtype = 384, F32
    slot = 4 * 2 * C
    ws_bytes = k.WORKSPACE_BYTES if room is None else k.WS_COUNTER_BYTES + room * slot + slot // 2
    blocks, per = reduce_ws_blocks(n, 2, C, 1, ws_bytes)
    if room is None:
        assert (blocks, per) == ({51: 7, 67: 9, 131: 17}[n], 8)
    else:
        assert (blocks, per) == (3, 18) and reduce_blocks(n, 2) == (7, 8)
    for family in FAMILIES:
        z64 = B.bn_fwd_operands(dtype, 1, n, C, 5000 + n, family)[0][0]
        zbuf, zv = sliced(z64, dtype, 8, 4)
        sbuf, stats = fvec(2 * C, fill=NAN)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        ws[:-k.WS_COUNTER_BYTES].fill_(0x7f)
        ws[-k.WS_COUNTER_BYTES:].zero_()
        with k.deterministic():
            names = recorded(lambda: _lib.call("fs_channel_stats_ws", k._stream(), n, C, 1, k._p(zv), zbuf.shape[1], k.dtype_code(dtype), k._p(stats),
                                               k._p(ws), ws_bytes))
        assert [n_ for n_ in names if n_.startswith(BN_NAMES)] == ["chan_reduce_kernel"], names
        what = "ordered statistics %d pixels room=%s %s" % (n, room, family)
        ref, bound = stats_bounds(z64)
        got = stats.double().cpu()
        if family == "grid":
            assert torch.equal(got, ref), what + ": not the exact sums"
        B.assert_within(got, ref, bound, what)
        assert int(ws[-k.WS_COUNTER_BYTES:].view(torch.int32).abs().sum()) == 0, what + ": arrival counters were not left at zero"
        used = ws[:blocks * slot]
        assert bool((used.view(torch.int32) != 0x7f7f7f7f).all()), what + ": a partial slot in use was not written"
        rest = ws[blocks * slot:-k.WS_COUNTER_BYTES]
        assert bool((rest == 0x7f).all()), what + ": the workspace beyond %d partial slots was written" % blocks
        margins_ok(sbuf, what)
        untouched(zbuf, 4, C, NAN, what)


# ---- the apply pass alone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,C,G", [(BF16, 1024, 2), (F32, 768, 3), (BF16, 1024, 3)], ids=["bf16-2x1024-table", "f32-3x768-elementwise", "bf16-3x1024-elementwise"])
def test_apply_pass_table_and_per_element_form(dtype, C, G):
    """fs_channel_stats_g + fs_bn_train_apply_g at (G, 37): groups * C = 2048 is the last size the LDS table of (scale, shift) holds; 2304
    and 3072 take the form that derives both per element.  ReLU from channel 8 on: the constant channel 0 of the grid family, whose
    normalised value hangs on eps alone, is stored as it comes out."""
    from fasterseg_amd import _lib
    k = K()
    n = 37
    for family in FAMILIES:
        c = Case(dtype, G, n, C, family, 1 | (8 << 8))
        dt = k.dtype_code(dtype)

        def launch():
            _lib.call("fs_channel_stats_g", k._stream(), G * n, C, G, k._p(c.zv), c.zbuf.shape[1], dt, k._p(c.stats))
            _lib.call("fs_bn_train_apply_g", k._stream(), G * n, C, G, k._p(c.zv), c.zbuf.shape[1], k._p(c.stats), k._p(c.gamma), k._p(c.beta), EPS,
                      MOMENTUM, k._p(c.rm), k._p(c.rv), k._p(c.nbt), k._p(c.saved), k._p(c.yv), c.ybuf.shape[1], dt, c.relu)
        c.check(recorded(launch), GRID, stats=True, tag=" G*C=%d" % (G * C))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_three_launch_form(dtype):
    """k.channel_stats + k.bn_finalize + k.affine_act on a 1 x 9 x 13 map (117 pixels)"""
    k = K()
    N, H, W = 1, 9, 13
    for family in FAMILIES:
        for C in (8, 40):
            c = Case(dtype, 1, N * H * W, C, family, relu_for(C))
            v = c.v
            x = c.zbuf.view(N, H, W, -1).permute(0, 3, 1, 2)[:, v:v + C]
            y = c.ybuf.view(N, H, W, -1).permute(0, 3, 1, 2)[:, 2 * v:2 * v + C]

            def launch():
                k.channel_stats(x, c.stats)
                mean, invstd, scale, shift = k.bn_finalize(c.stats, N * H * W, c.gamma, c.beta, EPS, MOMENTUM, c.rm, c.rv, c.nbt)
                c.saved.copy_(torch.cat([mean, invstd, scale, shift]))
                k.affine_act(x, scale, shift, bool(c.relu), out=y)
            names = recorded(launch)
            assert sorted(n_ for n_ in names if n_.startswith(BN_NAMES + ("ew_",))) == ["bn_finalize_kernel", "chan_reduce_kernel", "ew_kernel"], names
            c.check([n_ for n_ in names if n_ != "bn_finalize_kernel"], ["chan_reduce_kernel"], stats=True, tag=" three launches")


# ---- the ReLU tail of a fused pair and its two counters ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("G,n,unit", [(2, 257, False), (3, 96, False), (2, 600, True)], ids=["small-2x257", "column-3x96", "grid-wide-2x600"])
def test_relu_tail_and_two_counters(G, n, unit, dtype):
    """relu = 1 | 2 | (16 << 8), C = 40: ReLU from channel 16 on (a multiple of both vector widths inside C), channels below keep their
    negative outputs; bit 1: both adjacent num_batches_tracked counters advance by G, the word after them survives"""
    k = K()
    relu = 1 | 2 | (16 << 8)
    body = fwd_body(n, G, unit)
    assert body == (GRID if unit else SMALL if G == 2 else COLUMN)
    for family in FAMILIES:
        c = Case(dtype, G, n, 40, family, relu)
        names = recorded((lambda: c.act_train_fwd(k.stream_workspace("cuda"))) if unit else c.group_fwd)
        c.check(names, body, stats=unit)


# ---- the conv -> BatchNorm unit on a selection filter ------------------------------------------------------------------------------------
# (N, H, W, BatchNorm groups, bit-reproducible mode) -> pixels per group, the BatchNorm kernels of the route
UNIT_CASES = [((2, 16, 16, 2, False), SMALL), ((3, 8, 12, 3, False), COLUMN), ((1, 32, 32, 1, False), ["bn_train_apply_kernel"]),
              ((2, 20, 32, 2, False), GRID), ((2, 20, 32, 2, True), GRID), ((1, 32, 32, 1, True), GRID)]
UNIT_IDS = ["column-small-2x256", "column-3x96", "epilogue-1x1024", "pass-2x640", "pass-2x640-ordered", "pass-1x1024-ordered"]
SELECT = [1.0, -1.0, 0.5, 2.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case,body", UNIT_CASES, ids=UNIT_IDS)
def test_conv_unit_routes_on_a_selection_filter(case, body, dtype):
    """fs_conv_bn_act_train_fwd, 1x1 convolution, Cin = 8: output channel c takes input channel c % 8 times 1, -1, 0.5 or 2, the input is
    on the grid j / 16 with |j| <= 16.  Any correct contraction gives z exactly (asserted first, bit for bit), on the grid j / 32 with
    |j| <= 64: exact sums.  Then the unit's BatchNorm outputs are held to the exact-sum bound on the column route, with the statistics
    from the conv epilogue, with the separate pass, and with the separate pass in bit-reproducible mode."""
    from fasterseg_amd import _lib
    from fasterseg_amd._lib import ConvDesc
    k = K()
    N, H, W, G, det = case
    P, cin, v = N * H * W, 8, vec_of(dtype)
    n = P // G
    x64 = B.bn_fwd_operands(dtype, 1, P, cin, 6000 + P, "grid", jmax=16)[0][0]            # (P, 8)
    xbuf, xv = sliced(x64, dtype, v, 0)
    for C in (8, 40):
        w = torch.zeros(C, cin, dtype=torch.float64)
        for co in range(C):
            w[co, co % cin] = SELECT[(co // 2) % 4]
        z64 = (x64 @ w.t())
        j = z64 * 32
        assert bool((j == j.round()).all()) and float((j * j).view(G, n, C).sum(1).max()) < 2.0 ** 24
        c = Case(dtype, G, n, C, "grid", 1, z=z64.view(G, n, C), key=("unit", P))
        zbuf = torch.full((P, C + 3 * v), SENTINEL, dtype=dtype, device="cuda")       # the unit's z has y's channel stride: a buffer shaped like y's
        zv = zbuf[:, v:v + C]
        zv.fill_(NAN)
        wd = w.view(C, 1, 1, cin).to(dtype).contiguous().cuda()
        d = ConvDesc(N, H, W, cin, C, 1, 1, 1, 0, H, W, xbuf.shape[1], c.ybuf.shape[1], k.dtype_code(dtype), k.FS_CONV_RELU)
        d.bn_groups = G

        def launch():
            _lib.call("fs_conv_bn_act_train_fwd", k._stream(), ctypes.byref(d), k._p(xv), k._p(wd), k._p(c.gamma), k._p(c.beta), k._p(c.rm), k._p(c.rv),
                      k._p(c.nbt), EPS, MOMENTUM, k._p(c.stats), k._p(c.saved), k._p(zv), k._p(c.yv), *k.stream_workspace("cuda"))
        if det:
            with k.deterministic():
                names = recorded(launch)
        else:
            names = recorded(launch)
        assert any(n_.startswith("conv_") for n_ in names), names
        what = c.what + " unit"
        assert torch.equal(bit_view(zv), bit_view(z64.to(dtype))), what + ": the convolution's z is not the exact selection"
        untouched(zbuf, v, C, SENTINEL, what + " (z)")
        untouched(xbuf, 0, cin, NAN, what + " (x)")
        c.check(names, body, stats=body != SMALL and body != COLUMN, z_kept=False, tag=" unit")
