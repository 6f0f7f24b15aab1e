"""Problem builders, fp64 references and hand-built command lists for the grouped launches (csrc/group.h).

Every problem owns its operands and outputs on the device and its reference on the CPU: plain PyTorch in fp64 on operands rounded to
the storage dtype (F.conv2d / F.batch_norm(training=True) / F.interpolate(align_corners=True) and their autograd, explicit sums for
the weighted sums and the axpy).  Outputs live in a channel slice of a wider buffer with a margin of pixels before and after it: the
slice starts as NaN (overwritten outputs) or as a random base (accumulated outputs), everything around it holds a sentinel that must
survive the launch.  `run_joined` / `run_programs` send hand-built command lists (program._List) through fs_exec_program (JOIN runs) and
fs_exec_program_group (k one-command programs); argument layouts are the emit(...) calls of fasterseg_amd/program.py.

`python -m tests._grouped_cases conv|wgrad|bn` runs the convolution / weight-gradient / BatchNorm tables in this process (the library
reads FS_IGEMM2_GROUP_*, FS_WGRAD_GROUP_BLOCKS and FS_GROUP_BN_MIXED once, at load or first use), prints one line per problem and exits
non-zero at the first failure."""
import ctypes
import os
import sys
from collections import Counter

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SENTINEL = 7.25          # exact in bf16 and fp32
MARGIN = 3               # pixels of sentinel before and after every map
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
SIZES = [2, 12, 13]
DEVICE = "cuda"


def vec_of(dtype):
    return 4 if dtype == F32 else 8


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def q(t, dtype):
    """round to the storage dtype, back in fp64"""
    return t.to(dtype).to(torch.float64)


def to_pix(x):
    """(N, C, H, W) -> (N*H*W, C), the NHWC pixel order of the kernels"""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def check(got, want, dtype, what):
    """tests/test_kernels_gpu.check, returning the largest error (the bar every convolution / resample / weighted-sum test asserts)"""
    from tests.test_kernels_gpu import check as bar
    assert bool(torch.isfinite(got).all()), "%s: %d elements of the output slice are not finite (never written?)" % (
        what, int((~torch.isfinite(got)).sum()))
    bar(got, want, dtype, what)
    return float((got.double() - want.double()).abs().max())


class Slab:
    """A (pixels, C) map as the channel slice [c0, c0 + C) of a (MARGIN + pixels + MARGIN, cs) buffer filled with SENTINEL."""

    def __init__(self, pixels, C, dtype, cs=None, c0=0, data=None, fill=None):
        v = vec_of(dtype)
        cs = cs or (C + v - 1) // v * v
        assert cs % v == 0 and c0 % v == 0 and c0 + C <= cs
        self.pixels, self.C, self.cs, self.c0, self.dtype = pixels, C, cs, c0, dtype
        self.buf = torch.full((pixels + 2 * MARGIN, cs), SENTINEL, dtype=dtype, device=DEVICE)
        self.view = self.buf[MARGIN:MARGIN + pixels, c0:c0 + C]
        if data is not None:
            assert tuple(data.shape) == (pixels, C), (tuple(data.shape), pixels, C)
            self.view.copy_(data.to(dtype))
        elif fill is not None:
            self.view.fill_(fill)
        assert self.view.data_ptr() % 16 == 0

    @property
    def ref(self):
        from fasterseg_amd.program import ABS, Ref
        return Ref(ABS, self.view.data_ptr())

    def read(self):
        return self.view.double().cpu()

    def assert_surroundings(self, what):
        mask = torch.ones(self.buf.shape, dtype=torch.bool, device=DEVICE)
        mask[MARGIN:MARGIN + self.pixels, self.c0:self.c0 + self.C] = False
        bad = int((self.buf[mask] != SENTINEL).sum())
        assert bad == 0, "%s: %d margin / padding elements around the slice were overwritten" % (what, bad)


class FVec:
    """n floats between two 4-float sentinel margins"""

    def __init__(self, n, data=None, fill=None, dtype=torch.float32):
        self.n = n
        pad = 4 if dtype == torch.float32 else 2         # 16 bytes either way
        self.pad = pad
        self.buf = torch.full((n + 2 * pad,), 7, dtype=dtype, device=DEVICE) if dtype == torch.int64 else \
            torch.full((n + 2 * pad,), SENTINEL, dtype=dtype, device=DEVICE)
        self.view = self.buf[pad:pad + n]
        if data is not None:
            self.view.copy_(data.reshape(-1).to(dtype))
        elif fill is not None:
            self.view.fill_(fill)

    @property
    def ref(self):
        from fasterseg_amd.program import ABS, Ref
        return Ref(ABS, self.view.data_ptr())

    def read(self):
        return self.view.double().cpu()

    def assert_surroundings(self, what):
        want = 7 if self.buf.dtype == torch.int64 else SENTINEL
        edge = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        assert bool((edge == want).all()), "%s: the floats around the vector were overwritten" % what


def dev(t, dtype):
    """a plain device operand (filter packs, coefficients)"""
    return t.to(dtype).contiguous().to(DEVICE)


def absolute(t):
    from fasterseg_amd.program import absolute as a
    return a(t)


def workspace():
    from fasterseg_amd import kernels as K
    from fasterseg_amd.program import ABS, Ref
    ptr, nbytes = K.stream_workspace("cuda")
    return Ref(ABS, ptr), nbytes


# ---------------------------------------------------------------------------------------------------
# the two routes into the grouped code
# ---------------------------------------------------------------------------------------------------
def _zero_slots(k=1):
    from fasterseg_amd.program import N_SLOTS
    return (ctypes.c_void_p * (k * N_SLOTS))()


def run_joined(op, commands):
    """fs_exec_program on ONE list: every command but the last carries the JOIN bit (program.hip run_pool)."""
    from fasterseg_amd import kernels as K
    from fasterseg_amd.program import N_SLOTS, ZF, _List
    lst = _List(ZF)
    for i, args in enumerate(commands):
        lst.emit(op, *args, join=i + 1 < len(commands))
    words, n, blob, _ = lst.finish()
    K.call("fs_exec_program", K._stream(), words, n, blob, _zero_slots(), N_SLOTS)


def run_programs(op, programs):
    """fs_exec_program_group on k programs; programs[i] is the list of (unjoined) commands of program i (program.hip run_same_op)."""
    from fasterseg_amd import kernels as K
    from fasterseg_amd.program import MAX_GROUP, N_SLOTS, ZF, _List
    k = len(programs)
    assert 1 <= k <= MAX_GROUP
    lists = []
    for commands in programs:
        lst = _List(ZF)
        for args in commands:
            lst.emit(op, *args)
        lists.append(lst.finish())
    words = (ctypes.c_void_p * k)(*[ctypes.addressof(w) for w, _, _, _ in lists])
    counts = (ctypes.c_longlong * k)(*[n for _, n, _, _ in lists])
    blobs = (ctypes.c_void_p * k)(*[ctypes.addressof(b) for _, _, b, _ in lists])
    K.call("fs_exec_program_group", K._stream(), k, words, counts, blobs, _zero_slots(k), N_SLOTS)


def run(route, op, commands):
    if route == "join":
        run_joined(op, commands)
    else:
        run_programs(op, [[c] for c in commands])


def recorded(fn):
    """kernel name -> launches of fn() (census level 2: every FS_LAUNCH by name)"""
    from fasterseg_amd import census
    with census.recording(level=2) as rec:
        fn()
        torch.cuda.synchronize()
    return {name: count for name, (count, _) in rec.kernels.items()}


def launches(kernels, *names):
    return sum(kernels.get(n, 0) for n in names)


def chunks(items, n=12):
    """program.hip hands the commands of one kind to the grouped entry points FS_MAX_GROUP at a time, in order"""
    return [items[i:i + n] for i in range(0, len(items), n)]


# ---------------------------------------------------------------------------------------------------
# convolutions (OP_CONV_FWD)
# ---------------------------------------------------------------------------------------------------
def ref_conv(x, w, stride, pad):
    if pad < 0:
        return F.conv2d(x[:, :, -pad:, -pad:], w, None, stride, 0)
    return F.conv2d(x, w, None, stride, pad)


def out_hw(H, W, k, stride, pad):
    if pad < 0:          # FactorizedReduce's second branch convolves x[:, :, 1:, 1:] (fs_conv_desc.pad = -1)
        return (H + pad - k) // stride + 1, (W + pad - k) // stride + 1
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


# geom = (N, Cin, H, W, Cout, k, stride, pad) of the FORWARD convolution; kind: plain | affine (BN-statistics epilogue + scale / shift /
# ReLU) | dgrad (its stride-2 data gradient, FS_CONV_TRANSPOSED) | twoseg (two filter banks as one GEMM, n_seg / n_jump); pad_to: channel
# stride of the output buffer; K = k*k*Cin runs from 16 to 3456 inside every group of 2, 12 and 13
CONV_TABLE = [
    dict(geom=(1, 32, 32, 48, 40, 3, 1, 1), kind="affine", y_cs=48, c0=8),
    dict(geom=(2, 16, 8, 12, 48, 1, 2, -1), y_cs=96, c0=48),                 # FactorizedReduce conv_2: second channel half of a wider map
    dict(geom=(2, 64, 9, 13, 96, 3, 2, 1), x_cs=80),
    dict(geom=(1, 128, 8, 8, 19, 1, 1, 0), y_cs=32),                         # classifier: 19 channels in a 32-padded buffer
    dict(geom=(1, 48, 9, 13, 32, 3, 2, 1), kind="dgrad"),                    # odd map: the four parity classes differ in size
    dict(geom=(2, 96, 8, 12, 48, 1, 2, 0), y_cs=96, c0=0),
    dict(geom=(1, 16, 20, 18, 144, 3, 1, 1)),
    dict(geom=(3, 384, 4, 8, 384, 3, 1, 1)),
    dict(geom=(2, 40, 12, 16, 96, 3, 1, 1), kind="twoseg", bank=(96, 64)),   # 2 x 48 output channels out of two [96][3][3][64] banks
    dict(geom=(1, 256, 4, 8, 256, 3, 1, 1)),
    dict(geom=(1, 64, 7, 9, 40, 1, 2, -1), kind="dgrad", y_cs=80, c0=16),
    dict(geom=(2, 48, 12, 10, 80, 3, 1, 1), y_cs=96, c0=8),
    dict(geom=(1, 32, 16, 24, 32, 3, 1, 1)),
]


class ConvProblem:
    def __init__(self, spec, dtype, seed):
        from fasterseg_amd import kernels as K
        from fasterseg_amd._lib import ConvDesc
        self.spec, self.dtype, self.kind = spec, dtype, spec.get("kind", "plain")
        N, Cin, H, W, Cout, k, stride, pad = spec["geom"]
        Ho, Wo = out_hw(H, W, k, stride, pad)
        dt = K.dtype_code(dtype)
        self.stats_ref = None
        self.scale = self.shift = None
        if self.kind == "dgrad":
            w = q(rnd(Cout, Cin, k, k, seed=seed + 1, scale=0.2), dtype)
            dy = q(rnd(N, Cout, Ho, Wo, seed=seed + 2), dtype)
            x0 = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
            ref_conv(x0, w, stride, pad).backward(dy)
            self.want = to_pix(x0.grad)
            self.x = Slab(N * Ho * Wo, Cout, dtype, cs=spec.get("x_cs"), data=to_pix(dy))
            self.w = dev(w.flip(2, 3).permute(1, 2, 3, 0), dtype)                    # [Cin][R][S][Cout], rotated by 180 degrees
            self.out_shape = (N * H * W, Cin)
            self.desc = ConvDesc(N, Ho, Wo, Cout, Cin, k, k, 1, k - 1 - pad, H, W, self.x.cs, 0, dt, K.FS_CONV_TRANSPOSED)
        else:
            x = q(rnd(N, Cin, H, W, seed=seed), dtype)
            self.x = Slab(N * H * W, Cin, dtype, cs=spec.get("x_cs"), data=to_pix(x))
            self.out_shape = (N * Ho * Wo, Cout)
            self.desc = ConvDesc(N, H, W, Cin, Cout, k, k, stride, pad, Ho, Wo, self.x.cs, 0, dt, 0)
            if self.kind == "twoseg":
                O, I = spec["bank"]
                half = Cout // 2
                wa = q(rnd(O, I, k, k, seed=seed + 1, scale=(2.0 / (Cin * k * k)) ** 0.5), dtype)
                wb = q(rnd(O, I, k, k, seed=seed + 2, scale=(2.0 / (Cin * k * k)) ** 0.5), dtype)
                self.w = dev(torch.cat([wa.permute(0, 2, 3, 1).reshape(-1), wb.permute(0, 2, 3, 1).reshape(-1)]), dtype)
                raw = torch.cat([ref_conv(x, wa[:half, :Cin], stride, pad), ref_conv(x, wb[:half, :Cin], stride, pad)], 1)
                self.desc.w_os, self.desc.w_ts, self.desc.n_seg, self.desc.n_jump = k * k * I, I, half, O - half
            else:
                w = q(rnd(Cout, Cin, k, k, seed=seed + 1, scale=(2.0 / (Cin * k * k)) ** 0.5), dtype)
                self.w = dev(w.permute(0, 2, 3, 1), dtype)                             # [Cout][R][S][Cin]
                raw = ref_conv(x, w, stride, pad)
            self.want = to_pix(raw)
            if self.kind == "affine":
                self.desc.flags = K.FS_CONV_RELU
                scale, shift = rnd(Cout, seed=seed + 3).abs().float().double() + 0.5, rnd(Cout, seed=seed + 4).float().double()
                self.scale, self.shift = dev(scale, F32), dev(shift, F32)
                self.want = F.relu(self.want * scale + shift)
                rp = to_pix(raw)
                self.stats_ref = torch.cat([rp.sum(0), (rp * rp).sum(0)])
                self.stats_base = rnd(2 * Cout, seed=seed + 5).float().double()
        self.reset()

    def reset(self):
        pixels, C = self.out_shape
        self.y = Slab(pixels, C, self.dtype, cs=self.spec.get("y_cs"), c0=self.spec.get("c0", 0), fill=float("nan"))
        self.desc.y_cs = self.y.cs
        self.stats = FVec(len(self.stats_ref), data=self.stats_base) if self.stats_ref is not None else None

    def args(self):
        from fasterseg_amd.program import NULL, _Desc
        ws, wsb = workspace()
        return (_Desc(self.desc), self.x.ref, absolute(self.w), absolute(self.scale), absolute(self.shift), self.y.ref,
                self.stats.ref if self.stats else NULL, ws, wsb)

    def verify(self, what):
        err = check(self.y.read(), self.want, self.dtype, what)
        self.y.assert_surroundings(what)
        self.x.assert_surroundings(what + " (input)")
        if self.stats is not None:          # the bars of test_conv2d_fwd for the epilogue's (sum, sumsq)
            C = self.out_shape[1]
            got = self.stats.read() - self.stats_base
            cnt = self.out_shape[0]
            assert torch.allclose(got[:C], self.stats_ref[:C], atol=2e-3 * cnt ** 0.5 + 1e-3, rtol=2e-3), what + ": epilogue sum"
            assert torch.allclose(got[C:], self.stats_ref[C:], atol=1e-3, rtol=3e-3), what + ": epilogue sumsq"
            self.stats.assert_surroundings(what + " (stats)")
        return err


_cache = {}


def cached(kind, dtype, build):
    key = (kind, dtype)
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def conv_problems(dtype, n):
    """the first n problems of the table (operands and references built once per dtype, outputs fresh)"""
    all_ = cached("conv", dtype, lambda: [ConvProblem(s, dtype, 100 + 10 * i) for i, s in enumerate(CONV_TABLE)])
    ps = all_[:n]
    for p in ps:
        p.reset()
    return ps


def conv_census_ok(kernels, n):
    """13 problems of one dtype: one grouped launch of 12 and one single launch"""
    single = launches(kernels, "conv_igemm2_kernel", "conv_igemm_kernel")
    assert kernels.get("conv_igemm2_group_kernel", 0) == 1 and single == (1 if n > 12 else 0), kernels


# ---------------------------------------------------------------------------------------------------
# weight gradients (OP_WGRAD_STRIDED)
# ---------------------------------------------------------------------------------------------------
# geom as above; layout of the gradient tensor the kernel accumulates into: "orsi" = a [O][R][S][I] view, "oirs" = an [O][I][R][S] view,
# both the leading [:Cout, :Cin] block of a (full_o, full_i) tensor; pair: Cout = two segments whose rows land in two adjacent tensors
# (n_seg / g_jump); into: problems naming the same buffer accumulate into ONE gradient tensor.  Tiles of 64 x 64 channels: full (64, 160,
# 384), narrow in one dimension (96 = 64 + 32, 48, 32), narrow in both; M = 96 .. 6039 pixels, mostly no multiple of KC = 64 / 128.
WGRAD_TABLE = [
    dict(geom=(2, 64, 24, 40, 96, 3, 1, 1), layout="orsi", full=(128, 96), dy_cs=128),
    dict(geom=(1, 32, 12, 8, 32, 1, 1, 0), layout="oirs", full=(48, 64)),
    dict(geom=(3, 48, 33, 61, 64, 3, 1, 1), layout="orsi", full=(64, 48), x_cs=64),
    dict(geom=(2, 160, 16, 24, 160, 3, 2, 1), layout="oirs", full=(160, 192)),
    dict(geom=(2, 96, 14, 18, 48, 1, 2, -1), layout="orsi", full=(96, 96), dy_cs=96),
    dict(geom=(2, 96, 14, 18, 48, 1, 2, 0), layout="oirs", full=(48, 96), dy_cs=96),
    dict(geom=(2, 64, 12, 16, 96, 3, 1, 1), layout="orsi", full=(80, 64), pair=True),
    dict(geom=(3, 384, 4, 8, 384, 3, 1, 1), layout="orsi", full=(384, 384)),
    dict(geom=(2, 32, 10, 14, 64, 3, 1, 1), layout="orsi", full=(64, 32), into="shared"),
    dict(geom=(1, 32, 20, 11, 64, 3, 1, 1), layout="orsi", full=(64, 32), into="shared", x_cs=48),
    dict(geom=(1, 96, 32, 48, 32, 3, 2, 1), layout="oirs", full=(32, 96), x_cs=128),
    dict(geom=(2, 48, 9, 13, 160, 1, 1, 0), layout="orsi", full=(160, 48), dy_cs=192),
    dict(geom=(1, 64, 16, 24, 64, 3, 1, 1), layout="oirs", full=(96, 64)),
]


class GradBuffer:
    """A gradient tensor (random base) that one or more problems accumulate into, and the fp64 sum they must add to it."""

    def __init__(self, shape, seed):
        self.base = rnd(*shape, seed=seed).float()
        self.want = torch.zeros(shape, dtype=torch.float64)
        self.mask = torch.zeros(shape, dtype=torch.bool)
        self.mag = torch.zeros(shape, dtype=torch.float64)         # sum over the contributors of sum_m |dy x|
        self.parts = []                                            # per contributor: (its sum_m |dy x| placed like `want`, P likewise, slabs)
        self.who = []
        self.reset()

    def bound(self):
        """tests/_bounds.wgrad_bound per contributor, summed: each problem adds onto the random base and whatever the others left, so its
        `base` is |base| + the others' magnitudes.  The slab count is the most any launch makes of M pixels (the grouped launch asks every
        problem for its share of the blocks: fewer slabs, never more).  #2 of the table contracts 6039 pixels, beyond the 2048 up to which
        the bound resolves a single lost pixel: it is held to the bound all the same (p_max=None), which still is orders of magnitude
        below the tensor-wide bar."""
        from tests import _bounds as B
        total = torch.zeros_like(self.mag)
        for mag, P, S in self.parts:
            total += B.wgrad_bound(mag, P, S, self.base.double().abs() + self.mag - mag, p_max=B.WGRAD_P_MAX if float(P.max()) <= B.WGRAD_P_MAX else None)
        return total

    def reset(self):
        self.dev = self.base.clone().to(DEVICE)

    def verify(self, dtype, what):
        what = "%s (problems %s)" % (what, self.who)
        got = self.dev.cpu()
        assert bool(torch.isfinite(got).all()), what + ": non-finite gradient"
        assert torch.equal(got[~self.mask], self.base[~self.mask]), what + ": elements outside the [:Cout, :Cin] block changed"
        delta = got.double() - self.base.double()
        scale = float(self.want.abs().max())
        tol = 2e-4 * scale + 1e-4 if dtype == F32 else 2e-2 * scale          # test_conv2d_dgrad_and_wgrad
        err = float((delta - self.want)[self.mask].abs().max())
        assert err <= tol, "%s: wgrad max err %.3e vs max|ref| %.3e (tol %.3e)" % (what, err, scale, tol)
        from tests import _bounds as B
        B.assert_within(delta[self.mask], self.want[self.mask], self.bound()[self.mask], what + " per element")
        return err


class WgradProblem:
    def __init__(self, spec, dtype, seed, buffers, tag):
        from fasterseg_amd import kernels as K
        from fasterseg_amd._lib import ConvDesc
        self.spec, self.dtype = spec, dtype
        N, Cin, H, W, Cout, k, stride, pad = spec["geom"]
        Ho, Wo = out_hw(H, W, k, stride, pad)
        x = q(rnd(N, Cin, H, W, seed=seed), dtype)
        dy = q(rnd(N, Cout, Ho, Wo, seed=seed + 1), dtype)
        w0 = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
        ref_conv(x, w0, stride, pad).backward(dy)
        grad = w0.grad                                                           # [Cout][Cin][R][S]
        from tests import _bounds as B
        ref, mag, P = B.wgrad_ref(x, dy, k, stride, pad)
        assert torch.allclose(ref, grad, rtol=1e-12, atol=1e-12)
        P = P.expand_as(mag)
        self.x = Slab(N * H * W, Cin, dtype, cs=spec.get("x_cs"), data=to_pix(x))
        dy_cs = spec.get("dy_cs")
        self.dy = Slab(N * Ho * Wo, Cout, dtype, cs=dy_cs, c0=(dy_cs - Cout) // 8 * 8 if dy_cs else 0, data=to_pix(dy))
        self.desc = ConvDesc(N, H, W, Cin, Cout, k, k, stride, pad, Ho, Wo, self.x.cs, self.dy.cs, K.dtype_code(dtype), 0)
        O, I = spec["full"]
        pair = bool(spec.get("pair"))
        rows = Cout // 2 if pair else Cout
        assert rows <= O and Cin <= I
        orsi = spec["layout"] == "orsi"
        shape = ((2,) if pair else (1,)) + ((O, k, k, I) if orsi else (O, I, k, k))
        name = spec.get("into") or "#%d" % tag
        if name not in buffers:
            buffers[name] = GradBuffer(shape, seed + 2)
        self.buffer = buffers[name]
        assert tuple(self.buffer.base.shape) == shape
        self.buffer.who.append(tag)
        mag_b, P_b = torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
        for t in range(shape[0]):
            g = grad[t * rows:(t + 1) * rows]
            if orsi:
                self.buffer.want[t, :rows, :, :, :Cin] += g.permute(0, 2, 3, 1)
                self.buffer.mask[t, :rows, :, :, :Cin] = True
                mag_b[t, :rows, :, :, :Cin] = mag[t * rows:(t + 1) * rows].permute(0, 2, 3, 1)
                P_b[t, :rows, :, :, :Cin] = P[t * rows:(t + 1) * rows].permute(0, 2, 3, 1)
            else:
                self.buffer.want[t, :rows, :Cin] += g
                self.buffer.mask[t, :rows, :Cin] = True
                mag_b[t, :rows, :Cin] = mag[t * rows:(t + 1) * rows]
                P_b[t, :rows, :Cin] = P[t * rows:(t + 1) * rows]
        self.buffer.mag += mag_b
        self.buffer.parts.append((mag_b, P_b, B.wgrad_max_slabs(N * Ho * Wo)))
        self.strides = (k * k * I, 1, I) if orsi else (I * k * k, k * k, 1)      # elements between O rows, I columns, taps
        if pair:
            self.desc.n_seg, self.desc.g_jump = rows, O - rows

    def args(self):
        from fasterseg_amd.program import _Desc
        ws, wsb = workspace()
        return (_Desc(self.desc), self.x.ref, self.dy.ref, absolute(self.buffer.dev)) + self.strides + (ws, wsb)


class WgradSet:
    def __init__(self, dtype, indices, seed0=500):
        self.dtype = dtype
        self.buffers = {}
        self.all = [WgradProblem(WGRAD_TABLE[t], dtype, seed0 + 10 * i, self.buffers, i) for i, t in enumerate(indices)]
        self.first(len(self.all))

    def first(self, n):
        """the first n problems with fresh gradient tensors (a tensor's contributors are all among them or none is)"""
        self.problems = self.all[:n]
        self.live = [b for b in self.buffers.values() if b.who[0] < n]
        assert all(max(b.who) < n for b in self.live)
        for b in self.buffers.values():
            b.reset()
        return self

    def verify(self, what):
        errs = {}
        for b in self.live:
            errs[",".join("#%d" % i for i in b.who)] = b.verify(self.dtype, what)
        for i, p in enumerate(self.problems):
            p.x.assert_surroundings("%s #%d (x)" % (what, i))
            p.dy.assert_surroundings("%s #%d (dy)" % (what, i))
        return errs


def wgrad_set(dtype, n):
    return cached("wgrad", dtype, lambda: WgradSet(dtype, list(range(len(WGRAD_TABLE))))).first(n)


# ---------------------------------------------------------------------------------------------------
# BatchNorm units (OP_BN_UNIT_FWD / OP_BN_UNIT_BWD)
# ---------------------------------------------------------------------------------------------------
# (pixels per group, groups, C, relu, dtype, accumulate dgamma / dbeta): column kernels up to 512 pixels per group (groups 1 / 2 inside
# the mixed launch, 4 through the "rest" route), grid-wide passes above; both dtypes in one call
BN_TABLE = [
    (96, 1, 384, 0, F32, True),
    (513, 1, 24, 1, F32, False),
    (256, 2, 64, 1, BF16, True),
    (384, 1, 96, 1, F32, False),
    (512, 2, 24, 0, F32, True),
    (3072, 1, 48, 1, BF16, True),
    (96, 4, 32, 1, F32, True),
    (256, 4, 40, 0, F32, False),
    (513, 2, 64, 1, BF16, False),
    (3072, 1, 32, 0, F32, True),
    (384, 4, 48, 0, BF16, True),
    (96, 4, 64, 1, BF16, False),
    (513, 2, 40, 1, F32, True),
]
EPS, MOMENTUM = 1e-5, 0.1


BN_FAMILIES = ["normal", "grid"]


class BnProblem:
    """family "normal": 1.5 N(0, 1) + 0.3, held to the bars of tests/test_bn_group_gpu.py.  family "grid" (tests/_bounds.bn_fwd_operands:
    z = j / 16 with exactly summable values, a constant channel, a channel with a small variance on a large mean, a negative gamma):
    the forward is held to the per-element exact-sum bound of tests/_bounds.bn_fwd instead - y, the four blocks of `saved` and the
    running statistics.  The per-tensor bars were set on the normal family; an honest kernel's cancellation in E[z^2] - m^2 of the
    grid's small-variance channel lies beyond them and inside the bound (tests/test_bn_fwd_bounds_selfcheck.py)."""

    def __init__(self, spec, seed, family="normal"):
        self.ppg, self.G, self.C, self.relu, self.dtype, self.acc = spec
        G, ppg, C, dtype = self.G, self.ppg, self.C, self.dtype
        self.pixels, self.family, self.bound = G * ppg, family, None
        self.dy0 = q(rnd(self.pixels, C, seed=seed + 1), dtype)
        if family == "grid":
            from tests import _bounds as B
            z, gamma, beta, self.rm0, self.rv0 = B.bn_fwd_operands(dtype, G, ppg, C, seed, "grid")
            self.z0 = z.reshape(self.pixels, C)
            self.bound = B.bn_fwd(dtype, z, gamma, beta, self.rm0, self.rv0, 0 if self.relu else None, True, eps=EPS, momentum=MOMENTUM)
        else:
            assert family == "normal", family
            self.z0 = q(rnd(self.pixels, C, seed=seed) * 1.5 + 0.3, dtype)
            gamma, beta = rnd(C, seed=seed + 2).abs().float().double() + 0.5, (rnd(C, seed=seed + 3) * 0.2).float().double()
            self.rm0, self.rv0 = (rnd(C, seed=seed + 4) * 0.1).float().double(), rnd(C, seed=seed + 5).abs().float().double() + 0.5
        self.dg0, self.db0 = rnd(C, seed=seed + 6).float().double(), rnd(C, seed=seed + 7).float().double()
        self.gamma, self.beta = dev(gamma, F32), dev(beta, F32)
        # reference, group after group (what the reference does when it evaluates one module on several inputs in turn)
        zr = self.z0.clone().requires_grad_(True)
        gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        rm, rv = self.rm0.clone(), self.rv0.clone()
        outs, means, invstds = [], [], []
        for g in range(G):
            zs = zr[g * ppg:(g + 1) * ppg].t().unsqueeze(0)                      # (1, C, ppg)
            o = F.batch_norm(zs, rm, rv, gr, br, True, MOMENTUM, EPS)
            outs.append((F.relu(o) if self.relu else o)[0].t())
            means.append(zs.detach().mean((0, 2)))
            invstds.append(1.0 / torch.sqrt(zs.detach().var((0, 2), unbiased=False) + EPS))
        y = torch.cat(outs, 0)
        y.backward(self.dy0)
        self.want = dict(y=y.detach(), dz=zr.grad, dgamma=gr.grad, dbeta=br.grad, rm=rm, rv=rv, mean=torch.stack(means), invstd=torch.stack(invstds))
        v = vec_of(dtype)
        self.z = Slab(self.pixels, C, dtype, cs=C + 2 * v, c0=v, data=self.z0)
        self.dy = Slab(self.pixels, C, dtype, cs=C + v, c0=0, data=self.dy0)
        self.reset()

    def reset(self):
        G, C, dtype = self.G, self.C, self.dtype
        v = vec_of(dtype)
        nan = float("nan")
        self.y = Slab(self.pixels, C, dtype, cs=C + 3 * v, c0=2 * v, fill=nan)
        self.dz = Slab(self.pixels, C, dtype, cs=C + v, c0=v, fill=nan)
        self.saved = FVec(G * 4 * C, fill=nan)
        self.stats = FVec(G * 2 * C, fill=0.0)                                    # zero-initialised accumulators (slot ZF of a real program)
        self.red = FVec((G + 1 if G > 1 else 1) * 2 * C, fill=0.0)
        self.rm, self.rv = FVec(C, data=self.rm0), FVec(C, data=self.rv0)
        self.nbt = FVec(1, fill=5, dtype=torch.int64)
        self.dgacc, self.dbacc = FVec(C, data=self.dg0), FVec(C, data=self.db0)

    def fwd_args(self):
        from fasterseg_amd import kernels as K
        ws, wsb = workspace()
        return (self.pixels, self.C, self.G, self.z.ref, self.z.cs, absolute(self.gamma), absolute(self.beta), float(EPS), float(MOMENTUM),
                self.rm.ref, self.rv.ref, self.nbt.ref, self.stats.ref, self.saved.ref, self.y.ref, self.y.cs, K.dtype_code(self.dtype),
                self.relu, ws, wsb)

    def bwd_args(self):
        from fasterseg_amd import kernels as K
        from fasterseg_amd.program import NULL
        ws, wsb = workspace()
        return (self.pixels, self.C, self.G, self.z.ref, self.z.cs, self.dy.ref, self.dy.cs, self.y.ref, self.y.cs, self.saved.ref,
                absolute(self.gamma), self.red.ref, K.dtype_code(self.dtype), self.relu, self.dz.ref, self.dz.cs,
                self.dgacc.ref if self.acc else NULL, self.dbacc.ref if self.acc else NULL, ws, wsb)

    @property
    def column(self):
        return self.ppg <= 512

    def _bars(self):
        """tests/test_bn_group_gpu.py: the column kernels' bars up to 512 pixels per group, the grid-wide passes' (float atomics) above"""
        from tests.test_bn_group_gpu import _close
        w, col = self.want, self.column
        wide = lambda t: None if col else 5 * float(t.abs().max())
        return _close, dict(dgamma=wide(w["dgamma"]), dbeta=wide(w["dbeta"]), mean=None if col else 5.0,
                            invstd=float(w["invstd"].abs().max()) * (1 if col else 5), rm=None if col else 5.0, rv=None if col else 5.0)

    def verify_fwd(self, what):
        close, s = self._bars()
        w, dtype = self.want, self.dtype
        y = self.y.read()
        assert bool(torch.isfinite(y).all()), what + ": y holds unwritten elements"
        saved = self.saved.read().view(self.G, 4, self.C)
        if self.family == "grid":
            from tests import _bounds as B
            assert bool(torch.isfinite(saved).all()), what + ": saved holds unwritten elements"
            B.bn_fwd_check(self.bound, dict(saved=saved, y=y.view(self.G, self.ppg, self.C), rm=self.rm.read(), rv=self.rv.read()), what + " (grid)")
        else:
            close(y, w["y"], dtype, what + " y")
            assert bool(torch.isfinite(saved[:, :2]).all()), what + ": saved statistics hold unwritten elements"
            close(saved[:, 0], w["mean"], F32, what + " saved mean", scale=s["mean"])
            close(saved[:, 1], w["invstd"], F32, what + " saved invstd", scale=s["invstd"])
            close(self.rm.read(), w["rm"], F32, what + " running_mean after %d sequential updates" % self.G, scale=s["rm"])
            close(self.rv.read(), w["rv"], F32, what + " running_var", scale=s["rv"])
        assert int(self.nbt.view[0]) == 5 + self.G, what + ": num_batches_tracked"
        for t in (self.y, self.z, self.saved, self.rm, self.rv, self.nbt, self.stats):
            t.assert_surroundings(what)
        return float((y - w["y"]).abs().max())

    def verify_bwd(self, what):
        close, s = self._bars()
        w, dtype, C = self.want, self.dtype, self.C
        dz = self.dz.read()
        assert bool(torch.isfinite(dz).all()), what + ": dz holds unwritten elements"
        close(dz, w["dz"], dtype, what + " dz")
        red = self.red.read()
        close(red[C:2 * C], w["dgamma"], dtype, what + " dgamma", scale=s["dgamma"])
        close(red[:C], w["dbeta"], dtype, what + " dbeta", scale=s["dbeta"])
        dg, db = self.dgacc.read() - self.dg0, self.dbacc.read() - self.db0
        if self.acc:
            close(dg, w["dgamma"], dtype, what + " dgamma accumulated", scale=s["dgamma"])
            close(db, w["dbeta"], dtype, what + " dbeta accumulated", scale=s["dbeta"])
        else:
            assert float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0, what + ": accumulators written without being passed"
        for t in (self.dz, self.dy, self.z, self.y, self.red, self.dgacc, self.dbacc, self.saved):
            t.assert_surroundings(what)
        return float((dz - w["dz"]).abs().max())


def bn_problems(n, family="normal"):
    """the first n problems of the table in one operand family (operands and references built once per family, outputs fresh)"""
    all_ = cached("bn", family, lambda: [BnProblem(s, 900 + 10 * i, family) for i, s in enumerate(BN_TABLE)])
    ps = all_[:n]
    for p in ps:
        p.reset()
    return ps


def bn_expected(problems, backward, mixed=True):
    """Launches units.hip's bn_fwd_group / bn_bwd_group must issue for these calls (12 per grouped call, a lone call its own sequence):
    column maps of 1 / 2 groups and the statistics / reduction passes of wide maps share the mixed launch (one per dtype), column maps
    of more groups take the generic column kernel ("rest"), wide maps a second launch; a bucket of one runs the single-problem kernel.
    mixed=False (FS_GROUP_BN_MIXED=0): one launch per (dtype, column-kernel variant), per statistics / reduction pass and per second pass."""
    d = "bwd" if backward else "fwd"
    apply_ = "bn_bwd_apply" if backward else "bn_train_apply"
    exp = Counter()

    def bucket(ps, family):
        if ps:
            exp[family + ("_group_kernel" if len(ps) > 1 else "_kernel")] += 1
    for chunk in chunks(problems):
        if len(chunk) == 1:
            p = chunk[0]
            if p.column:
                exp[("bn_small_%s_kernel" if p.G <= 2 else "bn_group_%s_kernel") % d] += 1
            else:
                exp["chan_reduce_kernel"] += 1
                exp[apply_ + "_kernel"] += 1
            continue
        for dtype in DTYPES:
            ps = [p for p in chunk if p.dtype == dtype]
            wide = [p for p in ps if not p.column]
            bucket([p for p in ps if p.column and p.G > 2], "bn_group_" + d)
            if mixed:
                if [p for p in ps if not (p.column and p.G > 2)]:
                    exp["bn_%s_mixed_group_kernel" % d] += 1
            else:
                bucket([p for p in ps if p.column and p.G == 1], "bn_small_" + d)
                bucket([p for p in ps if p.column and p.G == 2], "bn_small_" + d)
                bucket(wide, "chan_reduce")
            bucket(wide, apply_)
    return dict(exp)


BN_KERNELS = ("bn_small_fwd", "bn_small_bwd", "bn_group_fwd", "bn_group_bwd", "chan_reduce", "bn_train_apply", "bn_bwd_apply", "bn_fwd_mixed",
              "bn_bwd_mixed")


def only(kernels, families):
    names = set()
    for f in families:
        names.update((f + "_kernel", f + "_group_kernel"))
    return {k: v for k, v in kernels.items() if k in names}


# ---------------------------------------------------------------------------------------------------
# conv -> BatchNorm -> [ReLU] units (OP_UNIT_FWD / OP_UNIT_BWD)
# ---------------------------------------------------------------------------------------------------
# (N, Cin, Cout, H, W, k, stride, BatchNorm groups, relu, dx wanted).  Output pixels per group: up to 512 the column kernels (mode 0),
# above them the statistics come out of the convolution's epilogue (mode 2: `stats_ready` normalisations) unless units.hip's
# stats_in_epilogue refuses (#3: 15360 pixels) or a grouped batch's 32-row sub-tiles straddle two groups (#2: 528 pixels per group)
# - those take the statistics pass (mode 1).
UNIT_TABLE = [
    (1, 32, 32, 32, 48, 3, 1, 1, 1, True),          # 1536 px: epilogue
    (2, 64, 48, 16, 24, 3, 2, 1, 1, True),          # 192 px: column kernel
    (2, 16, 32, 24, 22, 3, 1, 2, 0, False),         # 2 x 528 px: statistics pass
    (1, 16, 32, 96, 160, 3, 1, 1, 0, True),         # 15360 px: statistics pass
    (2, 48, 96, 32, 48, 1, 2, 1, 1, True),          # 1x1 stride 2, 768 px: epilogue
    (4, 32, 64, 16, 32, 3, 1, 2, 1, True),          # 2 x 1024 px: per-group epilogue statistics
    (3, 96, 96, 8, 16, 3, 1, 1, 1, False),          # 384 px: column
    (2, 32, 48, 24, 40, 3, 2, 1, 0, True),          # 480 px: column
    (4, 24, 40, 8, 16, 3, 1, 4, 1, True),           # 4 x 128 px: generic column kernel ("rest")
    (1, 64, 64, 24, 36, 3, 1, 1, 1, True),          # 864 px: epilogue
    (2, 32, 32, 20, 28, 1, 1, 1, 0, False),         # 1x1, 1120 px: epilogue
    (2, 40, 56, 18, 30, 3, 2, 2, 1, True),          # 2 x 135 px: column, two groups
]
UNIT_SIZES = [2, 5, 12]


def stats_in_epilogue(M, C, dtype):
    """units.hip: the conv epilogue keeps the statistics while its same-address atomics cost less than a pass over z.  A restatement
    (with UnitProblem.mode) of the library's routing, used only to predict launch counts; units.hip points back here - a retuned rule
    changes both, and UNIT_TABLE must keep units on either side of it (test_grouped_conv_bn_units asserts the modes it reaches)"""
    return M / 32 * 0.02 <= 8.0 + M * C * (4 if dtype == F32 else 2) / 3.0e6


class UnitProblem:
    def __init__(self, spec, dtype, seed, layout):
        from fasterseg_amd import kernels as K
        from fasterseg_amd._lib import ConvDesc
        N, cin, cout, H, W, k, stride, G, relu, self.want_dx = spec
        # bf16 is compared without the ReLU, as in tests/test_conv_unit_gpu.py: z is stored rounded, so outputs within a rounding of zero
        # flip their mask against the reference - a property of the storage type (the rectified bf16 path is pinned by the BatchNorm units)
        relu = relu if dtype == F32 else 0
        self.spec, self.dtype, self.G, self.C, self.relu = spec, dtype, G, cout, relu
        pad = k // 2
        Ho, Wo = out_hw(H, W, k, stride, pad)
        self.ppg = N // G * Ho * Wo
        self.mode = 0 if self.ppg <= 512 else (1 if (G > 1 and self.ppg % 32 != 0) or not stats_in_epilogue(self.ppg, cout, dtype) else 2)
        x = q(rnd(N, cin, H, W, seed=seed), dtype)
        w = q(rnd(cout, cin, k, k, seed=seed + 1, scale=(2.0 / (cin * k * k)) ** 0.5), dtype)
        gamma, beta = rnd(cout, seed=seed + 2).abs().float().double() + 0.5, (rnd(cout, seed=seed + 3) * 0.2).float().double()
        self.rm0, self.rv0 = (rnd(cout, seed=seed + 4) * 0.1).float().double(), rnd(cout, seed=seed + 5).abs().float().double() + 0.5
        self.dg0, self.db0 = rnd(cout, seed=seed + 6).float().double(), rnd(cout, seed=seed + 7).float().double()
        xr, wr, gr, br = (t.clone().requires_grad_(True) for t in (x, w, gamma, beta))
        rm, rv = self.rm0.clone(), self.rv0.clone()
        zc = F.conv2d(xr, wr, None, stride, pad)
        zc.retain_grad()
        ng = N // G
        y = torch.cat([F.batch_norm(zc[g * ng:(g + 1) * ng], rm, rv, gr, br, True, MOMENTUM, EPS) for g in range(G)], 0)
        y = F.relu(y) if relu else y
        dy = q(rnd(*y.shape, seed=seed + 8), dtype)
        y.backward(dy)
        zg = zc.detach().reshape(G, ng, cout, Ho * Wo)
        self.want = dict(z=to_pix(zc.detach()), y=to_pix(y.detach()), rm=rm, rv=rv, dx=to_pix(xr.grad), dgamma=gr.grad, dbeta=br.grad,
                         dz=to_pix(zc.grad), mean=zg.mean((1, 3)), invstd=1.0 / torch.sqrt(zg.var((1, 3), unbiased=False) + EPS))
        v = vec_of(dtype)
        self.px_in, self.px_out, self.cin = N * H * W, N * Ho * Wo, cin
        self.x = Slab(self.px_in, cin, dtype, cs=cin + v, c0=v, data=to_pix(x))
        self.dy = Slab(self.px_out, cout, dtype, cs=cout + v, c0=0, data=to_pix(dy))
        self.w = dev(w.permute(0, 2, 3, 1), dtype)
        self.w_flip = dev(w.flip(2, 3).permute(1, 2, 3, 0), dtype)
        self.gamma, self.beta = dev(gamma, F32), dev(beta, F32)
        self.desc = ConvDesc(N, H, W, cin, cout, k, k, stride, pad, Ho, Wo, self.x.cs, cout + 2 * v, K.dtype_code(dtype),
                             K.FS_CONV_RELU if relu else 0)
        self.desc.bn_groups = G
        # the weight gradient accumulates into the leading block of a wider tensor, [O][R][S][I] or [O][I][R][S]
        O, I = cout + 16, cin + 8
        orsi = layout == "orsi"
        self.grad = GradBuffer((1,) + ((O, k, k, I) if orsi else (O, I, k, k)), seed + 9)
        if orsi:
            self.grad.want[0, :cout, :, :, :cin] = wr.grad.permute(0, 2, 3, 1)
            self.grad.mask[0, :cout, :, :, :cin] = True
        else:
            self.grad.want[0, :cout, :cin] = wr.grad
            self.grad.mask[0, :cout, :cin] = True
        self.strides = (k * k * I, 1, I) if orsi else (I * k * k, k * k, 1)
        self.reset()

    def reset(self):
        G, C, dtype = self.G, self.C, self.dtype
        v = vec_of(dtype)
        nan = float("nan")
        self.z = Slab(self.px_out, C, dtype, cs=C + 2 * v, c0=v, fill=nan)
        self.y = Slab(self.px_out, C, dtype, cs=C + 2 * v, c0=0, fill=nan)
        self.dz = Slab(self.px_out, C, dtype, cs=C, fill=nan)                      # dense: the unit's dz has channel stride Cout
        self.dx = Slab(self.px_in, self.cin, dtype, cs=self.cin + 2 * v, c0=v, fill=nan)
        self.saved = FVec(G * 4 * C, fill=nan)
        self.stats = FVec(G * 2 * C, fill=0.0)
        self.red = FVec((G + 1 if G > 1 else 1) * 2 * C, fill=0.0)
        self.rm, self.rv = FVec(C, data=self.rm0), FVec(C, data=self.rv0)
        self.nbt = FVec(1, fill=5, dtype=torch.int64)
        self.dgacc, self.dbacc = FVec(C, data=self.dg0), FVec(C, data=self.db0)
        self.grad.reset()
        self.grad.who = ["unit"]

    def fwd_args(self):
        from fasterseg_amd.program import _Desc
        ws, wsb = workspace()
        return (_Desc(self.desc), self.x.ref, absolute(self.w), absolute(self.gamma), absolute(self.beta), self.rm.ref, self.rv.ref, self.nbt.ref,
                float(EPS), float(MOMENTUM), self.stats.ref, self.saved.ref, self.z.ref, self.y.ref, ws, wsb)

    def bwd_args(self):
        from fasterseg_amd.program import NULL, _Desc
        ws, wsb = workspace()
        dx = self.want_dx
        return (_Desc(self.desc), self.x.ref, absolute(self.w_flip) if dx else NULL, self.z.ref, self.y.ref if self.relu else NULL, self.dy.ref,
                self.dy.cs, self.saved.ref, absolute(self.gamma), self.red.ref, self.dgacc.ref, self.dbacc.ref, self.dz.ref,
                absolute(self.grad.dev)) + self.strides + (self.dx.ref if dx else NULL, self.dx.cs if dx else self.cin, 0, 0, ws, wsb)

    def _close(self, got, want, what, scale=None):
        """tests/test_conv_unit_gpu.py: 2e-4 (fp32) / 3e-2 (bf16) of max|ref| (running statistics: of 1)"""
        assert bool(torch.isfinite(got).all()), what + ": unwritten or non-finite elements"
        s = float(want.abs().max()) if scale is None else scale
        err = float((got - want).abs().max())
        tol = 2e-4 if self.dtype == F32 else 3e-2
        assert err <= tol * max(s, 1e-6), "%s: max err %.3e, max|ref| %.3e" % (what, err, s)
        return err

    def verify_fwd(self, what):
        w = self.want
        check(self.z.read(), w["z"], self.dtype, what + " z")
        err = self._close(self.y.read(), w["y"], what + " y")
        self._close(self.rm.read(), w["rm"], what + " running_mean", scale=1.0)
        self._close(self.rv.read(), w["rv"], what + " running_var", scale=1.0)
        # saved (mean, invstd) per group: the mean at the running mean's bar (of 1), the inverse deviation of its own maximum
        saved = self.saved.read().view(self.G, 4, self.C)
        self._close(saved[:, 0], w["mean"], what + " saved mean", scale=1.0)
        self._close(saved[:, 1], w["invstd"], what + " saved invstd")
        assert int(self.nbt.view[0]) == 5 + self.G, what + ": num_batches_tracked"
        for t in (self.z, self.y, self.x, self.saved, self.rm, self.rv, self.nbt, self.stats):
            t.assert_surroundings(what)
        return err

    def verify_bwd(self, what):
        w, C = self.want, self.C
        red = self.red.read()
        self._close(red[C:2 * C], w["dgamma"], what + " dgamma")
        self._close(red[:C], w["dbeta"], what + " dbeta")
        self._close(self.dgacc.read() - self.dg0, w["dgamma"], what + " dgamma accumulated")
        self._close(self.dbacc.read() - self.db0, w["dbeta"], what + " dbeta accumulated")
        err = self._close(self.dz.read(), w["dz"], what + " dz")
        if self.want_dx:
            err = max(err, self._close(self.dx.read(), w["dx"], what + " dx"))
        else:
            assert bool(torch.isnan(self.dx.read()).all()), what + ": dx was written although its pointer is null"
        got = self.grad.dev.cpu()
        assert torch.equal(got[~self.grad.mask], self.grad.base[~self.grad.mask]), what + ": weight gradient outside the [:Cout, :Cin] block changed"
        self._close((got.double() - self.grad.base.double())[self.grad.mask], self.grad.want[self.grad.mask], what + " dw")
        for t in (self.dz, self.dx, self.dy, self.red, self.dgacc, self.dbacc, self.z, self.y):
            t.assert_surroundings(what)
        return err


def unit_problems(dtype, n):
    all_ = cached("unit", dtype, lambda: [UnitProblem(s, dtype, 2100 + 20 * i, "orsi" if i % 2 == 0 else "oirs") for i, s in enumerate(UNIT_TABLE)])
    ps = all_[:n]
    for p in ps:
        p.reset()
    return ps


def unit_expected(ps, backward):
    """One grouped convolution (forward: the convolutions, backward: the data gradients), one deferred grouped weight gradient, and the
    BatchNorm launches of bn_fwd_group / bn_bwd_group over units in modes 0 (column), 1 (statistics pass) and 2 (statistics ready)."""
    exp = Counter()
    rest = [p for p in ps if p.mode == 0 and p.G > 2]
    if rest:
        exp[("bn_group_%s_group_kernel" if len(rest) > 1 else "bn_group_%s_kernel") % ("bwd" if backward else "fwd")] += 1
    if backward:
        wide = [p for p in ps if p.mode != 0]
        exp["bn_bwd_mixed_group_kernel"] += 1
        if wide:
            exp["bn_bwd_apply_group_kernel" if len(wide) > 1 else "bn_bwd_apply_kernel"] += 1
        exp["wgrad_group_kernel"] += 1
        if sum(p.want_dx for p in ps) > 1:
            exp["conv_igemm2_group_kernel"] += 1
    else:
        second = [p for p in ps if p.mode == 1]
        exp["conv_igemm2_group_kernel"] += 1
        exp["bn_fwd_mixed_group_kernel"] += 1
        if second:
            exp["bn_train_apply_group_kernel" if len(second) > 1 else "bn_train_apply_kernel"] += 1
    return dict(exp)


# ---------------------------------------------------------------------------------------------------
# bilinear resamples (OP_BILINEAR_FWD / OP_BILINEAR_BWD)
# ---------------------------------------------------------------------------------------------------
# (N, C, Hi, Wi), (Ho, Wo), relu
RESIZE_TABLE = [
    ((2, 32, 9, 12), (18, 24), 1),
    ((1, 64, 16, 32), (8, 16), 0),
    ((1, 16, 15, 21), (29, 41), 1),
    ((2, 24, 29, 41), (15, 21), 0),
    ((1, 40, 7, 14), (3, 7), 1),
    ((1, 8, 4, 8), (32, 64), 0),
    ((1, 24, 5, 5), (5, 5), 1),
    ((3, 48, 8, 12), (16, 24), 1),
    ((1, 96, 12, 16), (6, 8), 0),
    ((2, 8, 17, 23), (33, 45), 1),
    ((1, 384, 4, 8), (8, 16), 0),
    ((1, 32, 3, 7), (7, 14), 1),
    ((1, 16, 10, 10), (20, 20), 0),
]


class ResizeProblem:
    def __init__(self, spec, dtype, seed):
        from fasterseg_amd import kernels as K
        from fasterseg_amd._lib import ResizeDesc
        (N, C, Hi, Wi), (Ho, Wo), relu = spec
        self.dtype, self.relu, self.C = dtype, relu, C
        v = vec_of(dtype)
        x = q(rnd(N, C, Hi, Wi, seed=seed), dtype).requires_grad_(True)
        y = F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=True)
        yr = F.relu(y) if relu else y
        dy = q(rnd(N, C, Ho, Wo, seed=seed + 1), dtype)
        yr.backward(dy)
        self.want_y, self.want_dx = to_pix(yr.detach()), to_pix(x.grad)
        self.px_in, self.px_out = N * Hi * Wi, N * Ho * Wo
        self.x = Slab(self.px_in, C, dtype, cs=C + v, c0=v, data=to_pix(x.detach()))
        self.dy = Slab(self.px_out, C, dtype, cs=C + 2 * v, c0=v, data=to_pix(dy))
        # the backward's ReLU mask is the stored forward output: the reference's, rounded to the storage dtype, in a buffer of dy's stride
        self.y_out = Slab(self.px_out, C, dtype, cs=C + 2 * v, c0=0, data=self.want_y)
        self.fwd_desc = lambda y_cs: ResizeDesc(N, Hi, Wi, Ho, Wo, C, self.x.cs, y_cs, K.dtype_code(dtype), relu, 0)
        self.bwd_desc = lambda dx_cs: ResizeDesc(N, Hi, Wi, Ho, Wo, C, dx_cs, self.dy.cs, K.dtype_code(dtype), relu, 0)
        self.reset()

    def reset(self):
        v = vec_of(self.dtype)
        self.y = Slab(self.px_out, self.C, self.dtype, cs=self.C + 3 * v, c0=v, fill=float("nan"))
        self.dx = Slab(self.px_in, self.C, self.dtype, cs=self.C + 2 * v, c0=2 * v, fill=float("nan"))

    def fwd_args(self):
        from fasterseg_amd.program import _Desc
        return (_Desc(self.fwd_desc(self.y.cs)), self.x.ref, self.y.ref)

    def bwd_args(self):
        from fasterseg_amd.program import NULL, _Desc
        return (_Desc(self.bwd_desc(self.dx.cs)), self.dy.ref, self.y_out.ref if self.relu else NULL, self.dx.ref)

    def verify_fwd(self, what):
        err = check(self.y.read(), self.want_y, self.dtype, what)
        self.y.assert_surroundings(what)
        self.x.assert_surroundings(what + " (x)")
        return err

    def verify_bwd(self, what):
        err = check(self.dx.read(), self.want_dx, self.dtype, what)
        for t in (self.dx, self.dy, self.y_out):
            t.assert_surroundings(what)
        return err


def resize_problems(dtype, n):
    all_ = cached("resize", dtype, lambda: [ResizeProblem(s, dtype, 1300 + 10 * i) for i, s in enumerate(RESIZE_TABLE)])
    ps = all_[:n]
    for p in ps:
        p.reset()
    return ps


# ---------------------------------------------------------------------------------------------------
# weighted sums (OP_WSUM / OP_WSUM_BWD / OP_WSUM_DOTS) and axpy (OP_AXPY)
# ---------------------------------------------------------------------------------------------------
# (pixels, C, operands)
WSUM_TABLE = [(35, 8, 1), (3072, 48, 5), (105, 384, 2), (768, 96, 8), (315, 40, 5), (1536, 24, 2), (96, 64, 8), (2000, 16, 1), (35, 192, 5),
              (513, 32, 2), (3072, 8, 8), (63, 72, 5), (260, 56, 2)]


class WsumProblem:
    def __init__(self, spec, dtype, seed):
        self.pixels, self.C, self.n = spec
        self.dtype = dtype
        P, C, n = spec
        v = vec_of(dtype)
        xs = [q(rnd(P, C, seed=seed + i), dtype) for i in range(n)]
        coef = (rnd(n, seed=seed + 8) * 0.5).float().double()
        self.dy0 = q(rnd(P, C, seed=seed + 9), dtype)
        self.coef = dev(coef, F32)
        self.want_out = sum(c * x for c, x in zip(coef, xs))
        self.want_dx = [c * self.dy0 for c in coef]
        self.want_dots = torch.stack([(self.dy0 * x).sum() for x in xs])
        self.dots_scale = float(self.dy0.pow(2).sum().sqrt()) * max(float(x.pow(2).sum().sqrt()) for x in xs)
        self.dots_base = rnd(8, seed=seed + 10).float().double()
        # operands with different channel strides and offsets
        self.xs = [Slab(P, C, dtype, cs=C + (i % 3) * v, c0=(i % 3) * v, data=x) for i, x in enumerate(xs)]
        self.dy = Slab(P, C, dtype, cs=C + v, c0=v, data=self.dy0)
        self.need = [i % 3 != 1 for i in range(n)]                               # fs_weighted_sum_bwd skips null operands
        self.reset()

    def reset(self):
        v = vec_of(self.dtype)
        nan = float("nan")
        self.out = Slab(self.pixels, self.C, self.dtype, cs=self.C + 2 * v, c0=v, fill=nan)
        self.dxs = [Slab(self.pixels, self.C, self.dtype, cs=self.C + (1 + i % 2) * v, c0=(i % 2) * v, fill=nan) for i in range(self.n)]
        self.dots = FVec(8, data=self.dots_base)

    def _arrays(self, slabs, need=None):
        return [s.ref if need is None or need[i] else None for i, s in enumerate(slabs)], [s.cs for s in slabs]

    def wsum_args(self):
        from fasterseg_amd import kernels as K
        ptrs, cs = self._arrays(self.xs)
        return (self.pixels, self.C, self.n, ptrs, cs, absolute(self.coef), self.out.ref, self.out.cs, K.dtype_code(self.dtype))

    def bwd_args(self):
        from fasterseg_amd import kernels as K
        ptrs, cs = self._arrays(self.dxs, self.need)
        return (self.pixels, self.C, self.n, self.dy.ref, self.dy.cs, absolute(self.coef), ptrs, cs, K.dtype_code(self.dtype))

    def dots_args(self):
        from fasterseg_amd import kernels as K
        ptrs, cs = self._arrays(self.xs)
        return (self.pixels, self.C, self.n, self.dy.ref, self.dy.cs, ptrs, cs, K.dtype_code(self.dtype), self.dots.ref)

    def verify_wsum(self, what):
        err = check(self.out.read(), self.want_out, self.dtype, what)
        for t in [self.out] + self.xs:
            t.assert_surroundings(what)
        return err

    def verify_bwd(self, what):
        err = 0.0
        for i, s in enumerate(self.dxs):
            if self.need[i]:
                err = max(err, check(s.read(), self.want_dx[i], self.dtype, "%s dx%d" % (what, i)))
            else:
                assert bool(torch.isnan(s.read()).all()), "%s: dx%d was written although its pointer is null" % (what, i)
            s.assert_surroundings(what)
        self.dy.assert_surroundings(what)
        return err

    def verify_dots(self, what):
        got = self.dots.read() - self.dots_base
        assert bool(torch.isfinite(got).all()), what
        err = float((got[:self.n] - self.want_dots).abs().max())
        assert err < 1e-4 * self.dots_scale + 1e-3, "%s: dots max err %.3e (scale %.3e)" % (what, err, self.dots_scale)     # test_weighted_sum_fwd_bwd_dots
        assert float(got[self.n:].abs().max()) == 0.0 if self.n < 8 else True, what + ": dots beyond the operand count changed"
        self.dots.assert_surroundings(what)
        return err


def wsum_problems(dtype, n):
    all_ = cached("wsum", dtype, lambda: [WsumProblem(s, dtype, 1700 + 20 * i) for i, s in enumerate(WSUM_TABLE)])
    ps = all_[:n]
    for p in ps:
        p.reset()
    return ps


# (pixels, C, dtype, accumulate): overwrite / accumulate and fp32 / bf16 mixed in ONE call - four buckets of three
AXPY_TABLE = [(126, 40, F32, 0), (35, 8, BF16, 1), (3072, 48, F32, 1), (513, 24, BF16, 0), (96, 384, F32, 0), (2000, 16, F32, 1),
              (768, 96, BF16, 1), (63, 72, BF16, 0), (260, 56, F32, 1), (1536, 32, BF16, 0), (105, 64, F32, 0), (315, 40, BF16, 1)]


class AxpyProblem:
    def __init__(self, spec, seed):
        self.pixels, self.C, self.dtype, self.acc = spec
        P, C, dtype, acc = spec
        v = vec_of(dtype)
        x = q(rnd(P, C, seed=seed), dtype)
        self.base = q(rnd(P, C, seed=seed + 1), dtype)
        alpha = float(torch.tensor(0.37 + 0.01 * (seed % 7), dtype=torch.float32))
        self.alpha = torch.full((8,), alpha, dtype=torch.float32, device=DEVICE)
        self.want = (self.base if acc else 0) + alpha * x                        # test_layout_copy_axpy_dot
        self.x = Slab(P, C, dtype, cs=C + v, c0=0, data=x)
        self.y = Slab(P, C, dtype, cs=C + 2 * v, c0=v, data=self.base if acc else None, fill=None if acc else float("nan"))

    def args(self):
        from fasterseg_amd import kernels as K
        return (self.pixels, self.C, self.x.ref, self.x.cs, absolute(self.alpha), self.y.ref, self.y.cs, K.dtype_code(self.dtype), self.acc)

    def verify(self, what):
        err = check(self.y.read(), self.want, self.dtype, what)
        self.y.assert_surroundings(what)
        self.x.assert_surroundings(what + " (x)")
        return err


# ---------------------------------------------------------------------------------------------------
# child-process entry: the convolution / weight-gradient tables under the environment switches the library reads at load
# ---------------------------------------------------------------------------------------------------
def child_conv():
    from fasterseg_amd.program import OP_CONV_FWD
    for dtype in DTYPES:
        for n in SIZES:
            ps = conv_problems(dtype, n)
            kernels = recorded(lambda: run_joined(OP_CONV_FWD, [p.args() for p in ps]))
            conv_census_ok(kernels, n)
            for i, p in enumerate(ps):
                err = p.verify("conv %s group of %d, problem %d %s %s" % (dtype, n, i, p.kind, p.spec["geom"]))
                print("conv %s n=%d #%d %s %s max err %.3e" % (dtype, n, i, p.kind, p.spec["geom"], err), flush=True)


def child_wgrad():
    from fasterseg_amd.program import OP_WGRAD_STRIDED
    for dtype in DTYPES:
        for n in SIZES:
            s = wgrad_set(dtype, n)
            kernels = recorded(lambda: run_joined(OP_WGRAD_STRIDED, [p.args() for p in s.problems]))
            assert kernels.get("wgrad_group_kernel", 0) == 1 and kernels.get("wgrad_kernel", 0) == (1 if n > 12 else 0), kernels
            for who, err in s.verify("wgrad %s group of %d" % (dtype, n)).items():
                print("wgrad %s n=%d problems %s max err %.3e" % (dtype, n, who, err), flush=True)


def child_bn():
    """the BatchNorm units without the mixed launches (FS_GROUP_BN_MIXED=0): chan_reduce_group_kernel and the grouped column kernels"""
    from fasterseg_amd.program import OP_BN_UNIT_BWD, OP_BN_UNIT_FWD
    mixed = os.environ.get("FS_GROUP_BN_MIXED", "1")[:1] != "0"
    for n in SIZES:
        for family in BN_FAMILIES:
            ps = bn_problems(n, family)
            # the backward's bars were set on the normal family, whose forward it follows
            for backward, op in ((False, OP_BN_UNIT_FWD), (True, OP_BN_UNIT_BWD))[:2 if family == "normal" else 1]:
                kernels = recorded(lambda: run_programs(op, [[p.bwd_args() if backward else p.fwd_args()] for p in ps]))
                assert only(kernels, BN_KERNELS) == bn_expected(ps, backward, mixed), (kernels, bn_expected(ps, backward, mixed))
                for i, p in enumerate(ps):
                    what = "bn %s %s n=%d #%d %s" % ("bwd" if backward else "fwd", family, n, i, BN_TABLE[i][:5])
                    err = p.verify_bwd(what) if backward else p.verify_fwd(what)
                    print("%s max err %.3e" % (what, err), flush=True)


if __name__ == "__main__":
    {"conv": child_conv, "wgrad": child_wgrad, "bn": child_bn}[sys.argv[1]]()
    torch.cuda.synchronize()
    print("ok", flush=True)
