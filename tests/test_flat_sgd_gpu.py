"""fs_sgd_momentum_multi (csrc/optim.hip sgd_multi_kernel through optim.FlatSGD) against the fp64 reference and per-element bound of
tests/_sgd_ref.py, on a zoo of parameters placed on the kernel's own tile and chunk edges (tests/test_sgd_layout.py shows on the CPU
that each lands on its branch).

All parameters are views into ONE fp32 buffer with 64 sentinel elements around each; gradient, momentum and pack buffers are dense, so
an overrun lands in a neighbour.  WHOLE buffers are compared: the parameter buffer (guards included), sync.flat (never written),
opt.momentum_buf, opt.pack_fwd, opt.pack_flip.  Every step is checked from the device's own state: p, m, g are read back before the
launch, step64 runs on those exact values, so one step's bound holds at every step.  The packs are compared bit for bit with the
rounding of the parameters the device stored.  A tensor the step must not touch has bound 0: its bits must not move.

tests/test_sgd_ref_selfcheck.py shows on the CPU, on the same operands, that these comparisons bite.  Which mutant each test stands
against:
  test_kernel_arithmetic            wd_after_blend, nesterov, dampening, no_momentum (momentum and parameter buffers, steps 2 and 3 with
                                    m != 0), clip_on_decay (c = 0.37), grad_param_order (every filter with taps > 1); the packs after
                                    every step: flip_one_axis, flip_none, fwd_oihw, bf16_truncated
  test_packs_after_construction,
  test_pack_only                    flip_one_axis, flip_none, fwd_oihw, bf16_truncated on the pack_only path
  test_step_end_to_end              clip_on_decay and a clip or rank average applied twice or not at all (c from the device's own norm)
  test_touched_mask, test_unused    no arithmetic mutant: a tensor walked that should be skipped, or the reverse, and writes outside a
                                    tensor's own slices (bound 0 everywhere else)"""
import numpy as np
import pytest
import torch

from tests import _bounds as B
from tests import _sgd_ref as R

pytestmark = pytest.mark.gpu

LR, MU, WD = 0.05, 0.9, 5e-4
PACKS = [None, torch.float32, torch.bfloat16]
N = len(R.SHAPES)
SIZES = [int(np.prod(s)) for s in R.SHAPES]


class Zoo:
    def __init__(self, pack_dtype):
        from fasterseg_amd.optim import FlatSGD
        from fasterseg_amd.parallel import FlatGradientSync
        self.pack_dtype = pack_dtype
        self.v = R.Values()
        self.offs, total = R.param_layout()
        self.buf = torch.empty(total, dtype=torch.float32, device="cuda")
        self.params = [torch.nn.Parameter(self.buf[o:o + n].view(s)) for o, n, s in zip(self.offs, SIZES, R.SHAPES)]
        assert all(p.data_ptr() == self.buf.data_ptr() + 4 * o for p, o in zip(self.params, self.offs))
        self.sync = FlatGradientSync(self.params)
        self.sync.sync()                                                        # single rank: only releases the gradient sink prepare() took
        assert self.sync.flat.numel() == sum(SIZES)
        self.goffs = self.sync.offsets
        self.packed = sorted((k for k in range(N) if pack_dtype is not None and R.packable(R.SHAPES[k])), key=lambda k: self.goffs[k])
        self.write_params()
        self.opt = FlatSGD(self.sync, LR, MU, WD, pack_dtype=pack_dtype)
        assert self.opt.chunks.shape[0] == sum(len(R.chunk_model(*R.geometry(s), k in self.packed)[1]) for k, s in enumerate(R.SHAPES))

    def write_params(self):
        host = np.full(self.buf.numel(), R.SENTINEL, np.float32)
        for k in range(N):
            host[self.offs[k]:self.offs[k] + SIZES[k]] = self.v.p[k].reshape(-1)
        self.buf.copy_(torch.from_numpy(host))

    def dense(self, per_tensor):
        """per-tensor arrays in parameter shape -> one flat array in the order of the gradient / momentum buffers"""
        out = np.zeros(sum(SIZES), np.float32)
        for k in range(N):
            out[self.goffs[k]:self.goffs[k] + SIZES[k]] = R.to_grad_order(per_tensor[k]).reshape(-1)
        return out

    def reset(self, momentum=False, lr=LR, mu=MU, wd=WD, max_norm=None, unused="skip"):
        opt = self.opt
        self.write_params()
        self.sync.flat.copy_(torch.from_numpy(self.dense(self.v.g)))
        self.sync.grad_scale = 1.0
        self.sync._touched = [True] * N
        if momentum:
            opt.momentum_buf.copy_(torch.from_numpy(self.dense(self.v.m)))
        else:
            opt.momentum_buf.zero_()
        opt.lr, opt.momentum, opt.weight_decay, opt.max_norm, opt.unused = lr, mu, wd, max_norm, unused
        opt._ever_touched = opt._last_touched = None
        opt.touched_dev.fill_(1)
        if self.packed:
            opt._launch(None, pack_only=True)
        self.hyper = (R.f32(lr), R.f32(mu), R.f32(wd))

    def snap(self):
        """the device's state, on the host"""
        opt = self.opt
        s = dict(p=self.buf.cpu().numpy(), g=self.sync.flat.cpu().numpy(), m=opt.momentum_buf.cpu().numpy())
        if self.packed:
            it = torch.int32 if self.pack_dtype == torch.float32 else torch.int16
            s["fwd"], s["flip"] = opt.pack_fwd.view(it).cpu().numpy(), opt.pack_flip.view(it).cpu().numpy()
        return s

    def tensor(self, s, k):
        """(p, m, g) of tensor k in the parameter's shape, fp64"""
        shape = R.SHAPES[k]
        p = s["p"][self.offs[k]:self.offs[k] + SIZES[k]].reshape(shape)
        m, g = (R.to_param_order(s[n][self.goffs[k]:self.goffs[k] + SIZES[k]], shape) for n in ("m", "g"))
        return p.astype(np.float64), m.astype(np.float64), g.astype(np.float64)

    def expect(self, s, c, touched, c_rel=0.0):
        """one step from state s -> (parameter buffer, its bound, momentum buffer, its bound); bound 0 where nothing may change"""
        lr, mu, wd = self.hyper
        ep, bp = s["p"].astype(np.float64), np.zeros(s["p"].size)
        em, bm = s["m"].astype(np.float64), np.zeros(s["m"].size)
        for k in range(N):
            if not touched[k]:
                continue
            p, m, g = self.tensor(s, k)
            m1, p1 = R.step64(p, m, g, c, lr, mu, wd)
            b_m, b_p = R.bound(p, m, g, c, lr, mu, wd, c_rel)
            ep[self.offs[k]:self.offs[k] + SIZES[k]], bp[self.offs[k]:self.offs[k] + SIZES[k]] = p1.reshape(-1), b_p.reshape(-1)
            a = self.goffs[k]
            em[a:a + SIZES[k]], bm[a:a + SIZES[k]] = R.to_grad_order(m1).reshape(-1), R.to_grad_order(b_m).reshape(-1)
        return ep, bp, em, bm

    def check_packs(self, s, what):
        """both pack buffers, whole, against packs64 of the parameters in state s"""
        if not self.packed:
            assert self.opt.pack_fwd is None and self.opt.pack_flip is None
            return
        want = [R.packs64(self.tensor(s, k)[0], self.pack_dtype) for k in self.packed]
        for name, j in (("fwd", 0), ("flip", 1)):
            w = np.concatenate([x[j].reshape(-1) for x in want])
            assert w.shape == s[name].shape
            bad = np.nonzero(w != s[name])[0]
            assert bad.size == 0, "%s: pack_%s differs at %d of %d elements, first at %d" % (what, name, bad.size, w.size, bad[0])

    def check_step(self, before, after, c, touched, what, c_rel=0.0):
        ep, bp, em, bm = self.expect(before, c, touched, c_rel)
        within(after["p"], ep, bp, what + " parameters")
        within(after["m"], em, bm, what + " momentum")
        same_bits(before["g"], after["g"], what + " sync.flat")
        self.check_packs(after, what)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b, what):
    bad = np.nonzero(bits(a) != bits(b))[0]
    assert bad.size == 0, "%s: %d of %d elements changed, first at %d" % (what, bad.size, a.size, bad[0])


def within(got32, ref64, bound, what):
    """bound > 0: |got - ref| <= bound through assert_within (prints the worst err / bound); bound == 0 (guards, skipped tensors): the
    bits the reference holds, which are fp32 values the device held before"""
    frozen = bound == 0
    same_bits(got32[frozen], ref64[frozen].astype(np.float32), what + " (guards and untouched tensors)")
    if not frozen.all():
        B.assert_within(torch.from_numpy(got32[~frozen]), torch.from_numpy(ref64[~frozen]), torch.from_numpy(bound[~frozen]), what)


@pytest.fixture(scope="module", params=PACKS, ids=["nopacks", "packs_f32", "packs_bf16"])
def zoo(request):
    return Zoo(request.param)


def test_layout_of_the_zoo_on_the_device(zoo):
    """packed tensors as FlatSGD chooses them, each with a packed neighbour where the tests below rely on one"""
    n_packed = sum(R.packable(s) for s in R.SHAPES)
    assert len(zoo.packed) == (0 if zoo.pack_dtype is None else n_packed) and n_packed == 5
    if zoo.packed:
        assert zoo.opt.pack_fwd.numel() == zoo.opt.pack_flip.numel() == sum(SIZES[k] for k in zoo.packed)
    for k in TOUCH_ONE:
        if R.packable(R.SHAPES[k]):                                             # a pack's neighbours are the packs of the packed tensors around it
            order = sorted((j for j in range(N) if R.packable(R.SHAPES[j])), key=lambda j: zoo.goffs[j])
            assert 0 < order.index(k) < len(order) - 1
        else:                                                                   # gradient and momentum slices follow the registration order
            assert R.packable(R.SHAPES[k - 1]) or R.packable(R.SHAPES[k + 1])
            assert abs(zoo.goffs[k] - zoo.goffs[k + 1]) in (SIZES[k], SIZES[k + 1])


def test_packs_after_construction(zoo):
    from fasterseg_amd.optim import FlatSGD
    zoo.reset()
    s0 = zoo.snap()
    old = zoo.opt
    try:
        zoo.opt = FlatSGD(zoo.sync, LR, MU, WD, pack_dtype=zoo.pack_dtype)
        s = zoo.snap()
        zoo.check_packs(s, "construction %s" % zoo.pack_dtype)
        same_bits(s0["p"], s["p"], "construction: parameters")
        assert not s["m"].any()
    finally:
        zoo.opt = old
        zoo.reset()


@pytest.mark.parametrize("c,momentum,mu,wd", [(None, False, MU, WD), (1.0, False, MU, WD), (0.37, True, MU, WD), (0.37, True, 0.0, 0.0)],
                         ids=["noscale", "c1", "c0.37", "c0.37_plain"])
def test_kernel_arithmetic(zoo, c, momentum, mu, wd):
    """three consecutive launches with a scale tensor of the test's own; every element of the parameter and momentum buffers inside the
    bound, guards and sync.flat bit-unchanged, packs bit-equal to the rounding of the stored parameters"""
    zoo.reset(momentum=momentum, mu=mu, wd=wd)
    scale = None if c is None else torch.tensor(c, dtype=torch.float32, device="cuda")
    c64 = 1.0 if c is None else R.f32(c)
    for step in range(3):
        before = zoo.snap()
        zoo.opt._launch(scale)
        after = zoo.snap()
        if step > 0 and mu > 0:
            assert before["m"].any()
        zoo.check_step(before, after, c64, [True] * N, "c=%s mu=%g wd=%g %s step %d" % (c, mu, wd, zoo.pack_dtype, step))


TOUCH_ONE = [8, 9, 7]            # (4097,) linear, (5, 29, 3, 3) tiled, (24, 264, 1, 1) packed: each next to a packed tensor


@pytest.mark.parametrize("k", TOUCH_ONE, ids=["linear", "tiled", "packed"])
def test_touched_mask(zoo, k):
    """one tensor touched: it updates within the bound, every other parameter, momentum slice and pack keeps its bits"""
    zoo.reset(momentum=True)
    touched = [i == k for i in range(N)]
    zoo.opt.touched_dev.copy_(torch.tensor(touched, dtype=torch.uint8))
    before = zoo.snap()
    zoo.opt._launch(torch.tensor(0.37, dtype=torch.float32, device="cuda"))
    after = zoo.snap()
    zoo.check_step(before, after, R.f32(0.37), touched, "only %s touched, %s" % (R.SHAPES[k], zoo.pack_dtype))
    a, n = zoo.offs[k], SIZES[k]
    assert (bits(after["p"][a:a + n]) != bits(before["p"][a:a + n])).any(), "the touched tensor did not move"
    if zoo.packed:                                                              # the other tensors' packs: the bits they had, not merely right ones
        keep = np.ones(before["fwd"].size, bool)
        if k in zoo.packed:
            start = sum(SIZES[j] for j in zoo.packed[:zoo.packed.index(k)])
            keep[start:start + n] = False
        for name in ("fwd", "flip"):
            assert np.array_equal(before[name][keep], after[name][keep]), name


def test_pack_only(zoo):
    """refresh_packs() after both pack buffers were overwritten: packs right again, parameters and momentum bit-unchanged, and the
    gradient buffer (all NaN) not read"""
    zoo.reset(momentum=True)
    zoo.sync.flat.fill_(float("nan"))
    if zoo.packed:
        zoo.opt.pack_fwd.fill_(3.0)
        zoo.opt.pack_flip.fill_(-3.0)
    before = zoo.snap()
    zoo.opt.refresh_packs()
    after = zoo.snap()
    same_bits(before["p"], after["p"], "pack_only: parameters")
    same_bits(before["m"], after["m"], "pack_only: momentum")
    assert np.isnan(after["g"]).all() and not np.isnan(after["p"]).any() and not np.isnan(after["m"]).any()
    zoo.check_packs(after, "pack_only %s" % zoo.pack_dtype)
    if zoo.packed:
        as_float = lambda a: a.view(np.float32) if zoo.pack_dtype == torch.float32 else (a.astype(np.int32) << 16).view(np.float32)
        assert not np.isnan(as_float(after["fwd"])).any() and not np.isnan(as_float(after["flip"])).any()


@pytest.mark.parametrize("gs", [1.0, 0.5], ids=["one_rank", "two_ranks_deferred"])
@pytest.mark.parametrize("active", [True, False], ids=["clip", "noclip"])
def test_step_end_to_end(zoo, active, gs):
    """step() with max_norm: the returned norm against the fp64 norm of the gradient buffer (1e-4 relative, the tolerance of
    test_flat_sgd_matches_torch_sgd_with_clip), the update against c formed in fp64 FROM the returned norm as optim.py forms it,
    c = min(1, max_norm / (norm + 1e-6)) * grad_scale, charged 3 E32 for its three fp32 operations (the sum, and the quotient as torch
    forms float / tensor: a reciprocal and a product; the product with a grad_scale of 0.5 is exact).  grad_scale = 0.5 is what sync()
    leaves with two ranks under average="defer": SGD on the halved gradients, the clip decided on the halved norm."""
    norm64 = float(np.sqrt((zoo.dense(zoo.v.g).astype(np.float64) ** 2).sum())) * gs
    max_norm = R.f32(norm64 * (0.5 if active else 4.0))
    zoo.reset(momentum=True, max_norm=max_norm)
    for step in range(2):
        zoo.sync.grad_scale = gs
        zoo.sync._touched = [True] * N
        before = zoo.snap()
        norm = zoo.opt.step()
        after = zoo.snap()
        assert norm is zoo.opt.last_norm
        norm_dev = float(norm)
        print("norm: device %.9g, fp64 %.9g" % (norm_dev, norm64))
        assert abs(norm_dev - norm64) <= 1e-4 * norm64
        ratio = max_norm / (norm_dev + 1e-6)
        assert (ratio < 1.0) == active and (norm64 > max_norm) == active
        c64, c_rel = (ratio * gs, 3 * B.E32) if active else (gs, 0.0)           # an inactive clip is clamped to exactly 1, times 0.5 exactly
        zoo.check_step(before, after, c64, [True] * N, "step() clip=%d grad_scale=%g %s step %d" % (active, gs, zoo.pack_dtype, step), c_rel)


UNUSED_A, UNUSED_B = 6, 4        # (17, 28, 3, 3) tiled: touched in step 1 only; (16, 256, 1, 1) packed where there are packs: never


@pytest.mark.parametrize("mode", ["skip", "decay"])
def test_unused(zoo, mode):
    """three steps; A receives a gradient only in the first, B never.  "skip": A is bit-frozen in steps 2 and 3.  "decay": A follows the
    update with g = 0 (it decays and coasts on its momentum).  B is bit-frozen throughout in both modes."""
    zoo.reset(momentum=False, unused=mode)
    g = zoo.dense(zoo.v.g)
    for k in (UNUSED_A, UNUSED_B):
        assert np.abs(zoo.v.p[k]).min() > 0
    for step in range(3):
        touched = [k != UNUSED_B and (k != UNUSED_A or step == 0) for k in range(N)]
        host = g.copy()
        for k in range(N):
            if not touched[k]:
                host[zoo.goffs[k]:zoo.goffs[k] + SIZES[k]] = 0.0                # what prepare() leaves in the slice of an untouched parameter
        zoo.sync.flat.copy_(torch.from_numpy(host))
        zoo.sync._touched = list(touched)
        before = zoo.snap()
        assert zoo.opt.step() is None
        after = zoo.snap()
        walked = list(touched)
        if mode == "decay":
            walked[UNUSED_A] = True
        zoo.check_step(before, after, 1.0, walked, "unused=%s %s step %d" % (mode, zoo.pack_dtype, step))
        a, n = zoo.offs[UNUSED_A], SIZES[UNUSED_A]
        moved = (bits(after["p"][a:a + n]) != bits(before["p"][a:a + n])).any()
        assert moved == (step == 0 or mode == "decay")
        b, nb = zoo.offs[UNUSED_B], SIZES[UNUSED_B]
        same_bits(before["p"][b:b + nb], after["p"][b:b + nb], "B's parameters")
        assert not after["m"][zoo.goffs[UNUSED_B]:zoo.goffs[UNUSED_B] + nb].any()
