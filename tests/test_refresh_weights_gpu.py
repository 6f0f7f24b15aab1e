"""Reloading weights into a built inference engine (fs_refresh_weights, InferenceEngine.load_weights and its callers).

The reference changes the weights under a live evaluator: train/train.py:196-208 validates the model it is training,
search/train_search.py:141-183 after every epoch, train/train.py:124-135 loads a trained teacher into an existing model.  Here
a built engine follows with one grouped launch that rewrites its packs and folded BatchNorms in place; these tests pin
  1. the kernel alone: every entry form in ONE launch, packs byte-equal to the stand-alone pack kernels, folds against fp64,
     guard words around every destination;
  2. - 5. the engine: same addresses and graph, packs byte-equal to direct packs of the new net, logits against the CPU oracle
     through every way the plan can be issued, the in-place (training) path, the teacher, and the refusals;
  6. - 7. SegEvaluator.load_weights and StudentDistillStep.load_teacher.
Engines are built with FS_ENGINE_AUTOTUNE=0 and a fixed fuse_cells: nothing here waits for tuning."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (1, 3, 256, 512)
_cache = {}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 64          # elements in front of and behind every destination


class _Guarded:
    """A destination of n elements of `dtype` between two runs of GUARD sentinel elements."""

    def __init__(self, n, dtype):
        raw_t, self.pattern = (torch.int16, 0x5A5A) if dtype == torch.bfloat16 else (torch.int32, 0x5A5A5A5A)
        self.raw = torch.full((n + 2 * GUARD,), self.pattern, dtype=raw_t, device="cuda")
        self.view = self.raw[GUARD:GUARD + n].view(dtype)
        self.n = n

    def intact(self):
        return bool((self.raw[:GUARD] == self.pattern).all()) and bool((self.raw[GUARD + self.n:] == self.pattern).all())


def test_kernel_rewrites_every_form_in_one_launch():
    from fasterseg_amd import _lib as L, kernels as K
    lib = L.lib()
    g = torch.Generator().manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    w1 = rnd(19, 128, 1, 1)                 # classifier-sized 1x1
    wide = rnd(48, 32, 3, 3)                # a USConv2d-style parent: the 40 x 24 block is read in place
    stem = rnd(16, 3, 3, 3)
    w32 = rnd(32, 8, 3, 3)
    half = 12
    gamma, beta, mean = rnd(2 * half), rnd(2 * half), rnd(2 * half) * 0.1
    var = (torch.rand(2 * half, generator=g) + 0.5).cuda()
    bias = rnd(19)
    eps = 1e-5
    chunk = lib.fs_refresh_chunk_elems()

    entries, dests, wants = [], [], []

    def pack(w, cout, cin, dtype, frag):
        n = lib.fs_packed_weight_frag_elems(cout, cin, K.dtype_code(dtype)) if frag else cout * cin * w.shape[2] * w.shape[3]
        d = _Guarded(n, dtype)
        e = L.RefreshEntry()
        e.kind, e.dtype, e.Cout, e.Cin, e.R, e.S = (L.FS_REFRESH_PACK_FRAG if frag else L.FS_REFRESH_PACK), K.dtype_code(dtype), cout, cin, w.shape[2], w.shape[3]
        e.o_stride, e.i_stride, e.src, e.dst = w.stride(0), w.stride(1), w.data_ptr(), d.view.data_ptr()
        want = K.pack_weight_frag(w, dtype, cout, cin) if frag else K.pack_weight(w, dtype, cout, cin)
        entries.append(e); dests.append(d); wants.append(want.reshape(-1))

    for dtype in (torch.float32, torch.bfloat16):
        pack(w1, 19, 128, dtype, False)
        pack(wide, 40, 24, dtype, False)
        pack(wide, 40, 24, dtype, True)
        pack(w32, 32, 8, dtype, True)
    pack(stem, 16, 3, torch.float32, False)
    assert wide.stride(0) != 24 * 9
    folds = []
    for lo in (0, half):
        sc, sh = _Guarded(half, torch.float32), _Guarded(half, torch.float32)
        e = L.RefreshEntry()
        e.kind, e.Cout, e.lo, e.eps = L.FS_REFRESH_FOLD, half, lo, eps
        e.src, e.beta, e.mean, e.var, e.dst, e.shift = gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), sc.view.data_ptr(), sh.view.data_ptr()
        entries.append(e); folds.append((lo, sc, sh))
    bdst = _Guarded(19, torch.float32)
    e = L.RefreshEntry()
    e.kind, e.Cout, e.src, e.shift = L.FS_REFRESH_BIAS, 19, bias.data_ptr(), bdst.view.data_ptr()
    entries.append(e)

    counts = [lib.fs_refresh_entry_chunks(ctypes.byref(e)) for e in entries]
    assert all(c >= 1 for c in counts), (counts, lib.fs_last_error())
    assert 19 * 128 < chunk and counts[0] == 1 and max(counts) > 1          # an entry below one chunk, entries over several
    table = (L.RefreshEntry * len(entries))(*entries)
    dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    chunks = torch.tensor([(t, k) for t, c in enumerate(counts) for k in range(c)], dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    L.call("fs_refresh_weights", K._stream(), K._p(dev), len(entries), K._p(chunks), chunks.shape[0])      # ONE launch
    torch.cuda.synchronize()

    for i, (d, want) in enumerate(zip(dests, wants)):
        raw = torch.int16 if want.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(d.view.view(raw), want.view(raw)), "pack entry %d differs from the stand-alone pack kernel" % i
        assert d.intact(), "pack entry %d wrote outside its destination" % i
    f32 = lambda v: np.float32(v).astype(np.float64)
    G, B, M, V = (t.double().cpu().numpy() for t in (gamma, beta, mean, var))
    for lo, sc, sh in folds:
        sl = slice(lo, lo + half)
        s = G[sl] / np.sqrt(V[sl] + f32(eps))              # eps as the fp32 the entry carries
        t = B[sl] - M[sl] * s
        es = np.abs(sc.view.double().cpu().numpy() - s)
        et = np.abs(sh.view.double().cpu().numpy() - t)
        print("fold lo=%d: max scale err / bound %.3f, max shift err / bound %.3f" % (
            lo, float((es / (4 * 2.0 ** -23 * np.abs(s))).max()), float((et / (5 * 2.0 ** -23 * (np.abs(B[sl]) + np.abs(M[sl] * s)))).max())))
        # one rounded add, rsqrtf within 2 ulp, one rounded multiply; then a multiply-subtract the compiler may contract or not
        assert (es <= 4 * 2.0 ** -23 * np.abs(s)).all()
        assert (et <= 5 * 2.0 ** -23 * (np.abs(B[sl]) + np.abs(M[sl] * s))).all()
        assert sc.intact() and sh.intact()
    assert torch.equal(bdst.view, bias) and bdst.intact()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. - 5. the engine
# ---------------------------------------------------------------------------------------------------------------------------
def _meta():
    with open(os.path.join(ROOT, "tests", "golden", "arch_1.json")) as f:
        return json.load(f)["eval_21"]


def _student(seed):
    """(net on the GPU, its state on the host) of the suite's small student with seeded weights AND running statistics."""
    from fasterseg_amd import archs
    from oracle.seeded import seeded_state
    net = archs.build_derived(1, training=False, lasts=[2, 1])
    state = seeded_state(net.state_dict(), seed)
    net.load_state_dict(state)
    return net.cuda().eval(), state


def _oracle(seed):
    """(input, oracle logits) of the student with seed `seed`: computed once on the host, shared, never modified."""
    if seed not in _cache:
        from oracle import ref_ops
        from oracle.seeded import resolve_aliases, seeded_input
        _, state = _student(seed)
        x = seeded_input(SHAPE, 3)
        with torch.no_grad():
            want = ref_ops.derived_forward(resolve_aliases({k: v.clone() for k, v in state.items()}, _meta()), _meta(), x, training=False)
        _cache[seed] = (x, want)
    return _cache[seed]


def _check(got, want, dtype, what):
    """The engine bars of tests/test_engine_gpu.py."""
    got = got.float().cpu()
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    if dtype == torch.float32:
        assert err <= 1e-3, "%s: fp32 logits differ from the oracle by %.3e (> 1e-3)" % (what, err)
    else:
        rel = err / float(want.abs().max())
        agree = float((got.argmax(1) == want.argmax(1)).float().mean())
        assert rel <= 5e-2, "%s: bf16 logits rel. error %.3e (> 5e-2)" % (what, rel)
        assert agree >= 0.97, "%s: bf16 arg-max agreement %.4f (< 0.97)" % (what, agree)


def _kept(eng):
    """Every weight-derived tensor the plan keeps (packs, scales, shifts)."""
    return [t for r in eng._refresh for t in (r["dst"], r["shift"]) if t is not None]


def _snapshot(eng):
    return [t.clone() for t in _kept(eng)]


def _same_bytes(a, b):
    raw = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    return all(torch.equal(raw(x), raw(y)) for x, y in zip(a, b))


def _check_every_issue_path(eng, x, want, dtype, what):
    with torch.no_grad():
        eng.input.copy_(x.cuda())
        eng.graph.replay()
        torch.cuda.synchronize()
        _check(eng.output.clone(), want, dtype, what + ": graph replay")
        eng.output.zero_()
        eng._launch_all()
        torch.cuda.synchronize()
        _check(eng.output.clone(), want, dtype, what + ": direct launch list")
        eng.output.zero_()
        eng._run_program()
        torch.cuda.synchronize()
        _check(eng.output.clone(), want, dtype, what + ": launch program")


def _check_packs_against(eng, dtype):
    """Every kept pack is what the stand-alone pack kernels give for the sources the engine is now bound to."""
    from fasterseg_amd import _lib as L, kernels as K
    n = 0
    for r in eng._refresh:
        if r["kind"] not in (L.FS_REFRESH_PACK, L.FS_REFRESH_PACK_FRAG):
            continue
        i, f = r["slot"]
        w = eng._sources[i][f].detach()
        direct = (K.pack_weight_frag if r["kind"] == L.FS_REFRESH_PACK_FRAG else K.pack_weight)(w, r["dtype"], r["cout"], r["cin"])
        assert _same_bytes([r["dst"].reshape(-1)], [direct.reshape(-1)]), "pack of op %d (%s) is not the direct pack" % (i, f)
        n += 1
    assert n >= 10, n


@pytest.mark.parametrize("cells", ["1", "0"], ids=["fused", "split"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_follows_another_net_of_the_same_architecture(dtype, cells, monkeypatch):
    from fasterseg_amd import engine
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    net_a, _ = _student(12345)
    net_b, _ = _student(999)
    x, want_b = _oracle(999)
    with torch.no_grad():
        eng = engine.InferenceEngine(net_a, SHAPE, dtype=dtype, fuse_cells=cells)
        eng.input.copy_(x.cuda())
        ptrs = [t.data_ptr() for t in eng._keep if torch.is_tensor(t)]
        graph, calls = id(eng.graph), [(c["fn"], c["label"]) for c in eng.calls]
        assert eng.graph is not None and len(_kept(eng)) >= 20
        eng.load_weights(net_b)
        torch.cuda.synchronize()
    assert [t.data_ptr() for t in eng._keep if torch.is_tensor(t)] == ptrs and id(eng.graph) == graph
    assert [(c["fn"], c["label"]) for c in eng.calls] == calls
    _check_packs_against(eng, dtype)
    _check_every_issue_path(eng, x, want_b, dtype, "after load_weights(net_b)")
    # there and back: the refresh is a pure function of the sources
    eng.load_weights(net_a)
    torch.cuda.synchronize()
    first = _snapshot(eng)
    eng.load_weights(net_b)
    eng.load_weights(net_a)
    torch.cuda.synchronize()
    assert _same_bytes(_snapshot(eng), first)
    x_a, want_a = _oracle(12345)
    _check(eng(x_a.cuda()).clone(), want_a, dtype, "back on net_a")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_rereads_parameters_updated_in_place(dtype, monkeypatch):
    """The training case: an optimizer (here copy_) changes the traced net's own tensors; load_weights() takes no argument."""
    from fasterseg_amd import engine
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    net, _ = _student(12345)
    _, state_b = _student(999)
    x, want_b = _oracle(999)
    with torch.no_grad():
        eng = engine.InferenceEngine(net, SHAPE, dtype=dtype, fuse_cells="1")
        own = net.state_dict()
        for k, v in state_b.items():
            own[k].copy_(v)                      # parameters and running statistics, in place
        eng.load_weights()
        torch.cuda.synchronize()
        assert not eng._stages, "sources on the device are read in place, not staged"
    _check_packs_against(eng, dtype)
    _check_every_issue_path(eng, x, want_b, dtype, "after in-place update + load_weights()")


def test_engine_stages_sources_that_are_not_on_the_device(monkeypatch):
    """A net on the host (what torch.load gives) is staged to the device, as the constructor's .to(device) does."""
    from fasterseg_amd import engine
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    net_a, _ = _student(12345)
    net_b, _ = _student(999)
    x, want_b = _oracle(999)
    with torch.no_grad():
        eng = engine.InferenceEngine(net_a, SHAPE, dtype=torch.float32, fuse_cells="1")
        eng.load_weights(net_b.cpu())
        _check(eng(x.cuda()).clone(), want_b, torch.float32, "after load_weights(host net)")


def test_teacher_engine_follows_new_weights(monkeypatch):
    from fasterseg_amd import archs, engine
    from oracle.seeded import seeded_input, seeded_state
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    nets = []
    for seed in (777, 778):
        net = archs.build_derived(0, training=False)
        net.load_state_dict(seeded_state(net.state_dict(), seed))
        nets.append(net.cuda().eval())
    shape = (2, 3, 256, 512)
    x = seeded_input(shape, 5).cuda()
    with torch.no_grad():
        eng = engine.InferenceEngine(nets[0], shape, dtype=torch.float32, fuse_cells="1", output="lowres")
        eng.load_weights(nets[1])
        got = eng(x).float().cpu()
        want = nets[1].forward_lowres(x).float().cpu()              # per-operator path of the NEW net
        stale = nets[0].forward_lowres(x).float().cpu()
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-3, float((got - want).abs().max())
    assert float((got - stale).abs().max()) > 1e-3                   # the two nets do differ by more than the bar


def test_load_weights_refuses_before_writing(monkeypatch):
    from fasterseg_amd import archs, engine
    from oracle.seeded import seeded_state
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    net_a, _ = _student(12345)
    with torch.no_grad():
        eng = engine.InferenceEngine(net_a, SHAPE, dtype=torch.bfloat16, fuse_cells="1")
    eng.load_weights()                       # tables exist from here on: a refusal has something it could have spoiled
    torch.cuda.synchronize()
    before = _snapshot(eng)
    teacher = archs.build_derived(0, training=False)
    teacher.load_state_dict(seeded_state(teacher.state_dict(), 777))
    with pytest.raises(ValueError, match=r"op \d+"):
        eng.load_weights(teacher.cuda().eval())
    net_b, _ = _student(999)
    with pytest.raises(ValueError, match="training mode"):
        eng.load_weights(net_b.train())
    torch.cuda.synchronize()
    assert _same_bytes(_snapshot(eng), before)
    x, want = _oracle(12345)
    _check(eng(x.cuda()).clone(), want, torch.bfloat16, "after two refused reloads")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. SegEvaluator.load_weights
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_evaluator_load_weights_matches_a_fresh_evaluator(dtype, monkeypatch):
    from fasterseg_amd.evaluator import SegEvaluator
    for k, v in (("FS_ENGINE_AUTOTUNE", "0"), ("FS_ENGINE_FUSE_CELLS", "1"), ("FS_ENGINE_FOLD_RESIZE", "0")):
        monkeypatch.setenv(k, v)             # no choice is timed: both evaluators get the same plans
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    img = torch.randint(0, 256, (256, 512, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
    net_a, _ = _student(12345)
    net_b, _ = _student(999)
    kw = dict(image_shape=(256, 512), dtype=dtype, multi_scales=[0.75, 1.0], is_flip=True, crop_size=256)

    def maps(ev):
        return [ev.sliding_eval(img, 256, 5 / 6).clone(), ev.whole_eval(img).clone()]
    ev = SegEvaluator(net_a, 19, mean, std, **kw)
    stale = maps(ev)                         # builds the window engine and the whole-image engine
    assert len(ev._lowres) >= 2
    ev.acc.add(stale[0], torch.zeros((256, 512), dtype=torch.uint8, device="cuda"))
    hist = ev.acc.result()[0].copy()
    ev.load_weights(net_b)
    assert ev.val_func is net_b and (ev.acc.result()[0] == hist).all()
    got = maps(ev)
    want = maps(SegEvaluator(net_b, 19, mean, std, **kw))
    torch.cuda.synchronize()
    for g_, w_, s_ in zip(got, want, stale):
        agree = float((g_ == w_).float().mean())
        if dtype == torch.float32:
            assert torch.equal(g_, w_), agree
        else:
            assert agree >= 0.97, agree
        assert not torch.equal(s_, w_)                          # the old weights give another map


# ---------------------------------------------------------------------------------------------------------------------------
# 7. StudentDistillStep.load_teacher
# ---------------------------------------------------------------------------------------------------------------------------
def test_distill_step_loads_a_teacher_after_construction(monkeypatch):
    from fasterseg_amd.train_step import StudentDistillStep
    from oracle.seeded import seeded_input, seeded_state
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    monkeypatch.setenv("FS_ENGINE_FUSE_CELLS", "1")
    st = StudentDistillStep(2, 128, 256, teacher_engine_dtype=torch.float32)
    imgs = seeded_input((2, 3, 128, 256), 9).cuda()
    before = st.teacher_logits(imgs).float().cpu().clone()
    graph = id(st.teacher_engine.graph)
    state = seeded_state(st.teacher.state_dict(), 4242)
    state["not.in.the.model"] = torch.zeros(3)                  # train/train.py:127 keeps only the model's keys
    st.load_teacher(state)
    assert id(st.teacher_engine.graph) == graph
    own = st.teacher.state_dict()
    first = next(iter(own))                 # the stem's filter: under one key only (shared cells appear under several, the last alias wins)
    assert torch.equal(own[first].cpu(), state[first]) and "not.in.the.model" not in own
    with torch.no_grad():
        got = st.teacher_logits(imgs).float().cpu()
        want = st.teacher.forward_lowres(imgs).float().cpu()
    assert float((got - want).abs().max()) <= 1e-3, float((got - want).abs().max())
    assert float((got - before).abs().max()) > 1e-3
