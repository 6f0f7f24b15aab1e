"""Parity of the train paths bench.py times, at the benchmarked size and in the benchmarked dtype.

* F12.L16 supernet (search/config_search.py:81-84) `_loss` forward + backward at the C3 map size (1x3x256x512, pretrain passes)
  and the C5 map size (1x3x224x448, search passes: 28x56 / 14x28 / 7x14 maps and the zoomed 3x7 ones) against fixtures the
  UNMODIFIED reference produced in fp64 (tests/golden/supernet_l16*, oracle/make_golden.py gen_supernet_l16) - through the bare
  modules (fp32) and through train_step.SupernetStep exactly as bench.py builds it (hipGraph replay of the fixed-width passes,
  MixedOp launch programs, pair batching, flat-gradient sink), fp32 AND bf16.
* the student's KL-distillation step (train/train.py:246-262: frozen teacher, 3 student heads, OHEM-CE + KLDiv) through
  train_step.StudentDistillStep as bench.py builds it, fp32 AND bf16, against the reference's fp64 run at 2x3x256x512
  (tests/golden/student_step*, oracle/make_golden.py gen_student_step).

Bars.  fp32 (exact-fp32 MFMA, fp32 storage): loss 2e-3 relative, gradient norms and per-tensor relative L2 5e-2 (measured: loss exact to
7 digits, per-tensor relative L2 <= 2e-2, i.e. the reference's own fp32-vs-fp64 difference: batch-statistics BN over a few dozen
samples amplifies a 1e-7 rounding to 1e-2 in the gradients of deep layers - an amplification of ~1e5).
bf16 (bf16 storage of every activation and activation gradient, bf16 MFMA operands, fp32 accumulation / statistics / master weights /
parameter gradients): the LOSS is within 1e-3 of the fp64 reference (bar 5e-3) and the same parameters receive gradients, but the
same ~1e5 amplification acts on the 4e-3 storage rounding: gradients of tensors next to the heads agree (cosine >= 0.99), those of
deep layers only in direction (measured cosine 0.5 - 0.9, norms within 40 %) - on these batch-1 fixtures a bf16 gradient is as far
from the fp64 one as a gradient of another mini-batch would be.  That is a property of bf16 storage under tiny-batch BatchNorm, not
of a kernel (every kernel is pinned per operator in bf16 in tests/test_kernels_gpu.py / test_ops_gpu.py); it is why bench.py prints
an fp32 leg for every train workload and why the bars below for bf16 gradients are sanity bars (cosine >= 0.25 - three runs measured
0.50 - 0.60 for the worst tensor - and norms within 2x for 95 % of the sampled tensors), not parity bars.  Measured values are written to gpurun_out/parity_metrics.json and quoted in DESIGN.md.
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from oracle.seeded import seeded_input, seeded_state
from tests._util import golden_get, load_json, load_npz

pytestmark = pytest.mark.gpu
WML = [4. / 12, 6. / 12, 8. / 12, 10. / 12, 1.]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"pretrain": (1, 3, 256, 512), "search": (1, 3, 224, 448)}


def _record(name, metrics):
    out = os.path.join(ROOT, "gpurun_out")
    if not os.path.isdir(out):
        return
    path = os.path.join(out, "parity_metrics.json")
    try:
        with open(path) as f:
            data = json.load(f)
    except Exception:
        data = {}
    data[name] = metrics
    with open(path, "w") as f:
        json.dump(data, f, indent=1)


def _l16_state(net):
    sd = seeded_state(net.state_dict(), 778)
    for k in list(sd):
        if k.split("_")[0] in ("alpha", "beta", "ratio"):
            sd[k] = sd[k] * 5.0
    return sd


def _batch(mode, fixture="supernet_l16"):
    shape = CASES[mode] if fixture == "supernet_l16" else tuple(load_json(fixture + "_meta.json")[mode]["shape"])
    store = load_npz(fixture + ".npz")
    return seeded_input(shape, 41).cuda(), torch.tensor(store[mode + "/target"]).cuda()


def _cos_rel(got, store, key):
    want, step = golden_get(store, key)
    g = got.detach().float().cpu().numpy().reshape(-1)[::step].astype(np.float64)
    w = want.reshape(-1).astype(np.float64)
    cos = float((g * w).sum() / (np.sqrt((g * g).sum() * (w * w).sum()) + 1e-300))
    rel = float(np.sqrt(((g - w) ** 2).sum()) / (np.sqrt((w * w).sum()) + 1e-300))
    return cos, rel


def _check(name, loss, params, mode, dtype, weights_only, fixture="supernet_l16", extra=None):
    store = load_npz(fixture + ".npz")
    meta = load_json(fixture + "_meta.json")[mode]
    bf16 = dtype == torch.bfloat16
    want = float(store[mode + "/loss"][0])
    loss_rel = abs(loss - want) / abs(want)
    is_arch = lambda k: k.split("_")[0] in ("alpha", "beta", "ratio")
    got_names = sorted(k for k, p in params.items() if p.grad is not None and not (weights_only and is_arch(k)))
    tag = "weights_with_grad" if weights_only else "params_with_grad"
    norm_bar = 1.0 if bf16 else 5e-2
    bad, worst = [], 0.0
    sampled = {k: w for k, w in meta["gradnorms"].items() if not (weights_only and is_arch(k))}
    for k, w in sampled.items():
        g = float(params[k].grad.float().norm())
        err = abs(g - w) / (w + 1e-12)
        worst = max(worst, err)
        if abs(g - w) > norm_bar * w + 1e-6:
            bad.append((k, g, w))
    cos_min, rel_max, per = 1.0, 0.0, {}
    for key in store:
        if key.startswith(mode + "/g/"):
            pname = key[len(mode + "/g/"):].split("@")[0]
            if params[pname].grad is None:
                continue
            cos, rel = _cos_rel(params[pname].grad, store, mode + "/g/" + pname)
            per[pname] = (round(cos, 5), round(rel, 5))
            cos_min, rel_max = min(cos_min, cos), max(rel_max, rel)
    _record(name, dict(loss=loss, want=want, loss_rel=loss_rel, n_with_grad=len(got_names), norms_checked=len(sampled), norms_missed=len(bad),
                       worst_norm_err=worst, cos_min=cos_min, rel_l2_max=rel_max, per_tensor=per, **(extra or {})))
    assert loss_rel <= (5e-3 if bf16 else 2e-3), (loss, want)
    assert len(got_names) == meta[tag] and hashlib.sha1("\n".join(got_names).encode()).hexdigest() == meta[tag + "_sha1"], \
        "a different set of parameters received gradients (%d vs %d)" % (len(got_names), meta[tag])
    assert len(bad) <= (len(sampled) // 20 if bf16 else len(sampled) // 100), bad[:8]
    if bf16:
        near_head = [v for k, v in per.items() if k.startswith("head")]
        assert cos_min >= 0.25 and all(c >= 0.99 for c, _ in near_head), per
    else:
        assert cos_min >= 0.999 and rel_max <= 5e-2, per


@pytest.mark.parametrize("mode", ["pretrain", "search"])
def test_l16_supernet_modules_fp32(mode):
    """The bare modules (per-module autograd path, architecture parameters differentiated too) at full depth / real map sizes."""
    from fasterseg_amd import model_search
    net = model_search.Network_Multi_Path(19, 16, torch.nn.CrossEntropyLoss(ignore_index=255), 12, WML, ['max', 'arch_ratio'],
                                          [(1, 1), (8. / 12, 8. / 12)])
    net.load_state_dict(_l16_state(net))
    net = net.cuda().train()
    x, target = _batch(mode)
    np.random.seed(5)
    torch.manual_seed(6)
    net.arch_idx = 0
    loss = net._loss(x, target, mode == "pretrain")
    loss.backward()
    _check("l16_modules_fp32_" + mode, float(loss.detach()), dict(net.named_parameters()), mode, torch.float32, weights_only=False)


class _FrozenLR:
    """train_step.SearchConfig with lr = 0: the step runs its optimizer kernel but leaves the weights where the fixture has them."""
    lr = 0.0
    momentum = 0.9
    weight_decay = 5e-4
    grad_clip = 5
    arch_learning_rate = 3e-4
    layers = 16
    Fch = 12
    width_mult_list = WML
    prun_modes = ['max', 'arch_ratio']
    stem_head_width = [(1, 1), (8. / 12, 8. / 12)]
    latency_weight = [0, 1e-2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["pretrain", "search"])
def test_l16_supernet_step_as_benchmarked(mode, dtype):
    """train_step.SupernetStep as bench.py runs it (graphs + programs + pair batching + flat-gradient sink, compute dtype), one
    weight step of `_loss` on the fixture's weights and batch: loss and gradients vs the reference's fp64 run."""
    from fasterseg_amd.train_step import SupernetStep
    st = SupernetStep(pretrain=(mode == "pretrain"), cfg=_FrozenLR, compute_dtype=dtype)
    st.architect = None                                   # the fixture is `_loss` of the weight step (train_search.py:246-250)
    st._prewarmed = True                                  # (the program prewarm after a first step re-arms the gradient buffer)
    st.model.load_state_dict({k: v.cuda() for k, v in _l16_state(st.model).items()})
    st.optimizer.refresh_packs()
    x, target = _batch(mode)
    np.random.seed(5)
    torch.manual_seed(6)
    st.model.arch_idx = 0
    loss, _ = st.step(x, target)
    torch.cuda.synchronize()
    assert st.graphs, "the fixed-width passes were not captured"
    _check("l16_step_%s_%s" % ("bf16" if dtype == torch.bfloat16 else "fp32", mode), float(loss), dict(st.model.named_parameters()), mode,
           dtype, weights_only=True)


def _bn_after(st, mode, fixture):
    """Running statistics after the step of the BatchNorms the fixture holds: num_batches_tracked (exact) and, per statistic, the error
    relative to the stored value and relative to the stored UPDATE (stored - initial: the part the step's batch statistics contribute)."""
    store = load_npz(fixture + ".npz")
    tracked = load_json(fixture + "_meta.json")[mode]["bn_num_batches_tracked"]
    bufs = dict(st.model.named_buffers())
    init = _l16_state(st.model)
    counts, value_rel, update_rel = [], {}, {}
    for m, n in tracked.items():
        counts.append((m, int(bufs[m + ".num_batches_tracked"]), n))
        for stat in ("running_mean", "running_var"):
            k = m + "." + stat
            got = bufs[k].detach().double().cpu()
            want = torch.from_numpy(store["%s/bn/%s" % (mode, k)]).double()
            r0 = init[k].double()
            value_rel[k] = float((got - want).norm() / want.norm())
            update_rel[k] = float((got - want).norm() / ((want - r0).norm() + 1e-30))
    return counts, value_rel, update_rel


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["pretrain", "search"])
def test_l16_supernet_step_at_benchmarked_batch(mode, dtype):
    """As test_l16_supernet_step_as_benchmarked, at the batches bench.py times (C3: 3 x 3x256x512 pretrain passes, C5: 2 x 3x224x448 search
    passes, distinct samples) against the reference's fp64 run (tests/golden/supernet_l16_b*, oracle/make_golden.py gen_supernet_l16_batch).
    At batch 1 a joint tail that normalised per sample, or split the two passes' halves at the wrong offset, and BN statistics reduced over
    the wrong N give the fixture's numbers; here they do not.  Also the running statistics after the step of every BatchNorm outside the
    cells (stem, refinement, heads: the joint tail's grouped BatchNorm updates them half after half) and of eight deep-cell ones that more
    than one pass updated: num_batches_tracked exactly, the values within 2e-2 relative; in fp32 also the update (value after the step
    minus the value before it) within 2e-2 relative, which a momentum update applied twice, in another order or with the statistics of
    the wrong half of the batch would miss by far more."""
    from fasterseg_amd.train_step import SupernetStep
    fixture = "supernet_l16_b"
    bf16 = dtype == torch.bfloat16
    st = SupernetStep(pretrain=(mode == "pretrain"), cfg=_FrozenLR, compute_dtype=dtype)
    st.architect = None
    st._prewarmed = True
    st.model.load_state_dict({k: v.cuda() for k, v in _l16_state(st.model).items()})
    st.optimizer.refresh_packs()
    x, target = _batch(mode, fixture)
    assert x.shape[0] == (3 if mode == "pretrain" else 2) and not torch.equal(x[0], x[1])
    np.random.seed(5)
    torch.manual_seed(6)
    st.model.arch_idx = 0
    loss, _ = st.step(x, target)
    torch.cuda.synchronize()
    assert st.graphs, "the fixed-width passes were not captured"
    assert any(len(g) > 1 for g in st._pass_groups), "no joint pass: the grouped tail is not exercised"
    counts, value_rel, update_rel = _bn_after(st, mode, fixture)
    extra = dict(bn_checked=len(counts), bn_value_rel_max=max(value_rel.values()), bn_update_rel_max=max(update_rel.values()),
                 bn_update_rel_worst=sorted(update_rel.items(), key=lambda kv: -kv[1])[:4])
    _check("l16_step_batch_%s_%s" % ("bf16" if bf16 else "fp32", mode), float(loss), dict(st.model.named_parameters()), mode, dtype,
           weights_only=True, fixture=fixture, extra=extra)
    assert len(counts) >= 20 and any(m.startswith("cells.") for m, _, _ in counts)
    assert all(got == want for _, got, want in counts), [c for c in counts if c[1] != c[2]]
    assert max(value_rel.values()) <= 2e-2, sorted(value_rel.items(), key=lambda kv: -kv[1])[:4]
    if not bf16:
        assert max(update_rel.values()) <= 2e-2, extra["bn_update_rel_worst"]


def test_l16_supernet_step_is_reproducible_in_loss():
    """Two fresh builds of the bf16 pretrain step on the same weights / batch / seeds give the same loss to 1e-3 relative (the
    remaining run-to-run differences are float atomics in BN statistics of maps > 512 px and in the weight-gradient slabs)."""
    from fasterseg_amd.train_step import SupernetStep
    out = []
    for _ in range(2):
        st = SupernetStep(pretrain=True, cfg=_FrozenLR, compute_dtype=torch.bfloat16)
        st._prewarmed = True
        st.model.load_state_dict({k: v.cuda() for k, v in _l16_state(st.model).items()})
        st.optimizer.refresh_packs()
        x, target = _batch("pretrain")
        np.random.seed(5)
        torch.manual_seed(6)
        out.append(float(st.step(x, target)[0]))
        del st
        torch.cuda.empty_cache()
    assert abs(out[0] - out[1]) <= 1e-3 * abs(out[0]), out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_student_distill_step_as_benchmarked(dtype):
    """train_step.StudentDistillStep as bench.py's C4 runs it (frozen teacher through the engine, student train forward with three
    heads, OHEM-CE + KLDiv evaluated from the low-resolution logits, flat-gradient sink, compute dtype) on the fixture's weights and
    batch, 2 x 3x256x512: loss and gradients against the reference's fp64 run of train/train.py:246-262 (tests/golden/student_step*).
    (The 128x256 fixture of test_ops_gpu normalises 4 samples per channel in its coarsest maps: fine for fp32, meaningless for bf16.)"""
    from fasterseg_amd.engine import InferenceEngine
    from fasterseg_amd.train_step import StudentDistillStep
    store = load_npz("student_step.npz")
    norms = load_json("student_step_gradnorms.json")
    bf16 = dtype == torch.bfloat16
    B, H, W = 2, 256, 512
    st = StudentDistillStep(B, H, W, lr=0.0, teacher_engine_dtype=None, compute_dtype=dtype)
    st.teacher.load_state_dict({k: v.cuda() for k, v in seeded_state(st.teacher.state_dict(), 12345).items()})
    st.student.load_state_dict({k: v.cuda() for k, v in seeded_state(st.student.state_dict(), 12346).items()})
    st.optimizer.refresh_packs()
    st.teacher_engine = InferenceEngine(st.teacher, (B, 3, H, W), dtype=dtype, output="lowres" if st.fused_loss else "logits")
    x = seeded_input((B, 3, H, W), 61).cuda()
    target = torch.tensor(store["target"].astype(np.int64)).cuda()
    loss = float(st.step(x, target))
    torch.cuda.synchronize()
    want = float(store["loss"][0])
    params = dict(st.student.named_parameters())
    assert set(norms) == {k for k, p in params.items() if p.grad is not None}, "same set of parameters receives gradients"
    errs = {k: abs(float(params[k].grad.float().norm()) - w) / (w + 1e-12) for k, w in norms.items()}
    cos_min, rel_max, per = 1.0, 0.0, {}
    for key in store:
        if key.startswith("g/"):
            pname = key[2:].split("@")[0]
            cos, rel = _cos_rel(params[pname].grad, store, "g/" + pname)
            per[pname] = (round(cos, 5), round(rel, 5))
            cos_min, rel_max = min(cos_min, cos), max(rel_max, rel)
    bar = 1.0 if bf16 else 3e-2
    missed = sorted(((e, k) for k, e in errs.items() if e > bar), reverse=True)
    _record("student_step_" + ("bf16" if bf16 else "fp32"), dict(loss=loss, want=want, loss_rel=abs(loss - want) / want, worst_norm_err=max(errs.values()),
                                                              norms_missed=len(missed), cos_min=cos_min, rel_l2_max=rel_max, per_tensor=per))
    assert abs(loss - want) <= (5e-3 if bf16 else 2e-3) * want, (loss, want)
    assert len(missed) <= (len(norms) // 20 if bf16 else 0), missed[:8]
    if bf16:
        assert cos_min >= 0.25 and all(c >= 0.99 for k, (c, _) in per.items() if k.startswith("heads8.conv_1x1")), per
    else:
        assert cos_min >= 0.999 and rel_max <= bar, per


class _SmallSearch:
    """The 6-layer supernet of the reference fixtures with the weight step's settings (config_search.py:57-58,71,90)."""
    lr = 2e-2
    momentum = 0.9
    weight_decay = 5e-4
    grad_clip = 5
    arch_learning_rate = 3e-4
    layers = 6
    Fch = 12
    width_mult_list = WML
    prun_modes = ['max', 'arch_ratio']
    stem_head_width = [(1, 1), (8. / 12, 8. / 12)]
    latency_weight = [0, 1e-2]


@pytest.mark.parametrize("unused", ["decay", "skip"])
def test_weight_update_trajectory_matches_reference(unused):
    """Three iterations of the reference's weight-update loop (search/train_search.py:244-250: `_loss` -> backward ->
    clip_grad_norm_(model.parameters(), 5) -> SGD) on one batch, run by the UNMODIFIED reference in fp64 (oracle/make_golden.py
    `trajectory`), against SupernetStep + FlatSGD in fp32.  "decay" = the reference's pinned torch 1.1 (zero-filled gradients of unused
    parameters keep decaying them), "skip" = today's torch.  Checked: the three losses, the clip norm of every step, the final value of
    13 tensors.  The clip norm here covers the network weights only (architecture parameters are frozen in the weight step): the
    fixture holds both norms and the difference is asserted to be below 1e-3 relative - the deviation stated in DESIGN.md."""
    from oracle.seeded import seeded_input, seeded_state
    from fasterseg_amd.optim import FlatSGD
    from fasterseg_amd.train_step import SupernetStep
    store = load_npz("optimizer_trajectory.npz")
    sem = "zeros" if unused == "decay" else "none"
    st = SupernetStep(pretrain=True, cfg=_SmallSearch, compute_dtype=torch.float32, use_graphs=False)
    sd = seeded_state(st.model.state_dict(), 777)
    for k in list(sd):
        if k.split("_")[0] in ("alpha", "beta", "ratio"):
            sd[k] = sd[k] * 5.0
    st.model.load_state_dict({k: v.cuda() for k, v in sd.items()})
    st.optimizer = FlatSGD(st.sync, _SmallSearch.lr, _SmallSearch.momentum, _SmallSearch.weight_decay, max_norm=_SmallSearch.grad_clip,
                           pack_dtype=torch.float32, unused=unused)
    st._prewarmed = True
    x = seeded_input((2, 3, 128, 256), 31).cuda()
    g = torch.Generator().manual_seed(32)
    target = torch.randint(0, 19, (2, 16, 32), generator=g)
    target[torch.rand(2, 16, 32, generator=g) < 0.05] = 255
    target = target.cuda()
    st.model.arch_idx = 0
    for step in range(3):
        np.random.seed(100 + step)
        torch.manual_seed(200 + step)
        loss, _ = st.step(x, target)
        want = float(store["%s/loss%d" % (sem, step)][0])
        assert abs(float(loss) - want) <= 2e-3 * abs(want), (step, float(loss), want)
        norm_w, norm_all = float(store["%s/norm_weights%d" % (sem, step)][0]), float(store["%s/norm_all%d" % (sem, step)][0])
        assert abs(norm_all - norm_w) <= 1e-3 * norm_all              # what excluding alpha / beta / ratio from the clip norm changes
        assert abs(float(st.optimizer.last_norm) - norm_w) <= 2e-2 * norm_w, (step, float(st.optimizer.last_norm), norm_w)
    params = dict(st.model.named_parameters())
    worst = 0.0
    names = sorted({k[len(sem) + 7:].split("@")[0] for k in store.keys() if k.startswith(sem + "/final/")})
    assert len(names) == 13
    for name in names:
        want_np, stride = golden_get(store, "%s/final/%s" % (sem, name))            # big tensors are stored as flat[::stride]
        want = torch.from_numpy(np.asarray(want_np)).float().reshape(-1)
        got = params[name].detach().float().cpu().reshape(-1)[::stride]
        # compare the UPDATE (final - initial), which is what the optimizer computed
        init = sd[name].float().reshape(-1)[::stride]
        du_want, du_got = want - init, got - init
        rel = float((du_got - du_want).norm() / (du_want.norm() + 1e-12))
        worst = max(worst, rel)
        # yardstick: what the reference's own fp32 run of the same three steps loses against its fp64 run on this tensor (7 % for
        # the stem, 1e-3 next to the heads: tiny-batch BatchNorm amplifies fp32 rounding)
        ref32 = float(store["ref_fp32_update_err/" + name][0])
        assert rel <= 3.0 * ref32 + 2e-2, (name, rel, ref32)
    print("trajectory %s: worst relative error of an update vs the reference's fp64 run %.3e" % (unused, worst))


class _Search(_FrozenLR):
    """search/config_search.py:57-59,71-73,97-99: the weight step's SGD(2e-2) and the arch step's Adam(3e-4) both move."""
    lr = 2e-2


def _adam_replay(names, store, tag, init):
    """The architecture parameters after each of the fixture's two arch steps, replayed with torch Adam on the stored `tag` gradients."""
    params = [torch.nn.Parameter(init[k].double().clone()) for k in names]
    opt = torch.optim.Adam(params, lr=_Search.arch_learning_rate, betas=(0.5, 0.999))
    out = []
    for it in (0, 1):
        for k, p in zip(names, params):
            key = "%s/it%d/arch_grad/%s" % (tag, it, k)
            p.grad = torch.from_numpy(store[key]).double() if key in store else None
        opt.step()
        out.append({k: p.detach().clone() for k, p in zip(names, params)})
    return out


def _cos_rel_vec(g, w):
    cos = float((g * w).sum() / (np.sqrt((g * g).sum() * (w * w).sum()) + 1e-300))
    return cos, float(np.sqrt(((g - w) ** 2).sum()) / (np.sqrt((w * w).sum()) + 1e-300))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_search_iteration_matches_reference(dtype):
    """Two full iterations of the search loop (train_search.py:225-250) at the C5 batch, 2 x 3x224x448, through SupernetStep as bench.py
    runs it (graphs, programs, joint passes, flat-gradient sink, Architect with the shipped 1080Ti latency table) against the unmodified
    reference in fp64 (tests/golden/search_iter_l16*, oracle/make_golden.py gen_search_iteration_l16).  Per iteration:
    * the architecture gradients the arch step leaves in .grad (822 values, 16 tensors; the three the reference leaves None must be None or
      zero): cosine and relative L2, concatenated and per tensor, against bars set by the reference's OWN fp32 run of the same iterations
      (rel <= 3 rel32 + 1e-2; cos >= 0.999 in iteration 1, where the fixture's weights give cos32 >= 0.9997; in iteration 2 - weights SGD
      has moved, alphas Adam has moved, fp32 itself drifts to cos32 0.98 - cos >= 1 - 9 (1 - cos32), the rel bar restated: 1 - cos ~ rel^2 / 2).
      One tensor, ratio_1_2 (the widths of the 1/32 cells of architecture 1), has a gradient of norm ~1e-5 against ~1 for the rest - a
      sum of terms that cancel - and the HIP step reproduces it to cosine 0.9955 / relative L2 9.5e-2 in iteration 1, where the
      reference's fp32 run has 0.99999 / 5e-3: its bar is cosine 0.99 and relative L2 0.25 (the concatenated vector is unaffected);
    * Adam: a first step is lr * sign(g), so where |g_ref| >= 1e-3 max|g_ref| of its tensor the step's sign must be the reference's
      (entries at 1e-12 carry a sign that is noise even between fp32 and fp64) - for all but 1 % of those 619 entries outside ratio_1_2
      and 10 % of ratio_1_2's (measured: 2 and 3 flips in two runs, 2 of them in ratio_1_2; the reference's fp32 run: 0); after
      iteration 2 the parameters on the entries masked in both iterations are within lr / 2 of the reference's, but for at most
      3x + 1 % of the entries the fp32 yardstick misses (it misses 20 of 607; measured 25);
    * the latency (PyTorch arithmetic on the table) at 1e-5, the arch `_loss`, the weight-step loss at 2e-3;
    * the clip norm: FlatSGD clips by the norm over the network weights, the reference by the norm over model.parameters(), which
      also counts the arch step's gradients still in .grad plus what the weight step's backward adds to them: the fixture's two norms
      differ by <= 1e-3 (measured 2.7e-4 and 3.7e-4), and last_norm is within 2e-2 of the weights-only one;
    * the update (after - before) of ten weights within 3x the fp32 yardstick + 2e-2.
    bf16: sanity bars - loss 5e-3, clip norm within 25 %, in iteration 1 concatenated cosine >= 0.25 and Adam signs for >= 60 % of the
    masked entries (three runs: 0.48-0.67 and 74-78 %; iteration 2: cosine 0.21-0.65 - the architecture gradients are sums over every cell,
    and bf16 storage under batch-2 BatchNorm moves deep-layer gradients by tens of per cent, module docstring)."""
    from fasterseg_amd import operations
    from fasterseg_amd.train_step import SupernetStep
    from oracle.seeded import search_iteration_batch
    bf16 = dtype == torch.bfloat16
    store = load_npz("search_iter_l16.npz")
    meta = load_json("search_iter_l16_meta.json")
    names = meta["arch_params"]
    saved_lut = dict(operations.latency_lookup_table)
    metrics = {}
    try:
        st = SupernetStep(pretrain=False, cfg=_Search, lut=load_json("latency_lut_1080ti.json"), compute_dtype=dtype)
        st._prewarmed = True
        init = _l16_state(st.model)
        st.model.load_state_dict({k: v.cuda() for k, v in init.items()})
        st.optimizer.refresh_packs()
        params = dict(st.model.named_parameters())
        assert sorted(names) == sorted(k for k in params if k.split("_")[0] in ("alpha", "beta", "ratio"))
        assert {id(params[k]) for k in names} == {id(p) for p in st.arch_params}
        ref64, ref32 = _adam_replay(names, store, "f64", init), _adam_replay(names, store, "f32", init)
        weight_keys = sorted({k.split("/", 3)[3].split("@")[0] for k in store if k.startswith("f64/it0/update/")})
        assert len(weight_keys) == 10
        st.model.arch_idx = 0
        before = {k: params[k].detach().double().cpu().clone() for k in names}
        masks = {}
        for it in (0, 1):
            imgs, tgt, imgs_s, tgt_s = [t.cuda() for t in search_iteration_batch(it, (2, 3, 224, 448))]
            np.random.seed(300 + it)
            torch.manual_seed(400 + it)
            loss, loss_arch = st.step(imgs, tgt, imgs_s, tgt_s)
            torch.cuda.synchronize()
            p_ = "f64/it%d/" % it
            m = metrics["it%d" % it] = {}
            want = {k: float(store[p_ + k][0]) for k in ("loss_arch", "arch_loss", "latency", "loss", "norm_all", "norm_weights")}
            got = dict(loss_arch=float(loss_arch), arch_loss=float(st.last_arch_ce), latency=float(st.architect.latency_supernet),
                       loss=float(loss), norm_weights=float(st.optimizer.last_norm))
            m.update({k + "_rel": abs(got[k] - want[k]) / abs(want[k]) for k in got})
            m["ref_clip_norm_gap"] = abs(want["norm_all"] - want["norm_weights"]) / want["norm_all"]
            # architecture gradients
            gs, ws, g32s, per = [], [], [], {}
            for k in names:
                g = params[k].grad
                key = p_ + "arch_grad/" + k
                if key not in store:
                    assert k in meta["it%d" % it]["arch_grad_none"]
                    assert g is None or not bool(g.any()), "%s: the reference leaves no gradient, SupernetStep has one" % k
                    continue
                assert g is not None, k
                gv, wv, w32 = g.detach().double().cpu().numpy().reshape(-1), store[key].reshape(-1), store["f32/it%d/arch_grad/%s" % (it, k)].reshape(-1)
                gs.append(gv), ws.append(wv), g32s.append(w32)
                cos, rel = _cos_rel_vec(gv, wv)
                cos32, rel32 = _cos_rel_vec(w32, wv)
                per[k] = (cos, rel, cos32, rel32)
            cos, rel = _cos_rel_vec(np.concatenate(gs), np.concatenate(ws))
            cos32, rel32 = _cos_rel_vec(np.concatenate(g32s), np.concatenate(ws))
            m.update(arch_grad_cos=cos, arch_grad_rel=rel, ref32_cos=cos32, ref32_rel=rel32,
                     per_tensor={k: tuple(round(v, 5) for v in c) for k, c in per.items()})
            # Adam
            after = {k: params[k].detach().double().cpu().clone() for k in names}
            for k in names:
                key = p_ + "arch_grad/" + k
                if key in store:
                    a = np.abs(store[key])
                    masks[k] = (a >= 1e-3 * a.max()) & masks.get(k, True)
            sign_bad, off, off32, n_masked = 0, 0, 0, 0
            for k, mk in masks.items():
                mk = torch.from_numpy(np.asarray(mk))
                if it == 0:
                    bad_k = int((torch.sign(after[k] - before[k]) != torch.sign(ref64[0][k] - before[k]))[mk].sum())
                    sign_bad += bad_k
                    if bad_k:
                        m.setdefault("adam_sign_mismatch_per_tensor", {})[k] = bad_k
                off += int(((after[k] - ref64[it][k]).abs() > 0.5 * _Search.arch_learning_rate)[mk].sum())
                off32 += int(((ref32[it][k] - ref64[it][k]).abs() > 0.5 * _Search.arch_learning_rate)[mk].sum())
                n_masked += int(mk.sum())
            m.update(adam_sign_mismatch=sign_bad, adam_off=off, adam_off_ref32=off32, adam_masked=n_masked)
            # weights after SGD
            upd = {}
            for k in weight_keys:
                du_np, stride = golden_get(store, p_ + "update/" + k)           # the reference's w after SGD - w0
                w0 = init[k].double().reshape(-1)[::stride]
                du_want = torch.from_numpy(du_np).double().reshape(-1)
                du_got = params[k].detach().double().cpu().reshape(-1)[::stride] - w0
                upd[k] = (float((du_got - du_want).norm() / (du_want.norm() + 1e-30)), float(store["f32/it%d/update_err/%s" % (it, k)][0]))
            m["update_err"] = upd
            _record("search_iter_%s" % ("bf16" if bf16 else "fp32"), metrics)
            assert m["ref_clip_norm_gap"] <= 1e-3, m["ref_clip_norm_gap"]
            if bf16:
                assert all(m[k + "_rel"] <= 5e-3 for k in ("loss_arch", "arch_loss", "loss")), m
                assert m["norm_weights_rel"] <= 0.25, m
                assert it > 0 or (cos >= 0.25 and sign_bad <= 0.4 * n_masked), m           # measured: cosine 0.48-0.67, 22-26 % of the signs
                assert m["latency_rel"] <= (1e-5 if it == 0 else 1e-3), m
            else:
                assert all(m[k + "_rel"] <= 2e-3 for k in ("loss_arch", "arch_loss", "loss")), m
                assert m["latency_rel"] <= 1e-5, m
                assert m["norm_weights_rel"] <= 2e-2, m
                cos_bar = (lambda c32: 0.999) if it == 0 else (lambda c32: 1 - 9 * (1 - c32))     # (1 - cos ~ rel^2 / 2)
                assert cos >= cos_bar(cos32) and rel <= 3 * rel32 + 1e-2, m
                big = float(np.sqrt(sum((w * w).sum() for w in ws)))
                for k, (c, r, c32, r32) in per.items():
                    if np.linalg.norm(store[p_ + "arch_grad/" + k]) >= 1e-3 * big:
                        assert c >= cos_bar(c32) and r <= 3 * r32 + 1e-2, (it, k, per[k])
                    else:       # ratio_1_2: a gradient 1e-5 of the others (see the docstring)
                        assert c >= min(0.99, cos_bar(c32)) and r <= max(0.25, 3 * r32 + 1e-2), (it, k, per[k])
                flips = m.get("adam_sign_mismatch_per_tensor", {})
                assert sum(n for k, n in flips.items() if k != "ratio_1_2") <= 0.01 * n_masked, m
                assert flips.get("ratio_1_2", 0) <= 0.1 * int(np.asarray(masks["ratio_1_2"]).sum()), m
                assert off <= 3 * off32 + 0.01 * n_masked, m
                for k, (e, e32) in upd.items():
                    assert e <= 3 * e32 + 2e-2, (it, k, e, e32)
            before = after
    finally:
        operations.latency_lookup_table.clear()
        operations.latency_lookup_table.update(saved_lut)
