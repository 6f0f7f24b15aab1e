"""Train-step level checks on MI355X: the hipGraph-replayed supernet passes reproduce the eager step, fused in-place weight
gradient accumulation equals the autograd path, and the student distillation step runs end to end and learns."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class SmallSearch:
    lr = 2e-2
    momentum = 0.9
    weight_decay = 5e-4
    grad_clip = 5
    arch_learning_rate = 3e-4
    layers = 5
    Fch = 12
    width_mult_list = [4. / 12, 6. / 12, 8. / 12, 10. / 12, 1.]
    prun_modes = ['max', 'arch_ratio']
    stem_head_width = [(1, 1), (8. / 12, 8. / 12)]
    latency_weight = [0, 1e-2]


def _batch():
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(2, 3, 128, 256, generator=g).cuda()
    tgt = torch.randint(0, 19, (2, 16, 32), generator=g)
    tgt[torch.rand(2, 16, 32, generator=g) < 0.05] = 255
    return imgs, tgt.cuda()


def _run(use_graphs, steps=3):
    from fasterseg_amd.train_step import SupernetStep
    st = SupernetStep(pretrain=True, cfg=SmallSearch, seed=11, use_graphs=use_graphs)
    imgs, tgt = _batch()
    np.random.seed(21)
    losses = [float(st.step(imgs, tgt)[0]) for _ in range(steps)]
    probe = {k: p.detach().float().cpu().clone() for k, p in st.model.named_parameters()
             if k in ("stem.0.0.conv.0.weight", "cells.1.0._op._ops.3.conv1.weight", "cells.2.1.downsample._ops.4.bn2.bn.4.weight",
                      "head02.0.conv_1x1.weight")}
    return losses, probe


def test_graphed_supernet_step_equals_eager():
    eager_losses, eager_w = _run(False)
    graph_losses, graph_w = _run(True)
    for a, b in zip(eager_losses, graph_losses):
        assert abs(a - b) <= 5e-3 * abs(a), (eager_losses, graph_losses)
    assert eager_losses[-1] < eager_losses[0]                  # three SGD steps on one batch reduce the loss
    for k in eager_w:
        rel = float((eager_w[k] - graph_w[k]).norm() / (eager_w[k].norm() + 1e-12))
        assert rel < 2e-2, (k, rel)


def test_graphed_l16_supernet_step_tracks_eager_over_24_steps():
    """a capture-path fault that only shows "from the 5th replay on" would pass the 3-step comparison above
    and bench.py's step-0 gate.  The benchmarked configuration itself - F12.L16, 3 x 3x256x512, bf16, default switches - stepped 12 times
    from its hipGraphs and 12 times eagerly from the same seeds: every loss finite, the two trajectories side by side (float atomics and
    grouped-vs-single launches reorder sums, tiny-batch BatchNorm amplifies that: the bar is one per cent, an inf / NaN / runaway
    replay is orders of magnitude), probe weights finite and close.  Round 6: the default capture layout is now the one rounds 4-5 had to
    refuse (layer calls on the capture's origin stream, FS_GROUP_CAPTURE=1 - the fault was hipMemsetAsync nodes), so
    this runs 24 replays of it (>= 20)."""
    from fasterseg_amd.train_step import SupernetStep

    def run(use_graphs):
        st = SupernetStep(pretrain=True, seed=11, use_graphs=use_graphs, compute_dtype=torch.bfloat16)
        g = torch.Generator().manual_seed(3)
        imgs = torch.randn(3, 3, 256, 512, generator=g).cuda()
        tgt = torch.randint(0, 19, (3, 32, 64), generator=g)
        tgt[torch.rand(3, 32, 64, generator=g) < 0.05] = 255
        tgt = tgt.cuda()
        np.random.seed(21)
        losses = []
        for _ in range(24):
            losses.append(float(st.step(imgs, tgt)[0]))
            assert bool(torch.isfinite(st.sync.flat).all()), ("non-finite gradient after step %d" % len(losses), use_graphs, losses)
        probe = {k: p.detach().float().cpu().clone() for k, p in st.model.named_parameters()
                 if k in ("stem.0.0.conv.0.weight", "cells.3.1._op._ops.3.conv1.weight", "cells.9.2._op._ops.1.conv1.weight", "head02.0.conv_1x1.weight")}
        del st
        torch.cuda.empty_cache()
        return losses, probe
    graph_losses, graph_w = run(True)
    eager_losses, eager_w = run(False)
    assert all(np.isfinite(graph_losses)) and all(np.isfinite(eager_losses)), (graph_losses, eager_losses)
    worst = max(abs(a - b) / abs(a) for a, b in zip(eager_losses, graph_losses))
    print("24-step L16 trajectories: eager %s\n graphed %s\n worst relative gap %.3e" % (eager_losses, graph_losses, worst))
    assert worst <= 1e-2, (worst, eager_losses, graph_losses)          # measured 5.4e-4 (profiles/r05_gpu_tests.log)
    assert min(graph_losses[-3:]) < graph_losses[0]                   # it trains
    assert len(graph_w) == 4
    for k in graph_w:
        assert bool(torch.isfinite(graph_w[k]).all()), k
        rel = float((eager_w[k] - graph_w[k]).norm() / (eager_w[k].norm() + 1e-12))
        assert rel < 0.15, (k, rel)


def test_deterministic_mode_makes_supernet_steps_bit_identical():
    """kernels.deterministic() (fs_set_deterministic): two fresh builds of the graphed pretrain step - fused MixedOp programs, eager
    lanes, pair batching and all - on the same batch and seeds produce the SAME bits: losses of three consecutive SGD steps and the
    updated weights.  (Default mode: weight-gradient slabs and large-map BatchNorm reductions use float atomics, whose order varies.)"""
    from fasterseg_amd import kernels as K
    with K.deterministic():
        a_losses, a_w = _run(True)
        b_losses, b_w = _run(True)
    assert a_losses == b_losses, (a_losses, b_losses)
    for k in a_w:
        assert torch.equal(a_w[k], b_w[k]), k


def _run_search(use_graphs, steps=2):
    import json
    import os
    from fasterseg_amd.train_step import SupernetStep
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latency_lut_1080ti.json")) as f:
        lut = json.load(f)
    st = SupernetStep(pretrain=False, cfg=SmallSearch, seed=11, use_graphs=use_graphs, lut=lut)
    imgs, tgt = _batch()
    imgs_s, tgt_s = imgs.flip(3).contiguous(), tgt.flip(2).contiguous()
    init = [p.detach().cpu().clone() for p in st.arch_params]
    np.random.seed(21)
    torch.manual_seed(22)                      # Gumbel noise of the arch_ratio passes comes from the host generator
    out = [st.step(imgs, tgt, imgs_s, tgt_s) for _ in range(steps)]
    losses = [(float(a), float(b)) for a, b in out]
    delta = torch.cat([(p.detach().cpu() - i).reshape(-1) for p, i in zip(st.arch_params, init)])
    return losses, delta


def test_graphed_search_step_equals_eager():
    """Architecture step + weight step with the six fixed-width passes replayed from hipGraphs vs the plain eager
    Architect.step / _loss sequence: same losses, same Adam updates of alpha/beta/ratio."""
    eager_losses, eager_delta = _run_search(False)
    graph_losses, graph_delta = _run_search(True)
    for (a, la), (b, lb) in zip(eager_losses, graph_losses):
        assert abs(a - b) <= 5e-3 * abs(a) and abs(la - lb) <= 5e-3 * abs(la), (eager_losses, graph_losses)
    assert float(eager_delta.abs().max()) > 1e-4               # Adam moved the architecture parameters
    differing = float(((eager_delta - graph_delta).abs() > 1e-4).float().mean())
    assert differing < 0.05, differing


def test_fused_weight_grad_accumulation_matches_autograd():
    """FlatGradientSync makes the wgrad kernel accumulate in place into [O][R][S][I]-stored .grad views; the result must equal
    the plain autograd path (fresh gradient tensors + accumulate)."""
    from fasterseg_amd import archs
    from fasterseg_amd.parallel import FlatGradientSync
    torch.manual_seed(0)
    x = torch.randn(2, 3, 64, 128, device="cuda")
    grads = []
    for fused in (False, True):
        net = archs.init_weight(archs.build_derived(1, training=True), 5).cuda().train()
        sync = FlatGradientSync(net.parameters()) if fused else None
        if sync:
            sync.prepare()
        p8, p16, p32 = net(x)
        (p8.square().mean() + p16.square().mean() + p32.square().mean()).backward()
        if sync:
            sync.sync()
            assert net.ffm.channel_attention[1].conv.weight.grad is None        # never used -> hidden from the optimizer
        grads.append({k: p.grad.detach().float().cpu().contiguous().clone() for k, p in net.named_parameters() if p.grad is not None})
    assert set(grads[0]) == set(grads[1])
    bad = [k for k in grads[0] if float((grads[0][k] - grads[1][k]).norm() / (grads[0][k].norm() + 1e-12)) > 3e-2]
    assert not bad, bad[:5]


WIDTHS = [4. / 12, 6. / 12, 8. / 12, 10. / 12, 1.]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("phase", ["w", "a"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
def test_mixed_op_program_matches_module_path(stride, phase, dtype, fused):
    """The launch program of a MixedOp (fs_exec_program) against the per-module autograd path on the same inputs: output,
    dx, d alpha, every parameter gradient (through the flat buffer) and the BN running statistics.  fused: the pairs' storage is
    made adjacent (fusion.colocate / flat_order), so the program evaluates 'conv' + 'conv_2x'.conv1 and 'conv_downup' +
    'conv_2x_downup'.conv1 as one two-segment conv -> BN unit each (and one shared down-sample) - the module path does not."""
    import copy
    from fasterseg_amd import fusion
    from fasterseg_amd import kernels as K
    from fasterseg_amd import model_search
    from fasterseg_amd.parallel import FlatGradientSync
    torch.manual_seed(3)
    m = model_search.MixedOp(48, 48 * stride, stride=stride, width_mult_list=WIDTHS).cuda().train()
    for p in m.parameters():
        if p.dim() == 1:
            p.data.uniform_(0.5, 1.5)
    if fused:
        assert fusion.colocate(m) == 2 * len(WIDTHS)
    state0 = copy.deepcopy(m.state_dict())
    sync = FlatGradientSync(fusion.flat_order(m, m.parameters()) if fused else m.parameters())
    x0 = K.to_nhwc(torch.randn(2, 32, 16, 24, device="cuda"), dtype)
    coef0 = torch.softmax(torch.randn(5, device="cuda"), 0)
    dy0 = K.to_nhwc(torch.randn(2, 40 * stride, 16 // stride, 24 // stride, device="cuda"), dtype)
    got = []
    saved_flag = model_search._PROGRAMS
    try:
        for use_program in (False, True):
            model_search._PROGRAMS = use_program
            m.load_state_dict(state0)
            for p in m.parameters():
                p.requires_grad_(phase == "w")
            if phase == "w":
                sync.prepare()
            x = x0.clone().requires_grad_(True)
            coef = coef0.clone().requires_grad_(phase == "a")
            out = m(x, coef, (8. / 12, 10. / 12))
            assert (type(out.grad_fn).__name__ == "_MixedOpProgramBackward") == use_program
            if use_program:
                assert all(pr.fused == fused for pr in m.__dict__["_programs"].values()), "program fusion state"
            out.backward(dy0)
            rec = {"out": out.detach().float().clone(), "dx": x.grad.float().clone()}
            if phase == "a":
                rec["dcoef"] = coef.grad.clone()
            else:
                sync.sync()
                rec["flat"] = sync.flat.clone()
                rec["touched"] = list(sync._touched)
            rec["running"] = torch.cat([b.float().reshape(-1) for n, b in m.named_buffers()])
            got.append(rec)
    finally:
        model_search._PROGRAMS = saved_flag
        for p in m.parameters():
            p.requires_grad_(True)
    ref, new = got
    # fp32: same kernels on both sides, but the BN statistics of the larger maps come from float atomics whose order varies
    # from run to run; a last-bit change of a mean can flip one ReLU-mask element (~1e-3 of a tensor's norm), typical 1e-5
    tol = 3e-3 if dtype == torch.float32 else 3e-2
    for k in ref:
        if k == "touched":
            assert ref[k] == new[k]
            continue
        rel = float((ref[k] - new[k]).norm() / (ref[k].norm() + 1e-12))
        assert rel < tol, (k, rel)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("use_program", [False, True], ids=["modules", "program"])
@pytest.mark.parametrize("geom", [(1, 16, 24), (2, 16, 24), (1, 32, 48)], ids=["s1-small", "s2-small", "s1-large"])
def test_mixed_op_on_batched_pair_equals_two_evaluations(geom, use_program, dtype):
    """One evaluation of a MixedOp on two inputs concatenated along the batch with functional.bn_groups(2) against the
    reference's two evaluations one after the other (model_search.py:322-329): both outputs, both input gradients, d alpha,
    all parameter gradients (sum of the two) and the BN running statistics / counters after the two sequential updates.
    The large geometry (768 px per group at full size, 192 after stride 2 / zoom) exercises the grid-wide grouped BN passes."""
    import copy
    from fasterseg_amd import functional as FN
    from fasterseg_amd import kernels as K
    from fasterseg_amd import model_search
    from fasterseg_amd.parallel import FlatGradientSync
    stride, H, W = geom
    torch.manual_seed(5)
    m = model_search.MixedOp(48, 48 * stride, stride=stride, width_mult_list=WIDTHS).cuda().train()
    for p in m.parameters():
        if p.dim() == 1:
            p.data.uniform_(0.5, 1.5)
    state0 = copy.deepcopy(m.state_dict())
    sync = FlatGradientSync(m.parameters())
    n = 1 if H > 16 else 2
    xa = K.to_nhwc(torch.randn(n, 32, H, W, device="cuda"), dtype)
    xb = K.to_nhwc(torch.randn(n, 32, H, W, device="cuda") * 2.0 + 0.5, dtype)          # different statistics per input
    coef0 = torch.softmax(torch.randn(5, device="cuda"), 0)
    dya = K.to_nhwc(torch.randn(n, 40 * stride, H // stride, W // stride, device="cuda"), dtype)
    dyb = K.to_nhwc(torch.randn(n, 40 * stride, H // stride, W // stride, device="cuda"), dtype)
    saved_flag = model_search._PROGRAMS
    got = []
    try:
        model_search._PROGRAMS = use_program
        for batched in (False, True):
            m.load_state_dict(state0)
            sync.prepare(passes=2)
            a, b = xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)
            coef = coef0.clone().requires_grad_(True)
            if batched:
                with FN.bn_groups(2):
                    out = m(FN.batch_pair(a, b), coef, (8. / 12, 10. / 12))
                assert (type(out.grad_fn).__name__ == "_MixedOpProgramBackward") == use_program
                out.backward(torch.cat([dya, dyb], 0))
                oa, ob = out[:n], out[n:]
            else:
                oa = m(a, coef, (8. / 12, 10. / 12))
                ob = m(b, coef, (8. / 12, 10. / 12))
                torch.autograd.backward([oa, ob], [dya, dyb])
            sync.sync()
            got.append({"oa": oa.detach().float().clone(), "ob": ob.detach().float().clone(), "da": a.grad.float().clone(),
                        "db": b.grad.float().clone(), "dcoef": coef.grad.clone(), "flat": sync.flat.clone(),
                        "touched": list(sync._touched),
                        "running": torch.cat([t.float().reshape(-1) for _, t in m.named_buffers()])})
    finally:
        model_search._PROGRAMS = saved_flag
    ref, new = got
    # fp32: the maps above 512 pixels per group take their BN statistics from float atomics in both runs (different kernels,
    # different order), and a last-bit change of a mean can flip a ReLU mask element: 2e-4 typically, 1.6e-3 seen once
    tol = 5e-3 if dtype == torch.float32 else 3e-2
    for k in ref:
        if k == "touched":
            assert ref[k] == new[k]
            continue
        rel = float((ref[k] - new[k]).norm() / (ref[k].norm() + 1e-12))
        assert rel < tol, (k, rel)


def test_supernet_pair_batching_equals_sequential_evaluation():
    """Eager pretrain steps with every doubly-fed cell evaluated once on the batched pair (FS_PAIR_BATCH, default) vs the two
    evaluations one after the other."""
    from fasterseg_amd import model_search
    saved_flag = model_search._PAIR_BATCH
    try:
        model_search._PAIR_BATCH = False
        ref_losses, ref_w = _run(False)
        model_search._PAIR_BATCH = True
        new_losses, new_w = _run(False)
    finally:
        model_search._PAIR_BATCH = saved_flag
    for a, b in zip(ref_losses, new_losses):
        assert abs(a - b) <= 5e-3 * abs(a), (ref_losses, new_losses)
    for k in ref_w:
        rel = float((ref_w[k] - new_w[k]).norm() / (ref_w[k].norm() + 1e-12))
        assert rel < 2e-2, (k, rel)


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphed"])
def test_direct_pair_buffers_and_grouped_merges_equal_the_copying_path(use_graphs):
    """Round 6: the producers of a doubly-fed cell's two inputs write into the halves of the joint buffer (no copy launches) and a layer's
    beta merges are one grouped launch - against round 5's two copies per pair and one merge launch per output, eager and captured."""
    from fasterseg_amd import model_search
    saved = (model_search._PAIR_DIRECT, model_search._MERGE_GROUP)
    try:
        model_search._PAIR_DIRECT = model_search._MERGE_GROUP = False
        ref_losses, ref_w = _run(use_graphs)
        model_search._PAIR_DIRECT = model_search._MERGE_GROUP = True
        new_losses, new_w = _run(use_graphs)
    finally:
        model_search._PAIR_DIRECT, model_search._MERGE_GROUP = saved
    for a, b in zip(ref_losses, new_losses):
        assert abs(a - b) <= 5e-3 * abs(a), (ref_losses, new_losses)
    for k in ref_w:
        rel = float((ref_w[k] - new_w[k]).norm() / (ref_w[k].norm() + 1e-12))
        assert rel < 2e-2, (k, rel)


def _run_joint(pretrain, use_graphs, joint, steps=3, widths=None, stem_share=False):
    """`steps` supernet steps with adjacent passes evaluated together (joint) or one after the other; returns the losses, probe weights and
    BatchNorm running statistics (the state two passes share).  widths: width_mult_list override (one width: every "random" draw of
    the two random passes meets in the same BatchNorms - the conflict path of the layer calls)."""
    from fasterseg_amd import train_step
    cfg = SmallSearch if widths is None else type("Cfg", (SmallSearch,), dict(width_mult_list=widths))
    from fasterseg_amd import model_search
    saved = train_step._JOINT_PASSES
    saved_stem = model_search._STEM_SHARE
    try:
        train_step._JOINT_PASSES = joint
        model_search._STEM_SHARE = bool(stem_share)
        lut = None
        if not pretrain:
            import json
            import os
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latency_lut_1080ti.json")) as f:
                lut = json.load(f)
        st = train_step.SupernetStep(pretrain=pretrain, cfg=cfg, seed=11, use_graphs=use_graphs, lut=lut)
        assert any(len(g) > 1 for g in st._groups()) == bool(joint)
        init = [p.detach().cpu().clone() for p in st.arch_params]
        imgs, tgt = _batch()
        np.random.seed(21)
        torch.manual_seed(21)
        losses = []
        for _ in range(steps):
            out = st.step(imgs, tgt, imgs, tgt)
            losses.append((float(out[0]), None if out[1] is None else float(out[1])))
    finally:
        train_step._JOINT_PASSES = saved
        model_search._STEM_SHARE = saved_stem
    probe = {k: p.detach().float().cpu().clone() for k, p in st.model.named_parameters()
             if k in ("stem.0.0.conv.0.weight", "cells.1.0._op._ops.3.conv1.weight", "cells.2.1.downsample._ops.4.bn2.bn.4.weight",
                      "cells.2.1.downsample._ops.4.bn2.bn.0.weight", "head02.0.conv_1x1.weight")}
    probe["arch_delta"] = torch.cat([(p.detach().cpu() - i).reshape(-1) for p, i in zip(st.arch_params, init)])
    stats = {k: b.detach().double().cpu().clone() for k, b in st.model.named_buffers() if "cells.2." in k or "cells.3.0" in k or k.startswith("stem.")}
    return losses, probe, stats


@pytest.mark.parametrize("pretrain,use_graphs,widths", [(True, False, None), (True, True, None), (False, True, None), (False, False, None),
                                                         (True, False, [8. / 12, 1.]), (True, True, [8. / 12, 1.])],
                         ids=["pretrain-eager", "pretrain-graphed", "search-graphed", "search-eager", "two-widths-eager", "two-widths-graphed"])
def test_joint_passes_equal_sequential_passes(pretrain, use_graphs, widths):
    """Round 6: adjacent passes of `_loss` evaluated together layer by layer (Network_Multi_Path.forward_multi: max + min as one captured
    graph, random + random as one eager joint pass) against pass-after-pass evaluation from the same seeds: losses, updated weights and
    architecture parameters, and - the state passes share - every BatchNorm's running statistics and update count.  With two
    widths the two random passes draw the same width for most MixedOps: those evaluations must not share a grouped launch
    (conflict_free_chunks), or a running-statistics update is lost."""
    ref_losses, ref_w, ref_stats = _run_joint(pretrain, use_graphs, False, widths=widths)
    new_losses, new_w, new_stats = _run_joint(pretrain, use_graphs, True, widths=widths)
    for a, b in zip(ref_losses, new_losses):
        for x, y in zip(a, b):
            if x is not None:
                assert abs(x - y) <= 5e-3 * abs(x), (ref_losses, new_losses)
    ref_delta, new_delta = ref_w.pop("arch_delta"), new_w.pop("arch_delta")
    for k in ref_w:
        rel = float((ref_w[k] - new_w[k]).norm() / (ref_w[k].norm() + 1e-12))
        assert rel < 2e-2, (k, rel)
    if not pretrain:            # Adam's steps follow the gradient's sign pattern: the same criterion as test_graphed_search_step_equals_eager
        assert float(ref_delta.abs().max()) > 1e-4
        differing = float(((ref_delta - new_delta).abs() > 1e-4).float().mean())
        assert differing < 0.05, differing
    assert ref_stats.keys() == new_stats.keys() and len(ref_stats) > 50
    for k in ref_stats:
        if k.endswith("num_batches_tracked"):
            assert torch.equal(ref_stats[k], new_stats[k]), k          # every BatchNorm saw the same number of momentum updates
        else:
            rel = float((ref_stats[k] - new_stats[k]).norm() / (ref_stats[k].norm() + 1e-9))
            assert rel < 2e-2, (k, rel)


@pytest.mark.parametrize("pretrain,use_graphs", [(True, False), (True, True), (False, True)], ids=["pretrain-eager", "pretrain-graphed", "search-graphed"])
def test_shared_stem_of_a_pass_pair_equals_per_pass_stems(pretrain, use_graphs):
    """FS_STEM_SHARE=1 (opt-in): the two passes of a pair feed the same images through the same stem - evaluated once, its BatchNorms given
    the second pass's momentum update in closed form (r2 = r1 + (1 - m)(r1 - r0), num_batches_tracked += 1), the two passes' gradients of its
    output added before its one backward.  Losses, weights and the stem's running statistics equal pass-after-pass evaluation."""
    ref_losses, ref_w, ref_stats = _run_joint(pretrain, use_graphs, False)
    new_losses, new_w, new_stats = _run_joint(pretrain, use_graphs, True, stem_share=True)
    for a, b in zip(ref_losses, new_losses):
        for x, y in zip(a, b):
            if x is not None:
                assert abs(x - y) <= 5e-3 * abs(x), (ref_losses, new_losses)
    ref_w.pop("arch_delta"), new_w.pop("arch_delta")
    for k in ref_w:
        assert float((ref_w[k] - new_w[k]).norm() / (ref_w[k].norm() + 1e-12)) < 2e-2, k
    stem = [k for k in ref_stats if k.startswith("stem.")]
    assert len(stem) >= 10
    for k in stem:
        if k.endswith("num_batches_tracked"):
            assert torch.equal(ref_stats[k], new_stats[k]), k
        else:
            assert float((ref_stats[k] - new_stats[k]).norm() / (ref_stats[k].norm() + 1e-9)) < 2e-2, k


def _ohem_kept(pred, target, thresh, min_kept):
    """(valid, kept) pixel counts of ProbOhemCrossEntropy2d's selection (loss_opr.py:70-93), restated in torch on the host."""
    prob = torch.softmax(pred.detach().double().cpu(), 1)
    t = target.cpu().reshape(-1)
    valid = t.ne(255)
    true_prob = prob.permute(1, 0, 2, 3).reshape(prob.shape[1], -1).gather(0, (t * valid).unsqueeze(0)).squeeze(0).masked_fill(~valid, 1)
    threshold = max(thresh, float(torch.sort(true_prob).values[min(true_prob.numel(), min_kept) - 1]))
    return int(valid.sum()), int((valid & true_prob.le(threshold)).sum())


def test_joint_tail_with_a_per_call_criterion_equals_pass_by_pass(monkeypatch):
    """The joint tail (forward_multi with batch_tails) returns the two passes' logits concatenated along the batch.  Pooling them into one
    criterion call equals the sum of two calls only for plain mean cross-entropy; OHEM (the reference's supernet criterion,
    train_search.py:62-66) selects pixels per call.  With losses.ProbOhemCrossEntropy2d on model._criterion, one eager pretrain step - both
    pass pairs (max + min, random + random) through the joint tail - gives the loss and gradients of pass-by-pass evaluation
    (_JOINT_PASSES = False) from the same seeds.  thresh / min_kept: at this initialisation every pixel's true-class probability is far
    below the reference's 0.7 (median ~0.035), so that threshold keeps every pixel and pools like CE; with thresh 0.01 the selection is
    made by min_kept (the 256 hardest of ~970 valid pixels per call), which pooling halves per pass."""
    from fasterseg_amd import losses, model_search, train_step
    thresh, min_kept = 0.01, 256
    monkeypatch.setattr(model_search, "_TAIL_BATCH", True)

    class Recording(losses.ProbOhemCrossEntropy2d):
        def forward(self, pred, target):
            self.calls.append((pred.detach().float().clone(), target.clone()))
            return super().forward(pred, target)

    cfg = type("Cfg", (SmallSearch,), dict(lr=0.0))
    probes = ("stem.0.0.conv.0.weight", "cells.1.0._op._ops.3.conv1.weight", "cells.2.1.downsample._ops.4.bn2.bn.4.weight",
              "head02.0.conv_1x1.weight", "head0.0.conv_1x1.bias")
    res = {}
    for joint in (False, True):
        monkeypatch.setattr(train_step, "_JOINT_PASSES", joint)
        st = train_step.SupernetStep(pretrain=True, cfg=cfg, seed=11, use_graphs=False)
        st._prewarmed = True
        assert [len(g) for g in st._groups()] == ([2, 2] if joint else [1, 1, 1, 1])
        crit = Recording(ignore_label=255, thresh=thresh, min_kept=min_kept)
        crit.calls = []
        st.model._criterion = crit
        imgs, tgt = _batch()
        np.random.seed(21)
        torch.manual_seed(21)
        loss = float(st.step(imgs, tgt)[0])
        params = dict(st.model.named_parameters())
        res[joint] = (loss, {k: params[k].grad.detach().double().cpu().clone() for k in probes}, crit.calls)
    (seq_loss, seq_g, seq_calls), (joint_loss, joint_g, joint_calls) = res[False], res[True]
    assert len(seq_calls) == 20 and all(c[0].shape[0] == 2 for c in seq_calls)
    for pred, target in seq_calls:                # OHEM is selecting: a proper subset of the valid pixels is kept, in every call
        valid, kept = _ohem_kept(pred, target, thresh, min_kept)
        assert min_kept <= kept < valid, (valid, kept)
    assert abs(joint_loss - seq_loss) <= 1e-3 * abs(seq_loss), (joint_loss, seq_loss)
    for k in probes:
        rel = float((joint_g[k] - seq_g[k]).norm() / (seq_g[k].norm() + 1e-12))
        assert rel < 2e-2, (k, rel)
    assert len(joint_calls) == 20 and all(c[0].shape[0] == 2 for c in joint_calls), "the criterion saw the logits of two passes at once"


@pytest.mark.parametrize("pretrain", [True, False], ids=["pretrain", "search"])
def test_dp_overlap_bookkeeping_of_the_last_eager_group_changes_nothing(pretrain):
    """Under DP the gradient buckets leave under the backward of the step's last EAGER group (FlatGradientSync.final_pass; in the search
    step that group's backward is issued after the graph replays that follow it).  FS_DP_OVERLAP=2 runs the bookkeeping on a single
    rank: buckets are declared complete before sync() (early_launches), and losses, weights, architecture parameters and BatchNorm
    statistics equal the step without it."""
    from fasterseg_amd import train_step
    saved = train_step._DP_OVERLAP
    res = {}
    try:
        for mode in (0, 2):
            train_step._DP_OVERLAP = mode
            lut = None
            if not pretrain:
                import json
                import os
                with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "latency_lut_1080ti.json")) as f:
                    lut = json.load(f)
            st = train_step.SupernetStep(pretrain=pretrain, cfg=SmallSearch, seed=11, use_graphs=True, lut=lut, bucket_mb=1)   # several buckets
            imgs, tgt = _batch()
            np.random.seed(21)
            torch.manual_seed(21)
            losses, early = [], []
            for _ in range(3):
                out = st.step(imgs, tgt, imgs, tgt)
                losses.append(float(out[0]))
                early.append(st.sync.early_launches)
            res[mode] = (losses, early, len(st.sync.buckets),
                         {k: p.detach().float().cpu().clone() for k, p in st.model.named_parameters()
                          if k in ("stem.0.0.conv.0.weight", "cells.1.0._op._ops.3.conv1.weight", "cells.2.1.downsample._ops.4.bn2.bn.4.weight",
                                   "head02.0.conv_1x1.weight") or k.startswith("alpha")},
                         {k: b.detach().double().cpu().clone() for k, b in st.model.named_buffers() if "cells.2." in k})
    finally:
        train_step._DP_OVERLAP = saved
    (l0, e0, nb, w0, s0), (l2, e2, _, w2, s2) = res[0], res[2]
    assert nb > 2 and all(e == 0 for e in e0)
    assert all(1 <= e <= nb for e in e2[1:]), (e2, nb)          # (the first step captures its graphs: hooks are off inside a capture)
    for a, b in zip(l0, l2):
        assert abs(a - b) <= 5e-3 * abs(a), (l0, l2)
    for k in w0:
        rel = float((w0[k] - w2[k]).norm() / (w0[k].norm() + 1e-12))
        assert rel < (0.1 if k.startswith("alpha") else 2e-2), (k, rel)
    for k in s0:
        if k.endswith("num_batches_tracked"):
            assert torch.equal(s0[k], s2[k]), k
        else:
            assert float((s0[k] - s2[k]).norm() / (s0[k].norm() + 1e-9)) < 2e-2, k


def test_prewarmed_programs_cover_every_random_width_draw():
    """After the first graphed step SupernetStep.prewarm_programs() has lowered every width combination of every MixedOp call
    site: later steps, whose "random" passes draw new widths each time, build no further program."""
    from fasterseg_amd import model_search
    from fasterseg_amd.train_step import SupernetStep
    st = SupernetStep(pretrain=True, cfg=SmallSearch, seed=11, use_graphs=True)
    imgs, tgt = _batch()
    np.random.seed(21)
    st.step(imgs, tgt)
    assert st.programs_prewarmed > 0
    mixed = [m for m in st.model.modules() if isinstance(m, model_search.MixedOp)]
    count = lambda: sum(len(m.__dict__.get("_programs", {})) for m in mixed)
    n0 = count()
    nw = len(SmallSearch.width_mult_list)
    assert n0 >= len(mixed) * nw, (n0, len(mixed))          # at least one sampled ratio per MixedOp
    losses = [float(st.step(imgs, tgt)[0]) for _ in range(4)]
    assert count() == n0, "a random-width pass lowered a program after the prewarm"
    assert all(np.isfinite(losses))


def test_supernet_step_with_programs_equals_module_path():
    """Eager pretrain steps (all four passes, random widths included) with the MixedOp programs vs the per-module path."""
    from fasterseg_amd import model_search
    saved_flag = model_search._PROGRAMS
    try:
        model_search._PROGRAMS = False
        ref_losses, ref_w = _run(False)
        model_search._PROGRAMS = True
        new_losses, new_w = _run(False)
    finally:
        model_search._PROGRAMS = saved_flag
    for a, b in zip(ref_losses, new_losses):
        assert abs(a - b) <= 5e-3 * abs(a), (ref_losses, new_losses)
    for k in ref_w:
        rel = float((ref_w[k] - new_w[k]).norm() / (ref_w[k].norm() + 1e-12))
        assert rel < 2e-2, (k, rel)


def test_flat_sgd_matches_torch_sgd_with_clip():
    """fs_sgd_momentum_multi over the flat buffers == clip_grad_norm_ + torch.optim.SGD(momentum, weight_decay) fed the same
    gradients, including parameters that receive no gradient (skipped) and the [O][R][S][I] gradient storage of filters."""
    from fasterseg_amd import archs
    from fasterseg_amd import functional as FN
    from fasterseg_amd.optim import FlatSGD
    from fasterseg_amd.parallel import FlatGradientSync
    torch.manual_seed(1)
    net = archs.init_weight(archs.build_derived(1, training=True), 5).cuda().train()
    sync = FlatGradientSync(net.parameters())
    opt = FlatSGD(sync, 0.05, 0.9, 5e-4, max_norm=0.5)
    ref = [p.detach().clone().requires_grad_(True) for p in sync.params]
    ref_opt = torch.optim.SGD(ref, lr=0.05, momentum=0.9, weight_decay=5e-4)
    x = torch.randn(2, 3, 64, 128, device="cuda")
    for step in range(3):
        sync.prepare()
        p8, p16, p32 = net(x)
        (p8.square().mean() + p16.square().mean() + 3 * p32.square().mean()).backward()
        sync.sync()
        for r, p in zip(ref, sync.params):
            r.grad = None if p.grad is None else p.grad.detach().clone().contiguous()
        assert any(r.grad is None for r in ref)
        norm_ref = torch.nn.utils.clip_grad_norm_(ref, 0.5)
        ref_opt.step()
        norm = opt.step()
        assert abs(float(norm) - float(norm_ref)) <= 1e-4 * float(norm_ref)
        assert float(norm_ref) > 0.5 or step > 0                 # the clip is active at least on the first step
        worst = max(float((r.detach() - p.detach()).abs().max()) for r, p in zip(ref, sync.params))
        assert worst < 2e-6, (step, worst)
        w = net.stem[0].conv[0].weight
        assert torch.equal(FN.packed_weight(w, torch.float32).reshape(w.shape[0], 3, 3, w.shape[1]), w.detach().permute(0, 2, 3, 1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_resident_packs_follow_the_optimizer(dtype):
    """FlatSGD(pack_dtype=...) rewrites the packed filter copies inside the update kernel: after every step they equal a
    fresh fs_pack_weight of the updated parameter (forward and flipped), and an in-place edit of the parameter invalidates
    them."""
    from fasterseg_amd import archs
    from fasterseg_amd import functional as FN
    from fasterseg_amd import kernels as K
    from fasterseg_amd.optim import FlatSGD
    from fasterseg_amd.parallel import FlatGradientSync
    torch.manual_seed(2)
    net = archs.init_weight(archs.build_derived(1, training=True), 5).cuda().train()
    sync = FlatGradientSync(net.parameters())
    opt = FlatSGD(sync, 0.05, 0.9, 5e-4, max_norm=1.0, pack_dtype=dtype)
    x = torch.randn(2, 3, 64, 128, device="cuda")
    convs = [p for p in sync.params if p.dim() == 4 and p.shape[0] % 8 == 0 and p.shape[1] % 8 == 0]
    assert len(convs) > 20
    FN.set_compute_dtype(dtype)
    try:
        for step in range(3):
            for w in convs[::7]:
                fwd, flip = FN.resident_pack(w, dtype)
                assert torch.equal(fwd, K.pack_weight(w.detach(), dtype)) and torch.equal(flip, K.pack_weight(w.detach(), dtype, flip=True))
            sync.prepare()
            p8, p16, p32 = net(x)
            (p8.float().square().mean() + p16.float().square().mean() + p32.float().square().mean()).backward()
            sync.sync()
            before = convs[0].detach().clone()
            opt.step()
            assert not torch.equal(before, convs[0].detach())
    finally:
        FN.set_compute_dtype(torch.float32)
    convs[0].data.mul_(1.0)                   # out-of-band edit: version bump -> the resident pack is no longer trusted
    with torch.no_grad():
        convs[0].add_(0.0)
    assert FN.resident_pack(convs[0], dtype) is None
    opt.refresh_packs()
    assert FN.resident_pack(convs[0], dtype) is not None


def test_student_distill_step_runs_and_learns():
    from fasterseg_amd.train_step import StudentDistillStep, synthetic_batch
    st = StudentDistillStep(2, 128, 256, teacher_engine_dtype=torch.bfloat16)
    imgs, tgt = synthetic_batch(2, 128, 256, 0, "cuda")
    losses = [float(st.step(imgs, tgt)) for _ in range(6)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
