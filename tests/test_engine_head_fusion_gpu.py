"""The inference engine with the head fusion forced (FS_ENGINE_FUSE_HEAD=2: fs_conv3x3_pw_fwd wherever head_fusion.match finds a chain)
against the same engine without it (FS_ENGINE_FUSE_HEAD=0: the separate launches), on the student (arch_1, eval build, seeded weights)
at 1x3x128x256, the smallest input the engine tests build.  The bound is the one tests/test_engine_gpu.py holds every kernel choice of
the bf16 engine to: max |difference| <= 5e-2 of max |logits| and arg-max agreement >= 97 %; both figures are printed.  The fused plan
must really hold the fused launches (tail and arm), issue the same result from the hipGraph, the direct launch list and the launch
program, and follow load_weights; output="classes" (the evaluator's engine) is held to the same arg-max agreement."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPE = (1, 3, 128, 256)
_cache = {}


def _net():
    if "net" not in _cache:
        from fasterseg_amd import archs
        from oracle.seeded import seeded_input, seeded_state
        net = archs.build_derived(1, training=False, lasts=[2, 1])
        net.load_state_dict(seeded_state(net.state_dict(), 12345))
        _cache["net"] = (net.cuda().eval(), seeded_input(SHAPE, 3).cuda())
    return _cache["net"]


def _engine(monkeypatch, mode, output="logits"):
    from fasterseg_amd import engine
    monkeypatch.setenv("FS_ENGINE_FUSE_HEAD", str(mode))
    monkeypatch.setenv("FS_ENGINE_AUTOTUNE", "0")
    monkeypatch.setenv("FS_ENGINE_FOLD_RESIZE", "1")        # "auto" times fold against chain per build: the two plans must differ in the heads only
    net, x = _net()
    with torch.no_grad():
        eng = engine.InferenceEngine(net, SHAPE, dtype=torch.bfloat16, fuse_cells="1", output=output)
        got = eng(x).clone()
        torch.cuda.synchronize()
    return eng, got


def test_forced_head_fusion_agrees_with_separate_launches(monkeypatch):
    net, x = _net()
    sep_eng, sep = _engine(monkeypatch, 0)
    fus_eng, fus = _engine(monkeypatch, 2)
    sep_fns, fus_fns = [c["fn"] for c in sep_eng.calls], [c["fn"] for c in fus_eng.calls]
    assert "fs_conv3x3_pw_fwd" not in sep_fns and sep_eng.head_log == []
    labels = [c["label"] for c in fus_eng.calls if c["fn"] == "fs_conv3x3_pw_fwd"]
    assert any(l.startswith("head 3x3+1x1") and "->19 " in l for l in labels), labels      # heads.conv_3x3 -> classifier
    assert any(l.startswith("head 3x3+1x1") and "->64 " in l for l in labels), labels      # an arm: 3x3 -> 1x1
    assert len(fus_fns) == len(sep_fns) - len(labels)
    assert fus_eng.total_flops == sep_eng.total_flops and fus_eng.total_bytes < sep_eng.total_bytes
    rel = float((fus - sep).abs().max()) / float(sep.abs().max())
    agree = float((fus.argmax(1) == sep.argmax(1)).float().mean())
    print("head fusion forced vs off: max |diff| / max |logits| %.3e, arg-max agreement %.5f" % (rel, agree))
    assert rel <= 5e-2 and agree >= 0.97, (rel, agree)
    # every way the plan can be issued gives the bits of the selected one
    with torch.no_grad():
        fus_eng.input.copy_(x)
        for issue in (fus_eng._launch_all, fus_eng._run_program, fus_eng._capture_once(1).replay):
            fus_eng.output.zero_()
            issue()
            torch.cuda.synchronize()
            assert torch.equal(fus_eng.output, fus), issue
        # the fused launches read the members' own packs, scales and shifts: a reload reaches them
        fus_eng.load_weights()
        assert torch.equal(fus_eng(x), fus)


def test_forced_head_fusion_classes_output(monkeypatch):
    _, sep = _engine(monkeypatch, 0, output="classes")
    eng, fus = _engine(monkeypatch, 2, output="classes")
    assert any(c["fn"] == "fs_conv3x3_pw_fwd" for c in eng.calls) and fus.dtype == torch.uint8
    agree = float((fus == sep).float().mean())
    print("head fusion forced vs off, class maps: agreement %.5f" % agree)
    assert agree >= 0.97, agree
