"""The head-fusion matcher of the inference engine (fasterseg_amd/head_fusion.py, engine.InferenceEngine._mark_head_fusions) on hand-built
op lists: no GPU needed, the pass only looks at op kinds, shapes and producer / consumer edges.  It must find `3x3 -> 1x1`, leave a
`1x1(BN, ReLU) -> 3x3` alone (that launch form was measured no faster and is not built), refuse an intermediate with a second consumer (the train-mode heads) or one that is the engine's
output, and with FS_ENGINE_FUSE_HEAD=0 leave the op list exactly as the engine without the fusion sees it."""
import os

import pytest
import torch

from fasterseg_amd import engine, head_fusion
from fasterseg_amd.engine import _Tracer
from fasterseg_amd.functional import SymTensor


class _W:          # stands in for a filter tensor: the tracer only reads .shape
    def __init__(self, *shape):
        self.shape = shape


BN = ("gamma", "beta", "mean", "var", 1e-5)     # the matcher only asks whether a BatchNorm is there


def _mark(ops, out_sym, mode=None, dtype=torch.bfloat16):
    e = engine.InferenceEngine.__new__(engine.InferenceEngine)
    e.ops, e.out_sym, e.dtype = ops, out_sym, dtype
    e.fuse_head = int(os.environ.get("FS_ENGINE_FUSE_HEAD", "1")) if mode is None else mode
    e._mark_head_fusions()
    return e


def _tail(second_reader=False, lowres_output=False, arm_reader_is_cat=False):
    """cat -> ffm 1x1 (BN, ReLU) -> head 3x3 (BN, ReLU) -> classifier 1x1 (+bias) -> logits up-sample, beside an arm 3x3 -> 1x1."""
    t = _Tracer(torch.bfloat16)
    x = SymTensor((1, 192, 64, 128), torch.bfloat16)
    r = t.conv(x, _W(128, 192, 3, 3), BN, None, 1, 1, True, False, 128, 192)              # op 0: refine 3x3 192 -> 128
    a = t.conv(r, _W(64, 128, 1, 1), BN, None, 1, 0, True, False, 64, 128)                # op 1: arm 1x1, the 3x3's only reader
    up = t.resize(a, (128, 256), False, 0)                                                 # op 2
    y = SymTensor((1, 64, 128, 256), torch.bfloat16)
    cat = t.cat([up, y])                                                                   # op 3
    f = t.conv(cat, _W(128, 128, 1, 1), BN, None, 1, 0, True, False, 128, 128)            # op 4: ffm.conv_1x1
    h = t.conv(f, _W(128, 128, 3, 3), BN, None, 1, 1, True, False, 128, 128)              # op 5: heads.conv_3x3
    c = t.conv(h, _W(19, 128, 1, 1), None, "bias", 1, 0, False, False, 19, 128)           # op 6: heads.conv_1x1
    if second_reader:                                                                      # train mode: a second head reads the 3x3's map
        t.conv(h, _W(19, 128, 1, 1), None, "bias", 1, 0, False, False, 19, 128)           # op 7
    out = t.resize(c, (1024, 2048), False, 1)
    if arm_reader_is_cat:                                                                  # the arm's 3x3 map also goes into a concat
        t.cat([r, SymTensor((1, 64, 64, 128), torch.bfloat16)])
    return t.ops, (h if lowres_output else out)


def test_matcher_fuses_3x3_then_1x1_and_leaves_the_1x1_in_front():
    ops, out = _tail()
    e = _mark(ops, out)
    assert e.head_matches == [dict(conv=0, post=1), dict(conv=5, post=6)]       # the arm, and heads.conv_3x3 -> heads.conv_1x1
    assert ops[1]["head"] is e.head_matches[0] and ops[6]["head"] is e.head_matches[1]
    assert "head" not in ops[4] and "head" not in ops[5]                         # ffm.conv_1x1 stays a launch of its own
    # 1x1(BN, ReLU) -> 3x3 alone (the 3x3's reader is the up-sample): the form that computes the 1x1 on the 3x3's halo is not built
    t = _Tracer(torch.bfloat16)
    x = SymTensor((1, 96, 32, 64), torch.bfloat16)
    p = t.conv(x, _W(64, 96, 1, 1), BN, None, 1, 0, True, False, 64, 96)
    c = t.conv(p, _W(64, 64, 3, 3), BN, None, 1, 1, True, False, 64, 64)
    out = t.resize(c, (256, 512), False, 1)
    assert head_fusion.match(t.ops, out) == []


def test_matcher_refuses_second_consumers_outputs_and_unsupported_members():
    ops, out = _tail(second_reader=True)                   # the train-mode heads: two readers of the 3x3's map
    assert head_fusion.match(ops, out) == [dict(conv=0, post=1)]
    ops, out = _tail(lowres_output=True)                   # the 3x3's map is the engine's output
    assert head_fusion.match(ops, out) == [dict(conv=0, post=1)]
    ops, out = _tail(arm_reader_is_cat=True)               # the arm's 3x3 also feeds a concat
    assert head_fusion.match(ops, out) == [dict(conv=5, post=6)]
    # the 3x3 must be stride 1 / pad 1 with at most 128 output channels (a multiple of 8), read its input as it is, and be alive
    for kw in (dict(stride=2), dict(cout=160), dict(cout=100), dict(fold=object()), dict(vres=(64, 128, False)), dict(dead=True)):
        ops, out = _tail()
        ops[5].update(kw)
        assert [m for m in head_fusion.match(ops, out) if m["conv"] == 5] == [], kw
    # the 1x1 behind must be a plain stride-1 1x1 on the 3x3's own map
    for kw in (dict(stride=2), dict(k=3, pad=1), dict(vres=(128, 256, False)), dict(cout=160)):
        ops, out = _tail()
        ops[6].update(kw)
        assert [m for m in head_fusion.match(ops, out) if m["conv"] == 5] == [], kw


def test_fuse_head_0_and_fp32_restore_the_parents_list(monkeypatch):
    ops, out = _tail()
    before = [dict(op) for op in ops]
    e = _mark(ops, out, mode=0)
    assert e.head_matches == [] and ops == before and not any("head" in op for op in ops)
    monkeypatch.setenv("FS_ENGINE_FUSE_HEAD", "0")
    ops, out = _tail()
    e = _mark(ops, out)
    assert e.head_matches == [] and not any("head" in op for op in ops)
    ops, out = _tail()
    e = _mark(ops, out, mode=1, dtype=torch.float32)       # the kernel is bf16 only: the fp32 engine keeps the separate launches
    assert e.head_matches == [] and not any("head" in op for op in ops)
    monkeypatch.setenv("FS_ENGINE_FUSE_HEAD", "2")
    ops, out = _tail()
    assert len(_mark(ops, out).head_matches) == 2
