"""fs_bilinear_argmax_conf / fs_score_confidence at the boundary, without a device: every refusal comes back as a status with its text
(dummy host buffers: the refusal precedes anything that touches the device), the threshold rule of kernels.confidence_threshold, the
ValueErrors of the engine before any allocation, and the ABI number the two added symbols leave alone."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
INVALID, UNSUPPORTED = 1, 2


def _lib():
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


def test_symbols_are_added_and_the_abi_number_stays():
    L, h = _lib()
    header = open(os.path.join(ROOT, "include", "fasterseg_hip.h")).read()
    assert L.EXPECTED_ABI == 221 == h.fs_version() == int(re.search(r"#define FS_ABI_VERSION (\d+)", header).group(1))
    for name in ("fs_bilinear_argmax_conf", "fs_score_confidence"):
        assert re.search(r"^fs_status %s\(" % name, header, re.M) and name in L.SIGNATURES and hasattr(h, name)
    assert "FS_ABI_VERSION stays" in header.split("fs_status fs_bilinear_argmax_conf(")[0][-2500:]
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fs_bilinear_argmax_conf" in integration and "fs_score_confidence" in integration


def test_bilinear_argmax_conf_refusals():
    L, h = _lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16

    def call(desc=None, x=base, classes=base + 1024, conf=base + 2048, min_conf=0, ignore=255, **kw):
        f = dict(N=1, Hi=4, Wi=4, Ho=8, Wo=8, C=19, x_cs=20, y_cs=0, dtype=BF16, relu=0, out_nchw=0)
        f.update(kw)
        d = L.ResizeDesc(*[f[n] for n, _ in L.ResizeDesc._fields_])
        return h.fs_bilinear_argmax_conf(None, ctypes.byref(d) if desc is None else None, x, classes, conf, min_conf, ignore)
    for kw, status, word in (
            (dict(desc=False), INVALID, b"null"), (dict(x=None), INVALID, b"null"), (dict(classes=None, conf=None), INVALID, b"null"),
            (dict(x=base + 4), INVALID, b"misaligned"), (dict(classes=base + 1025), INVALID, b"misaligned"),
            (dict(conf=base + 2050), INVALID, b"misaligned"), (dict(x=base + 8, dtype=F32), INVALID, b"misaligned"),
            (dict(dtype=3), INVALID, b"bad dtype"), (dict(dtype=-1), INVALID, b"bad dtype"),
            (dict(Wo=10), UNSUPPORTED, b"multiple of 4"), (dict(x_cs=16), INVALID, b"channel stride"), (dict(x_cs=22), INVALID, b"channel stride"),
            (dict(C=0), INVALID, b"bad dimension"), (dict(C=257, x_cs=260), INVALID, b"bad dimension"), (dict(N=0), INVALID, b"bad dimension"),
            (dict(min_conf=-1), INVALID, b"min_conf"), (dict(min_conf=256), INVALID, b"min_conf"),
            (dict(ignore=-1), INVALID, b"ignore_label"), (dict(ignore=256), INVALID, b"ignore_label")):
        assert call(**kw) == status, kw
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_bilinear_argmax_conf") and word in msg, (kw, msg)


def test_score_confidence_refusals():
    _, h = _lib()
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16

    def call(score=base, pixels=4, cs=20, C=19, classes=base + 1024, conf=base + 2048, min_conf=0, ignore=255):
        return h.fs_score_confidence(None, score, pixels, cs, C, classes, conf, min_conf, ignore)
    for kw, status, word in (
            (dict(score=None), INVALID, b"null"), (dict(classes=None, conf=None), INVALID, b"null"), (dict(score=base + 4), INVALID, b"misaligned"),
            (dict(pixels=-1), INVALID, b"negative"), (dict(cs=18), INVALID, b"channel stride"), (dict(cs=0), INVALID, b"channel stride"),
            (dict(C=0), INVALID, b"C=0"), (dict(C=21), INVALID, b"C=21"), (dict(C=-3), INVALID, b"C=-3"),
            (dict(min_conf=-1), INVALID, b"min_conf"), (dict(min_conf=256), INVALID, b"min_conf"),
            (dict(ignore=-1), INVALID, b"ignore_label"), (dict(ignore=256), INVALID, b"ignore_label")):
        assert call(**kw) == status, kw
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_score_confidence") and word in msg, (kw, msg)
    assert call(pixels=0) == 0                          # an empty buffer: nothing to do, nothing launched


def test_confidence_threshold_rule():
    from fasterseg_amd import kernels as K
    assert [K.confidence_threshold(t) for t in (0, 0.0, 0.9, 1, 1.0, 0.5, 1 / 255, 230 / 255)] == [0, 0, 230, 255, 255, 128, 1, 230]
    for t in range(256):                                # q >= ceil(255 t)  <=>  q / 255 >= t, for every byte
        assert K.confidence_threshold(t / 255) == t
    for bad in (-1e-9, 1.0000001, 2, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min_confidence"):
            K.confidence_threshold(bad)


def test_engine_refuses_confidence_arguments_before_any_allocation():
    from fasterseg_amd.engine import InferenceEngine
    net = torch.nn.Identity().eval()
    for output in ("logits", "classes", "lowres"):
        for kw in (dict(min_confidence=0.5), dict(ignore_label=255), dict(min_confidence=0.0, ignore_label=0)):
            with pytest.raises(ValueError, match="classes\\+confidence"):
                InferenceEngine(net, (1, 3, 64, 128), output=output, device="cpu", **kw)
    for kw, word in ((dict(min_confidence=1.5), "min_confidence"), (dict(min_confidence=-0.1), "min_confidence"),
                     (dict(ignore_label=256), "ignore_label"), (dict(ignore_label=-1), "ignore_label"), (dict(ignore_label=2.5), "ignore_label")):
        with pytest.raises(ValueError, match=word):
            InferenceEngine(net, (1, 3, 64, 128), output="classes+confidence", device="cpu", **kw)
    assert "fs_bilinear_argmax_conf" not in InferenceEngine._OPS          # the executor's command list is closed: the plan runs from its graph


def test_pseudo_labeler_refuses_an_ignore_label_that_is_a_class():
    from fasterseg_amd.tester import PseudoLabeler
    with pytest.raises(ValueError, match="ignore_label"):
        PseudoLabeler(torch.nn.Identity().eval(), 19, (0, 0, 0), (1, 1, 1), "unused", ignore_label=7, write=False, device="cpu")
    with pytest.raises(ValueError, match="min_confidence"):
        PseudoLabeler(torch.nn.Identity().eval(), 19, (0, 0, 0), (1, 1, 1), "unused", min_confidence=1.2, write=False, device="cpu")
