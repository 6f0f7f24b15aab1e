"""fs_bilinear_argmax_conf_pc / fs_score_confidence_pc / fs_confidence_hist at the boundary, without a device: the three symbols and the
ABI number they leave alone, every refusal as a status with its text (dummy host buffers: the refusal precedes anything that touches the
device) and the rules of kernels.class_threshold_table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
INVALID, UNSUPPORTED = 1, 2
NEW = ("fs_bilinear_argmax_conf_pc", "fs_score_confidence_pc", "fs_confidence_hist")


def _lib():
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


def _buffer():
    buf = (ctypes.c_char * 8192)()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_symbols_are_added_and_the_abi_number_stays():
    L, h = _lib()
    header = open(os.path.join(ROOT, "include", "fasterseg_hip.h")).read()
    assert L.EXPECTED_ABI == 221 == h.fs_version() == int(re.search(r"#define FS_ABI_VERSION (\d+)", header).group(1))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"^fs_status %s\(" % name, header, re.M) and name in L.SIGNATURES and hasattr(h, name)
        assert name in integration
    assert "FS_ABI_VERSION stays 221" in header.split("fs_status fs_bilinear_argmax_conf_pc(")[0][-1500:]
    assert len(L.SIGNATURES["fs_bilinear_argmax_conf_pc"]) == 7 and len(L.SIGNATURES["fs_score_confidence_pc"]) == 9
    assert len(L.SIGNATURES["fs_confidence_hist"]) == 8
    from fasterseg_amd import build
    assert "confidence.hip" in build.SOURCES


def test_bilinear_argmax_conf_pc_refusals():
    L, h = _lib()
    keep, base = _buffer()

    def call(desc=None, x=base, classes=base + 1024, conf=base + 2048, table=base + 4096, ignore=255, **kw):
        f = dict(N=1, Hi=4, Wi=4, Ho=8, Wo=8, C=19, x_cs=20, y_cs=0, dtype=BF16, relu=0, out_nchw=0)
        f.update(kw)
        d = L.ResizeDesc(*[f[n] for n, _ in L.ResizeDesc._fields_])
        return h.fs_bilinear_argmax_conf_pc(None, ctypes.byref(d) if desc is None else None, x, classes, conf, table, ignore)
    for kw, status, word in (
            (dict(desc=False), INVALID, b"null"), (dict(x=None), INVALID, b"null"), (dict(classes=None, conf=None), INVALID, b"null"),
            (dict(table=None), INVALID, b"min_conf_by_class"),
            (dict(x=base + 4), INVALID, b"misaligned"), (dict(classes=base + 1025), INVALID, b"misaligned"),
            (dict(conf=base + 2050), INVALID, b"misaligned"), (dict(x=base + 8, dtype=F32), INVALID, b"misaligned"),
            (dict(dtype=3), INVALID, b"bad dtype"), (dict(dtype=-1), INVALID, b"bad dtype"),
            (dict(Wo=10), UNSUPPORTED, b"multiple of 4"), (dict(x_cs=16), INVALID, b"channel stride"), (dict(x_cs=22), INVALID, b"channel stride"),
            (dict(C=0), INVALID, b"bad dimension"), (dict(C=257, x_cs=260), INVALID, b"bad dimension"), (dict(N=0), INVALID, b"bad dimension"),
            (dict(ignore=-1), INVALID, b"ignore_label"), (dict(ignore=256), INVALID, b"ignore_label")):
        assert call(**kw) == status, kw
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_bilinear_argmax_conf_pc:") and word in msg, (kw, msg)
    # the scalar form's messages still carry its own name (one body serves both)
    d = L.ResizeDesc(1, 4, 4, 8, 10, 19, 20, 0, BF16, 0, 0)
    assert h.fs_bilinear_argmax_conf(None, ctypes.byref(d), base, base + 1024, base + 2048, 0, 255) == UNSUPPORTED
    assert h.fs_last_error().startswith(b"fs_bilinear_argmax_conf:")


def test_score_confidence_pc_refusals():
    _, h = _lib()
    keep, base = _buffer()

    def call(score=base, pixels=4, cs=20, C=19, classes=base + 1024, conf=base + 2048, table=base + 4096, ignore=255):
        return h.fs_score_confidence_pc(None, score, pixels, cs, C, classes, conf, table, ignore)
    for kw, status, word in (
            (dict(score=None), INVALID, b"null"), (dict(classes=None, conf=None), INVALID, b"null"), (dict(score=base + 4), INVALID, b"misaligned"),
            (dict(table=None), INVALID, b"min_conf_by_class"),
            (dict(pixels=-1), INVALID, b"negative"), (dict(cs=18), INVALID, b"channel stride"), (dict(cs=0), INVALID, b"channel stride"),
            (dict(C=0), INVALID, b"C=0"), (dict(C=21), INVALID, b"C=21"), (dict(C=-3), INVALID, b"C=-3"),
            (dict(C=260, cs=260), UNSUPPORTED, b"C=260"),
            (dict(ignore=-1), INVALID, b"ignore_label"), (dict(ignore=256), INVALID, b"ignore_label")):
        assert call(**kw) == status, kw
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_score_confidence_pc:") and word in msg, (kw, msg)
    assert call(pixels=0) == 0                          # an empty buffer: nothing to do, nothing launched


def test_confidence_hist_refusals():
    _, h = _lib()
    keep, base = _buffer()

    def call(classes=base + 1, conf=base + 1027, gt=None, gt_bytes=0, n=16, C=19, hist=base + 4096):
        return h.fs_confidence_hist(None, classes, conf, gt, gt_bytes, n, C, hist)
    for kw, status, word in (
            (dict(n=-1), INVALID, b"negative"), (dict(hist=None), INVALID, b"null hist"), (dict(hist=base + 4100), INVALID, b"misaligned"),
            (dict(C=0), INVALID, b"C=0"), (dict(C=-1), INVALID, b"C=-1"), (dict(C=33), UNSUPPORTED, b"C=33"), (dict(C=256), UNSUPPORTED, b"C=256"),
            (dict(gt=base + 2048, gt_bytes=2), INVALID, b"uint8, int32 or int64"), (dict(gt=base + 2048, gt_bytes=0), INVALID, b"uint8, int32 or int64"),
            (dict(gt=base + 2050, gt_bytes=4), INVALID, b"misaligned"), (dict(gt=base + 2052, gt_bytes=8), INVALID, b"misaligned"),
            (dict(classes=None), INVALID, b"null classes"), (dict(conf=None), INVALID, b"null classes")):
        assert call(**kw) == status, kw
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_confidence_hist:") and word in msg, (kw, msg)
    assert call(n=0) == 0 and call(n=0, classes=None, conf=None) == 0          # nothing to count, nothing launched
    assert call(n=0, gt=base + 2048, gt_bytes=8, C=32) == 0
    assert call(n=0, gt_bytes=2) == 0                    # gt_bytes is read only beside labels


def test_class_threshold_table_rules():
    from fasterseg_amd import kernels as K
    t = K.class_threshold_table(0.9, 19, "cpu")
    assert t.dtype == torch.uint8 and tuple(t.shape) == (256,) and t.is_contiguous()
    assert (t[:19] == 230).all() and (t[19:] == 0).all()
    values = [i / 18 for i in range(19)]
    t = K.class_threshold_table(values, 19, "cpu")
    assert t[:19].tolist() == [K.confidence_threshold(v) for v in values] and (t[19:] == 0).all()
    assert K.class_threshold_table(np.asarray(values, dtype=np.float32), 19, "cpu")[:19].tolist() == [K.confidence_threshold(np.float32(v)) for v in values]
    raw = np.arange(237, 256, dtype=np.uint8)           # a uint8 array: the bytes themselves
    assert K.class_threshold_table(raw, 19, "cpu")[:19].tolist() == raw.tolist()
    assert K.class_threshold_table(torch.from_numpy(raw), 19, "cpu")[:19].tolist() == raw.tolist()
    assert (K.class_threshold_table(np.uint8(7), 3, "cpu")[:4].tolist()) == [7, 7, 7, 0]
    assert K.class_threshold_table([0, 1], 2, "cpu")[:3].tolist() == [0, 255, 0]          # integers that are not uint8: floats in [0, 1]
    assert K.class_threshold_table(1.0, 256, "cpu").tolist() == [255] * 256
    assert (K.class_threshold_bytes(0.5, 19) == K.class_threshold_table(0.5, 19, "cpu").numpy()).all()
    for bad in ([0.5] * 18, [0.5] * 20, [], np.zeros(20, dtype=np.uint8), np.zeros((19, 1)), [[0.5] * 19]):
        with pytest.raises(ValueError, match="class_thresholds"):
            K.class_threshold_table(bad, 19, "cpu")
    for bad in (1.5, -0.1, float("nan"), [0.5] * 18 + [2.0], [0.5] * 18 + [-1e-9], np.full(19, 230), "0.5", None, [None] * 19, True):
        with pytest.raises(ValueError, match="class_thresholds"):
            K.class_threshold_table(bad, 19, "cpu")
    for bad in (0, 257):
        with pytest.raises(ValueError, match="class_num"):
            K.class_threshold_table(0.5, bad, "cpu")
    # the launches' wrappers: a table and a threshold exclude each other (refused before anything is read)
    x = torch.zeros((1, 4, 4, 20)).permute(0, 3, 1, 2)[:, :19]
    with pytest.raises(ValueError, match="exclude"):
        K.bilinear_argmax_conf(x, (8, 8), min_confidence=0.5, class_thresholds=t)
    with pytest.raises(ValueError, match="exclude"):
        K.score_confidence(torch.zeros((4, 20)), 19, min_confidence=0.5, class_thresholds=t)
    with pytest.raises(ValueError, match="uint8\\[256\\]"):
        K.score_confidence(torch.zeros((4, 20)), 19, class_thresholds=t[:19])
