"""FS_F16 at the boundary, without a device: the host-only plan functions answer for dtype 2 what they answer for bf16 (same element
size, so the same tiles, chunk counts and pack sizes), the Python dtype tables know torch.float16, training refuses it by name before
anything is launched, and a training entry point of the C ABI answers a status for it as it does for an unknown dtype."""
import ctypes
import os
import re

import pytest
import torch

from tests import test_halo_plan as HP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16, F16 = 0, 1, 2
LARGE_MAP_LAYERS = [(32, 64, 128, 256), (64, 64, 128, 256), (128, 128, 128, 256), (192, 128, 128, 256)]   # test_large_map_keeps_the_plain_form
FORCED = {"rule": 0, "tile32": 0x1000, "tile64": 0x2000, "tile128": 0x3000, "ksplit": 0x4000, "no_ksplit": 0x8000, "ksplit16": 0x14000}


def _lib():
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


def test_enum_value_and_python_tables():
    L, _ = _lib()
    from fasterseg_amd import kernels as K
    header = open(os.path.join(ROOT, "include", "fasterseg_hip.h")).read()
    assert int(re.search(r"\bFS_F16\s*=\s*(\d+)", header).group(1)) == L.FS_F16 == F16
    assert "65504" in header and "NaN stays NaN" in header            # the conversion rule is stated where the type is declared
    assert K.dtype_code(torch.float16) == 2 and K.vec_of(torch.float16) == 8 and K.elem_size(torch.float16) == 2
    assert [K.elem_size(t) for t in (torch.float32, torch.bfloat16)] == [4, 2]
    assert [K.elem_size(c) for c in (L.FS_F32, L.FS_BF16, L.FS_F16)] == [4, 2, 2]
    with pytest.raises(TypeError):
        K.dtype_code(torch.float64)
    with pytest.raises(TypeError):
        K.elem_size(3)


@pytest.mark.parametrize("flag", sorted(FORCED), ids=sorted(FORCED))
@pytest.mark.parametrize("layer", HP.SMALL_MAP_LAYERS + LARGE_MAP_LAYERS, ids=lambda l: "%d-%d@%dx%d" % l)
def test_halo_plan_is_the_bf16_plan(layer, flag):
    want = HP.plan(*layer, BF16, flags=FORCED[flag])
    got = HP.plan(*layer, F16, flags=FORCED[flag])
    assert got[0] == 0 and got == want, (got, want)


def test_halo_plan_stride2_stats_and_refusals_follow_bf16():
    for kw in (dict(stride=2), dict(has_stats=1), dict(flags=0x4000, has_stats=1), dict(flags=0x4000 | 0x8000), dict(flags=0x4000, stride=2)):
        assert HP.plan(64, 64, 32, 64, F16, **kw) == HP.plan(64, 64, 32, 64, BF16, **kw), kw
    assert HP.plan(64, 64, 32, 64, 3)[0] == 1 and HP.plan(64, 64, 32, 64, -1)[0] == 1        # an unknown dtype stays an error


def test_pw_plan_frag_elems_and_refresh_chunks_are_the_bf16_ones():
    L, h = _lib()
    from fasterseg_amd import kernels as K
    for shape, c3, cout, y_cs in (((1, 128, 128, 256), 128, 19, 32), ((1, 192, 64, 128), 128, 64, 64), ((2, 72, 9, 33), 64, 64, 64)):
        for rows in (0, 4, 8):
            a = K.conv3x3_pw_plan(K.conv_pw_desc(shape, shape[1], c3, cout, y_cs, torch.bfloat16, rows=rows))
            b = K.conv3x3_pw_plan(K.conv_pw_desc(shape, shape[1], c3, cout, y_cs, torch.float16, rows=rows))
            assert a == b and b[0] in (4, 8), (shape, rows, a, b)
    d = K.conv_pw_desc((1, 128, 16, 32), 128, 128, 19, 32, torch.float32)
    assert h.fs_conv3x3_pw_plan(ctypes.byref(d), None, None, None) == 2 and b"16-bit" in h.fs_last_error()      # fp32 stays refused
    for cout, cin in ((40, 24), (19, 128), (256, 256), (8, 8), (33, 72)):
        assert h.fs_packed_weight_frag_elems(cout, cin, F16) == h.fs_packed_weight_frag_elems(cout, cin, BF16) > 0
    src, dst = (ctypes.c_float * 4)(), (ctypes.c_char * 16)()

    def chunks(kind, dtype, cout, cin, k):
        e = L.RefreshEntry()
        e.kind, e.dtype, e.Cout, e.Cin, e.R, e.S = kind, dtype, cout, cin, k, k
        e.o_stride, e.i_stride = cin * k * k, k * k
        e.src, e.dst = ctypes.cast(src, ctypes.c_void_p), ctypes.cast(dst, ctypes.c_void_p)
        # fs_refresh_entry_chunks keeps its published fp32 / bf16 contract (tests/test_refresh_abi.py); FS_F16 packs are validated by
        # fs_refresh_entry_chunks_infer, which answers the original's counts for the other two types
        assert h.fs_refresh_entry_chunks_infer(ctypes.byref(e)) == h.fs_refresh_entry_chunks(ctypes.byref(e)) or dtype == F16
        assert dtype != F16 or (h.fs_refresh_entry_chunks(ctypes.byref(e)) == -1 and b"dtype" in h.fs_last_error())
        return h.fs_refresh_entry_chunks_infer(ctypes.byref(e))
    for cout, cin in ((40, 24), (256, 192), (19, 128)):
        assert chunks(L.FS_REFRESH_PACK, F16, cout, cin, 3) == chunks(L.FS_REFRESH_PACK, BF16, cout, cin, 3) > 0
        assert chunks(L.FS_REFRESH_PACK, F16, cout, cin, 1) == chunks(L.FS_REFRESH_PACK, BF16, cout, cin, 1) > 0
        assert chunks(L.FS_REFRESH_PACK_FRAG, F16, cout, cin, 3) == chunks(L.FS_REFRESH_PACK_FRAG, BF16, cout, cin, 3) > 0
    assert chunks(L.FS_REFRESH_PACK, 3, 40, 24, 3) == -1 and chunks(L.FS_REFRESH_PACK_FRAG, -1, 40, 24, 3) == -1


def test_zoom_cell_supported_follows_the_element_size():
    L, h = _lib()
    from fasterseg_amd import kernels as K
    for c, want16, want32 in ((64, True, True), (192, True, False), (256, True, False), (288, False, False)):
        for dt, want in ((torch.float16, want16), (torch.bfloat16, want16), (torch.float32, want32)):
            d = K.zoom_desc((1, 64, 32, 64), 64, c, c, True, True, c, dt)
            assert K.zoom_cell_supported(d) == want, (c, dt)


def test_training_refuses_float16_by_name_before_any_launch():
    from fasterseg_amd import functional as FN
    from fasterseg_amd.optim import FlatSGD
    from fasterseg_amd.train_step import StudentDistillStep
    before = FN.get_compute_dtype()
    with pytest.raises(TypeError, match="float16"):
        FN.set_compute_dtype(torch.float16)
    assert FN.get_compute_dtype() == before
    with pytest.raises(TypeError, match="float16"):
        FlatSGD(None, 0.1, pack_dtype=torch.float16)                  # refused before the (absent) gradient buffer is looked at
    with pytest.raises(ValueError, match="teacher_engine_dtype"):
        StudentDistillStep(1, 64, 128, teacher_engine_dtype=torch.float16, device="cpu")       # ... before any model is built


def test_uint8_stem_entry_points():
    """fs_conv_stem_u8_fwd keeps the dtype contract it was published with (tests/test_stem_u8_abi.py); fs_conv_stem_u8_infer_fwd is the
    same launch for the three storage types, with the same refusals otherwise (host-side validation: fake aligned addresses)."""
    _, h = _lib()
    tail = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)

    def call(fn, **kw):
        a = dict(img=0x10000, w=0x20000, y=0x30000, y_cs=32, dtype=F16)
        a.update(kw)
        return fn(None, 1, 18, 264, 32, a["img"], a["w"], None, None, a["y"], a["y_cs"], a["dtype"], 1, *tail)
    assert call(h.fs_conv_stem_u8_fwd) == 1 and h.fs_last_error() == b"fs_conv_stem_u8_fwd: bad dtype"
    for kw, word in ((dict(dtype=3), b"bad dtype"), (dict(dtype=-1), b"bad dtype"), (dict(img=None), b"null pointer"), (dict(y=0x30004), b"misaligned"),
                     (dict(y_cs=36), b"misaligned"), (dict(y_cs=24), b"misaligned")):
        assert call(h.fs_conv_stem_u8_infer_fwd, **kw) == 1, kw
        assert h.fs_last_error().startswith(b"fs_conv_stem_u8_infer_fwd") and word in h.fs_last_error(), (kw, h.fs_last_error())
    from fasterseg_amd.engine import InferenceEngine
    assert InferenceEngine._OPS["fs_conv_stem_u8_infer_fwd"] == "OP_STEM_U8"


def test_engine_refuses_a_logits_dtype_that_is_neither_fp32_nor_its_own():
    from fasterseg_amd.engine import InferenceEngine

    with pytest.raises(ValueError, match="logits_dtype"):
        InferenceEngine(torch.nn.Identity().eval(), (1, 3, 64, 128), dtype=torch.float16, logits_dtype=torch.bfloat16)


def test_training_entry_points_answer_a_status_for_dtype_2():
    """As test_invalid_arguments_return_status_not_abort: dummy host buffers, the refusal comes before anything touches the device."""
    L, h = _lib()
    buf = (ctypes.c_char * 256)()
    for dtype in (F16, 3):
        d = L.ConvDesc(1, 8, 8, 8, 8, 3, 3, 1, 1, 8, 8, 8, 8, dtype, 0)
        assert h.fs_conv2d_wgrad(None, ctypes.byref(d), buf, buf, buf) == 1 and b"dtype" in h.fs_last_error()
        assert h.fs_conv2d_wgrad_ws(None, ctypes.byref(d), buf, buf, buf, 72, 1, 8, None, 0) == 1 and b"dtype" in h.fs_last_error()
        r = L.ResizeDesc(1, 4, 4, 8, 8, 8, 8, 8, dtype, 0, 0)
        assert h.fs_bilinear_bwd(None, ctypes.byref(r), buf, None, buf) == 1 and b"dtype" in h.fs_last_error()
        # an inference convolution asked for BatchNorm statistics or a training gather
    d = L.ConvDesc(1, 8, 8, 8, 8, 3, 3, 1, 1, 8, 8, 8, 8, F16, 0)
    assert h.fs_conv2d_fwd(None, ctypes.byref(d), buf, buf, None, None, buf, buf) == 2 and b"inference only" in h.fs_last_error()
    assert h.fs_conv3x3_s1_fwd(None, ctypes.byref(d), buf, buf, None, None, buf, buf) == 2 and b"inference only" in h.fs_last_error()
    for flag in (L.FS_CONV_TRANSPOSED, 4):
        d.flags = flag
        assert h.fs_conv2d_fwd(None, ctypes.byref(d), buf, buf, None, None, buf, None) == 2 and b"inference only" in h.fs_last_error()


def test_census_prices_fp16_as_two_bytes():
    L, _ = _lib()
    from fasterseg_amd import census
    sizes = [census.conv_bytes(L.ConvDesc(1, 8, 8, 32, 32, 3, 3, 1, 1, 8, 8, 32, 32, dt, 0)) for dt in (F32, BF16, F16)]
    assert sizes[0] == 2 * sizes[1] and sizes[1] == sizes[2]


def test_argmax_seed_excludes_at_most_one_percent():
    """The arg-max test of tests/test_f16_kernels_gpu.py compares only pixels whose top-two margin exceeds the resample bound (and the
    planted exact ties): with its seed the fp64 reference alone decides >= 99 % of the pixels of every case."""
    from tests import test_f16_kernels_gpu as T
    for case in T.ARGMAX_CASES:
        _, _, use, ties = T._argmax_inputs(case, seed=T.ARGMAX_SEED)
        assert float(use.double().mean()) >= 0.99 and int(ties.sum()) > 0, (case, float(use.double().mean()), int(ties.sum()))
