"""CPU-side checks of the uint8 stem's boundary (fs_conv_stem_u8_fwd, ABI 221): the symbol, the ABI number on both sides of the
binding, the op code of the launch program and the error convention.  Every refusal is decided on the host before a launch, so no
device is needed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _lib():
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


def _header():
    with open(os.path.join(ROOT, "include", "fasterseg_hip.h")) as f:
        return f.read()


def test_symbol_and_abi_number():
    L, h = _lib()
    assert hasattr(h, "fs_conv_stem_u8_fwd")
    assert h.fs_version() == L.EXPECTED_ABI == 221
    assert int(re.search(r"#define FS_ABI_VERSION (\d+)", _header()).group(1)) == 221
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "fs_version() == 221" in f.read()


def test_op_code_matches_the_header_enum():
    from fasterseg_amd import program as P
    from fasterseg_amd.engine import InferenceEngine
    body = re.search(r"enum \{(\s*FS_OP_MEMSET = 0,.*?)\};", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)                            # the enumerators in order, comments dropped
    names = [e.split("=")[0].strip() for e in body.split(",") if e.strip()]
    assert names[-1] == "FS_OP_COUNT" and names[-2] == "FS_OP_STEM_U8"          # appended directly before FS_OP_COUNT
    assert P.OP_STEM_U8 == names.index("FS_OP_STEM_U8")
    assert P.OP_STEM == names.index("FS_OP_STEM") and P.OP_CONV3X3_PW == names.index("FS_OP_CONV3X3_PW")
    assert InferenceEngine._OPS["fs_conv_stem_u8_fwd"] == "OP_STEM_U8"


def _call(h, **kw):
    """fs_conv_stem_u8_fwd with valid host-side arguments (fake aligned addresses: validation never dereferences them), then overrides."""
    a = dict(N=1, H=18, W=264, Cout=32, img=0x10000, w=0x20000, scale=None, shift=None, y=0x30000, y_cs=32, dtype=1, relu=1,
             mean=MEAN, std=STD)
    a.update(kw)
    return h.fs_conv_stem_u8_fwd(None, a["N"], a["H"], a["W"], a["Cout"], a["img"], a["w"], a["scale"], a["shift"], a["y"], a["y_cs"],
                                 a["dtype"], a["relu"], *(tuple(a["mean"]) + tuple(a["std"])))


def test_refusals_are_statuses_with_messages():
    L, h = _lib()
    assert L.FS_BF16 == 1
    FS_ERR_INVALID = 1
    bad = [
        (dict(img=None), b"null pointer"),
        (dict(w=None), b"null pointer"),
        (dict(y=None), b"null pointer"),
        (dict(dtype=2), b"bad dtype"),
        (dict(dtype=-1), b"bad dtype"),
        (dict(y=0x30004), b"misaligned"),                 # output slice not 16-byte aligned
        (dict(y_cs=36), b"misaligned"),                   # channel stride not a whole bf16 vector
        (dict(y_cs=24), b"misaligned"),                   # channel stride below Cout
        (dict(std=(0.229, 0.0, 0.225)), b"std"),
        (dict(std=(0.0, 0.224, 0.225)), b"std"),
        (dict(std=(0.229, 0.224, -0.0)), b"std"),
        (dict(H=1), b"bad shape"),
        (dict(N=0), b"bad shape"),
    ]
    for override, word in bad:
        assert _call(h, **override) == FS_ERR_INVALID, override
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_conv_stem_u8_fwd") and word in msg, (override, msg)
    try:
        L.call("fs_conv_stem_u8_fwd", None, 1, 18, 264, 32, None, None, None, None, None, 32, 1, 1, *(MEAN + STD))
    except L.FasterSegHipError as e:
        assert "fs_conv_stem_u8_fwd failed" in str(e)
    else:
        raise AssertionError("a null image must raise through _lib.call")


def test_fp32_entry_point_keeps_its_messages():
    L, h = _lib()
    assert h.fs_conv_stem_fwd(None, 1, 18, 264, 32, None, 0x20000, None, None, 0x30000, 32, 1, 1) == 1
    assert h.fs_last_error() == b"fs_conv_stem_fwd: null pointer"
    assert h.fs_conv_stem_fwd(None, 1, 18, 264, 32, 0x10000, 0x20000, None, None, 0x30004, 32, 1, 1) == 1
    assert h.fs_last_error() == b"fs_conv_stem_fwd: output slice misaligned (y_cs=32)"


def test_division_by_255_without_a_division():
    """csrc/stem.hip computes (float)u / 255.f as q = RN(u * y), q' = RN(q + RN(u - 255 q) * y) with y = RN(1 / 255): in exact rational
    arithmetic, q' is the correctly rounded quotient (numpy's float32 division) for every byte, and the plain product q is not."""
    from fractions import Fraction as F
    import numpy as np

    def rn32(x):
        """round-to-nearest-even of a rational to an fp32 value (normal range)"""
        if x == 0:
            return F(0)
        sign, x, e = (1 if x > 0 else -1), abs(x), 0
        while x >= 2:
            x, e = x / 2, e + 1
        while x < 1:
            x, e = x * 2, e - 1
        m = x * 2 ** 23
        fl = m.numerator // m.denominator
        rem = m - fl
        if rem > F(1, 2) or (rem == F(1, 2) and fl % 2 == 1):
            fl += 1
        return sign * F(fl) * F(2) ** (e - 23)
    y = rn32(F(1, 255))
    assert y == F(float(np.float32(1) / np.float32(255)))
    plain_wrong = 0
    for u in range(256):
        want = F(float(np.float32(u) / np.float32(255)))
        assert want == rn32(F(u, 255))
        q = rn32(u * y)
        plain_wrong += q != want
        r = rn32(F(u) - 255 * q)                 # fma(-255, q, u)
        assert rn32(q + r * y) == want, u        # fma(r, y, q)
    assert plain_wrong > 0                       # the correction is needed: the reciprocal multiply alone is a ulp off for some bytes
