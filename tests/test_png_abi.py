"""fs_png_deflate at the boundary, without a device: the three symbols and the ABI number they leave alone, every refusal as a status
with its text (dummy host buffers: the refusal precedes anything that touches the device), the bound's values, the wrapper's default
band height, PredictionWriter's device_png argument and png_bytes."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tests import _png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 2
NEW = ("fs_png_deflate_bound", "fs_png_deflate_workspace_bytes", "fs_png_deflate")


def _lib():
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


def test_symbols_are_added_and_the_abi_number_stays():
    L, h = _lib()
    header = open(os.path.join(ROOT, "include", "fasterseg_hip.h")).read()
    assert L.EXPECTED_ABI == 221 == h.fs_version() == int(re.search(r"#define FS_ABI_VERSION (\d+)", header).group(1))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"^(fs_status|size_t) %s\(" % name, header, re.M) and name in L.ALL_SYMBOLS and hasattr(h, name)
        assert name in integration
    assert "FS_ABI_VERSION stays 221" in header.split("size_t fs_png_deflate_bound(")[0][-4000:]
    assert len(L.SIGNATURES["fs_png_deflate"]) == 11
    assert L._SPECIAL["fs_png_deflate_bound"][1] is ctypes.c_size_t and L._SPECIAL["fs_png_deflate_workspace_bytes"][1] is ctypes.c_size_t
    assert int(re.search(r"#define FS_PNG_BAND_MAX_BYTES (\d+)", header).group(1)) == L.FS_PNG_BAND_MAX_BYTES == R.BAND_CAP
    from fasterseg_amd import build
    assert "png_deflate.hip" in build.SOURCES


def test_bound_and_workspace_values():
    _, h = _lib()
    for rows, row_bytes, rpb in ((1, 1, 1), (3, 5, 2), (7, 259, 4), (16, 1031, 5), (5, 600, 5), (4, 111, 3), (1024, 2048, 4), (1024, 2048, 7),
                                 (8, 2047, 8), (100000, 3, 1)):
        assert h.fs_png_deflate_bound(rows, row_bytes, rpb) == R.bound(rows, row_bytes, rpb), (rows, row_bytes, rpb)
        ws = h.fs_png_deflate_workspace_bytes(rows, row_bytes, rpb)
        bands = -(-rows // rpb)
        # every band needs room for its worst case (a multiple of 16, for the 16-byte stores) and a record of its length and checksums
        assert ws % 16 == 0 and ws >= bands * ((13 + 9 * min(rows, rpb) * (row_bytes + 1) + 7) // 8 + 4 + 24)
    assert h.fs_png_deflate_bound(0, 7, 3) == 2 + 5 + 4 and h.fs_png_deflate_workspace_bytes(0, 7, 3) == 0
    for bad in ((-1, 5, 1), (3, 0, 1), (3, -2, 1), (3, 5, 0), (3, 5, -1)):
        assert h.fs_png_deflate_bound(*bad) == 0 and h.fs_png_deflate_workspace_bytes(*bad) == 0


def test_png_deflate_refusals():
    _, h = _lib()
    keep = (ctypes.c_char * 8192)()
    base = ctypes.addressof(keep)
    base += (-base) % 16
    big = 1 << 40

    def call(src=base + 3, rows=3, row_bytes=5, pitch=5, rpb=2, out=base + 1024, cap=big, out_bytes=base + 2048, ws=base + 4096, ws_bytes=big):
        return h.fs_png_deflate(None, src, rows, row_bytes, pitch, rpb, out, cap, out_bytes, ws, ws_bytes)
    bound, need = h.fs_png_deflate_bound(3, 5, 2), h.fs_png_deflate_workspace_bytes(3, 5, 2)
    for kw, status, word in (
            (dict(src=None), INVALID, b"null"), (dict(out=None), INVALID, b"null"), (dict(out_bytes=None), INVALID, b"null"),
            (dict(ws=None), INVALID, b"null"),
            (dict(out_bytes=base + 2052), INVALID, b"misaligned"), (dict(ws=base + 4104), INVALID, b"misaligned"),
            (dict(rows=-1), INVALID, b"bad dimension"), (dict(row_bytes=0), INVALID, b"bad dimension"), (dict(row_bytes=-5), INVALID, b"bad dimension"),
            (dict(rpb=0), INVALID, b"bad dimension"), (dict(rpb=-2), INVALID, b"bad dimension"),
            (dict(pitch=4), INVALID, b"pitch"), (dict(pitch=-5), INVALID, b"pitch"),
            (dict(cap=bound - 1), INVALID, b"out_capacity"), (dict(cap=0), INVALID, b"out_capacity"),
            (dict(ws_bytes=need - 1), INVALID, b"ws_bytes"), (dict(ws_bytes=0), INVALID, b"ws_bytes"),
            (dict(rows=8, row_bytes=2048, pitch=2048, rpb=8), UNSUPPORTED, b"LDS cap"),                 # 16392 filtered bytes a band
            (dict(rows=1, row_bytes=16384, pitch=16384, rpb=1), UNSUPPORTED, b"LDS cap"),
            (dict(rows=1 << 20, row_bytes=2047, pitch=2047, rpb=8), UNSUPPORTED, b"2^31"),
            (dict(rows=(1 << 31) - 1, row_bytes=1, pitch=1, rpb=1), UNSUPPORTED, b"2^31")):
        assert call(**kw) == status, kw
        msg = h.fs_last_error()
        assert msg.startswith(b"fs_png_deflate:") and word in msg, (kw, msg)
    # the cap itself is accepted: a band of exactly 16384 filtered bytes gets as far as the capacity check
    assert call(rows=8, row_bytes=2047, pitch=2047, rpb=8, cap=0) == INVALID and b"out_capacity" in h.fs_last_error()
    assert call(rows=3, row_bytes=2047, pitch=2047, rpb=100, cap=0) == INVALID and b"out_capacity" in h.fs_last_error()   # a band is never taller than the map
    assert call(rows=0) == 0 and call(rows=0, src=None, out=None, out_bytes=None, ws=None, cap=0, ws_bytes=0) == 0      # nothing to do, nothing launched


def test_default_rows_per_band():
    from fasterseg_amd import kernels as K
    assert K.png_rows_per_band(1024, 2048) == 4                       # 256 bands of 8196 filtered bytes
    assert K.png_rows_per_band(1024, 3 * 2048) == 2                   # the LDS cap: 2 * 6145 <= 16384 < 3 * 6145
    assert K.png_rows_per_band(1, 1) == 1 and K.png_rows_per_band(255, 8) == 1 and K.png_rows_per_band(256, 8) == 1
    assert K.png_rows_per_band(1279, 8) == 5 and -(-1279 // 5) == 256 and K.png_rows_per_band(1275, 8) == 4
    assert K.png_rows_per_band(100000, 8) == 392 and -(-100000 // 392) >= 256 > -(-100000 // 393)
    assert K.png_rows_per_band(100000, 100) == 162                    # capped: 162 * 101 <= 16384 < 163 * 101
    assert K.png_rows_per_band(4, 16383) == 1
    with pytest.raises(ValueError, match="above"):
        K.png_rows_per_band(4, 16384)


def test_writer_needs_a_device_for_device_png():
    from fasterseg_amd.tester import PredictionWriter
    with pytest.raises(ValueError, match="device_png"):
        PredictionWriter(device=None, device_png=True)
    w = PredictionWriter(slots=1, workers=1, device=None)              # the default is the host path, as before
    assert w.device_png is False
    w.close()


def test_png_bytes_wraps_a_stream_into_a_file():
    from PIL import Image
    from fasterseg_amd.png import png_bytes
    rng = np.random.default_rng(5)
    for a, rpb in ((rng.integers(0, 19, (9, 33), dtype=np.uint8), 4), (rng.integers(0, 256, (4, 37, 3), dtype=np.uint8), 3)):
        data = png_bytes(a.shape[0], a.shape[1], 1 if a.ndim == 2 else 3, R.zstream(a, rpb))
        assert data == R.png_file(a, rpb)
        with Image.open(io.BytesIO(data)) as im:
            assert im.mode == ("L" if a.ndim == 2 else "RGB") and np.array_equal(np.asarray(im), a)
        assert np.array_equal(R.read_png(png_bytes(a.shape[0], a.shape[1], 1 if a.ndim == 2 else 3, np.frombuffer(R.zstream(a, rpb), np.uint8))), a)
    for bad in ((9, 33, 2), (9, 33, 4), (0, 33, 1), (9, 0, 1)):
        with pytest.raises(ValueError, match="png_bytes"):
            png_bytes(*bad, b"")
