"""CPU-side checks of the engine weight-reload boundary (fs_refresh_weights, refresh.hip): the entry descriptor's layout, the
host-only validator that stands between a caller's table and the kernel, and the error convention of the launch itself.  No
device is needed: nothing here launches."""
import ctypes

import pytest


def _lib():
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    return _lib, _lib.lib()


def _entry(L, kind, **kw):
    """A valid entry of `kind` (fake non-null addresses: the validator never dereferences them), then `kw` overrides."""
    e = L.RefreshEntry()
    e.kind, e.dtype, e.Cout, e.Cin, e.R, e.S, e.lo, e.eps = kind, L.FS_BF16, 40, 24, 3, 3, 0, 1e-5
    e.o_stride, e.i_stride = 32 * 9, 9
    e.src, e.beta, e.mean, e.var, e.dst, e.shift = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_entry_layout_matches_the_library():
    L, h = _lib()
    assert h.fs_struct_size(11) == ctypes.sizeof(L.RefreshEntry)
    assert h.fs_struct_size(10) == -1 and h.fs_struct_size(12) == -1          # 10 is unassigned
    assert h.fs_refresh_chunk_elems() > 0


BAD = [
    ("unknown kind", dict(kind=4), b"kind"),
    ("negative kind", dict(kind=-1), b"kind"),
    ("1x1 fragment pack", dict(kind=1, R=1, S=1), b"3x3"),
    ("3x1 fragment pack", dict(kind=1, R=3, S=1), b"3x3"),
    ("Cout 0", dict(kind=0, Cout=0), b"Cout"),
    ("Cin 0", dict(kind=0, Cin=0), b"Cin"),
    ("Cin 0 (frag)", dict(kind=1, Cin=0), b"Cin"),
    ("Cout -3 (fold)", dict(kind=2, Cout=-3), b"Cout"),
    ("null pack destination", dict(kind=0, dst=None), b"destination"),
    ("null frag destination", dict(kind=1, dst=None), b"destination"),
    ("null fold scale", dict(kind=2, dst=None), b"destination"),
    ("null fold shift", dict(kind=2, shift=None), b"destination"),
    ("null bias destination", dict(kind=3, shift=None), b"destination"),
    ("bad dtype", dict(kind=0, dtype=2), b"dtype"),
    ("bad dtype (frag)", dict(kind=1, dtype=-1), b"dtype"),
    ("null source", dict(kind=0, src=None), b"source"),
    ("null running_var", dict(kind=2, var=None), b"source"),
]


@pytest.mark.parametrize("what,override,word", BAD, ids=[b[0] for b in BAD])
def test_validator_rejects(what, override, word):
    L, h = _lib()
    override = dict(override)
    e = _entry(L, override.pop("kind"), **override)
    assert h.fs_refresh_entry_chunks(ctypes.byref(e)) == -1, what
    assert word in h.fs_last_error(), (what, h.fs_last_error())


def test_validator_counts_blocks_of_every_kind():
    L, h = _lib()
    chunk = h.fs_refresh_chunk_elems()
    ceil = lambda n: (n + chunk - 1) // chunk
    for dtype in (L.FS_F32, L.FS_BF16):
        assert h.fs_refresh_entry_chunks(ctypes.byref(_entry(L, L.FS_REFRESH_PACK, dtype=dtype))) == ceil(40 * 24 * 9)
        assert h.fs_refresh_entry_chunks(ctypes.byref(_entry(L, L.FS_REFRESH_PACK, dtype=dtype, R=1, S=1, Cout=19, Cin=128))) == ceil(19 * 128)
        frag = h.fs_packed_weight_frag_elems(40, 24, dtype)
        assert h.fs_refresh_entry_chunks(ctypes.byref(_entry(L, L.FS_REFRESH_PACK_FRAG, dtype=dtype))) == ceil(frag) > 1
    assert h.fs_refresh_entry_chunks(ctypes.byref(_entry(L, L.FS_REFRESH_FOLD, Cout=12, lo=12))) == 1
    assert h.fs_refresh_entry_chunks(ctypes.byref(_entry(L, L.FS_REFRESH_FOLD, Cout=chunk + 1))) == 2
    assert h.fs_refresh_entry_chunks(ctypes.byref(_entry(L, L.FS_REFRESH_BIAS, Cout=19, dst=None))) == 1
    assert h.fs_refresh_entry_chunks(None) == -1


def test_launch_returns_status_for_bad_tables():
    """Validated before any launch: a null table or a negative size is a status and a message, never an abort."""
    L, h = _lib()
    buf = (ctypes.c_char * 256)()
    assert h.fs_refresh_weights(None, None, 1, buf, 1) == 1 and b"null table" in h.fs_last_error()
    assert h.fs_refresh_weights(None, buf, 1, None, 1) == 1 and b"null table" in h.fs_last_error()
    assert h.fs_refresh_weights(None, buf, 1, buf, -1) == 1 and b"bad table size" in h.fs_last_error()
    assert h.fs_refresh_weights(None, buf, 0, buf, 1) == 1 and b"bad table size" in h.fs_last_error()
    with pytest.raises(L.FasterSegHipError, match="fs_refresh_weights failed"):
        L.call("fs_refresh_weights", None, None, 0, None, 0)
