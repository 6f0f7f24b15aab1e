"""tests/_png_ref.py checked against zlib and PIL, without a device: the reference encoder's streams inflate to the filtered bytes, its
files open in PIL and in the reader, every stream stays within fs_png_deflate_bound's formula, and the reader refuses damaged files."""
import io
import struct
import zlib

import numpy as np
import pytest

from tests import _png_ref as R

CASES = R.cases()


def test_the_cases_cover_what_they_claim():
    names = [n for n, _, _ in CASES]
    for H, W, rpb in ((1, 1, 1), (1, 3, 1), (3, 5, 2), (7, 259, 4), (16, 1031, 5), (9, 2048, 3), (5, 600, 5)):
        for kind in ("constant", "one run", "sweep", "literals", "noise", "19 classes"):
            assert "%s %dx%d/%d" % (kind, H, W, rpb) in names
    assert any(a.ndim == 3 and a.shape == (4, 37, 3) for _, a, _ in CASES)
    by = {n: (a, r) for n, a, r in CASES}
    f = R.filtered(by["one run 7x259/4"][0])
    assert (f == 2).all() and f[:4].size > 2 * 258                       # one run through the filter bytes, cut by the band boundary
    runs = set()                                                         # the sweep's bands: run lengths with every remainder 0..3
    for r in range(0, 16, 5):
        f = R.filtered(by["sweep 16x1031/5"][0])[r:r + 5].reshape(-1)
        cuts = np.flatnonzero(np.diff(f.astype(np.int16)) != 0)
        runs |= set(np.diff(np.concatenate([[-1], cuts, [f.size - 1]])).tolist())
    assert {1, 2, 3, 4, 5, 10, 13, 257, 258, 259, 260, 261, 262, 516, 517, 518, 519, 520, 775} <= runs
    assert {(n - 1) % 258 for n in runs} >= {0, 1, 2, 3}
    f = R.filtered(by["literals 7x259/4"][0])
    assert {0, 143, 144, 255} <= set(f.reshape(-1).tolist())
    a, rpb = by["full band 8x2047/8"]
    assert rpb * (a.shape[1] + 1) == R.BAND_CAP


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_round_trips_and_stays_within_the_bound(case):
    from PIL import Image
    _, a, rpb = case
    z = R.zstream(a, rpb)
    f = R.filtered(a)
    assert zlib.decompress(z) == f.tobytes()
    assert z[:2] == b"\x78\x01" and z[-9:-4] == b"\x01\x00\x00\xff\xff" and z[-4:] == struct.pack(">I", zlib.adler32(f.tobytes()))
    assert len(z) <= R.bound(a.shape[0], f.shape[1] - 1, rpb)
    png = R.png_file(a, rpb)
    assert np.array_equal(R.read_png(png), a)
    with Image.open(io.BytesIO(png)) as im:
        assert im.mode == ("L" if a.ndim == 2 else "RGB") and np.array_equal(np.asarray(im), a)


def test_bound_formula_values():
    """2 + sum over the bands of (ceil((3 + 9 n + 7 + 3) / 8) + 4) + 5 + 4, and a band of nine-bit literals comes within its filter
    bytes' saving (they are 8-bit literals) of it."""
    assert R.bound(1024, 2048, 4) == 2 + 256 * ((13 + 9 * 8196 + 7) // 8 + 4) + 9
    assert R.bound(3, 5, 2) == 2 + ((13 + 9 * 12 + 7) // 8 + 4) + ((13 + 9 * 6 + 7) // 8 + 4) + 9
    assert R.bound(1, 1, 1) == 2 + (4 + 4) + 9
    d = np.tile((144 + np.arange(300) % 100).astype(np.uint32), (7, 1))
    a = np.cumsum(d, axis=0).astype(np.uint8)    # every filtered byte but the filter bytes is a literal in 144..255, no two neighbours equal
    f = R.filtered(a)
    assert (f[:, 1:] >= 144).all() and (np.diff(f.astype(np.int16), axis=1) != 0).all()
    assert 0 <= R.bound(7, 300, 7) - len(R.zstream(a, 7)) <= 1          # the seven filter bytes save a bit each


def test_reader_rejects_damage():
    a = np.arange(35, dtype=np.uint8).reshape(5, 7)
    png = bytearray(R.png_file(a, 2))
    assert np.array_equal(R.read_png(bytes(png)), a)
    idat = bytes(png).index(b"IDAT")
    n = struct.unpack(">I", png[idat - 4:idat])[0]

    def with_crc(body):
        return bytes(png[:idat + 4]) + body + struct.pack(">I", zlib.crc32(b"IDAT" + body)) + bytes(png[idat + 8 + n:])
    body = bytes(png[idat + 4:idat + 4 + n])
    flipped = bytearray(body)
    flipped[4] ^= 0x10                               # one payload bit, CRC made right again: the inflate or its Adler-32 must object
    with pytest.raises(zlib.error):
        R.read_png(with_crc(bytes(flipped)))
    wrong_adler = body[:-1] + bytes([body[-1] ^ 1])
    with pytest.raises(zlib.error):
        R.read_png(with_crc(wrong_adler))
    bad_crc = bytearray(png)
    bad_crc[idat + 4 + n] ^= 1
    with pytest.raises(ValueError, match="CRC"):
        R.read_png(bytes(bad_crc))
    with pytest.raises(ValueError, match="not a PNG"):
        R.read_png(b"\x00" + bytes(png[1:]))
