"""The fs_png_deflate stream format (include/fasterseg_hip.h) as a plain Python encoder, a minimal PNG reader and the test maps.

The encoder is the specification executed byte by byte, nothing of the kernel's structure in it: filter, cut into bands, cut a band into
runs, write tokens through a bit writer.  The reader walks the chunks with a CRC check, inflates IDAT with zlib (which verifies the
Adler-32) and undoes the filters with numpy."""
import struct
import zlib

import numpy as np

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
BAND_CAP = 16384          # FS_PNG_BAND_MAX_BYTES


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def lsb(self, value, n):             # extra bits, block headers: least significant bit first
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huffman(self, code, n):          # Huffman codes: most significant bit first
        self.lsb(int(format(code, "0%db" % n)[::-1], 2), n)

    def symbol(self, s):                 # the fixed literal / length code of RFC 1951 3.2.6
        if s < 144:
            self.huffman(0x30 + s, 8)
        elif s < 256:
            self.huffman(0x190 + s - 144, 9)
        elif s < 280:
            self.huffman(s - 256, 7)
        else:
            self.huffman(0xC0 + s - 280, 8)

    def match(self, length):             # (length, distance 1)
        k = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
        self.symbol(257 + k)
        self.lsb(length - LEN_BASE[k], LEN_EXTRA[k])
        self.huffman(0, 5)

    def align(self):
        if self.n:
            self.lsb(0, 8 - self.n)


def filtered(a):
    """(H, W) or (H, W, 3) uint8 -> (H, 1 + row_bytes) uint8: filter byte 2 and the row minus the row above."""
    rows = np.ascontiguousarray(a).reshape(a.shape[0], -1)
    up = np.vstack([np.zeros((1, rows.shape[1]), np.uint8), rows[:-1]])
    return np.hstack([np.full((rows.shape[0], 1), 2, np.uint8), rows - up])


def band_stream(f):
    """One band's filtered bytes -> its fixed-Huffman block and the empty stored block behind it."""
    w = _Bits()
    w.lsb(0, 1)
    w.lsb(1, 2)
    f = bytes(f)
    i = 0
    while i < len(f):
        j = i
        while j < len(f) and f[j] == f[i]:
            j += 1
        w.symbol(f[i])
        rest = j - i - 1
        for _ in range(rest // 258):
            w.match(258)
        r = rest % 258
        if r >= 3:
            w.match(r)
        else:
            for _ in range(r):
                w.symbol(f[i])
        i = j
    w.symbol(256)
    w.lsb(0, 3)
    w.align()
    return bytes(w.out) + b"\x00\x00\xff\xff"


def zstream(a, rows_per_band):
    f = filtered(a)
    out = b"\x78\x01"
    for r in range(0, f.shape[0], rows_per_band):
        out += band_stream(f[r:r + rows_per_band].tobytes())
    return out + b"\x01\x00\x00\xff\xff" + struct.pack(">I", zlib.adler32(f.tobytes()))


def bound(rows, row_bytes, rows_per_band):
    """fs_png_deflate_bound's formula."""
    total = 2 + 5 + 4
    for r in range(0, rows, rows_per_band):
        n = min(rows_per_band, rows - r) * (row_bytes + 1)
        total += -(-(3 + 9 * n + 7 + 3) // 8) + 4
    return total


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(a, rows_per_band):
    H, W = a.shape[:2]
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)) + \
        chunk(b"IDAT", zstream(a, rows_per_band)) + chunk(b"IEND", b"")


def read_png(data):
    """bytes of an 8-bit grey or RGB PNG -> (H, W) or (H, W, 3) uint8; ValueError for a bad CRC, zlib.error for a bad stream."""
    if data[:8] != SIGNATURE:
        raise ValueError("not a PNG")
    at, idat, head = 8, b"", None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(kind + body):
            raise ValueError("bad CRC in %r" % kind)
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        at += 12 + n
    W, H, depth, colour = head[:4]
    assert depth == 8 and colour in (0, 2) and head[4:] == (0, 0, 0)
    bpp = 3 if colour == 2 else 1
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * bpp)
    out = np.zeros((H, W * bpp), np.uint8)
    for y in range(H):
        kind, row = raw[y, 0], raw[y, 1:]
        if kind == 0:
            out[y] = row
        elif kind == 2:
            out[y] = row + (out[y - 1] if y else 0)
        elif kind == 1:
            acc = row.reshape(W, bpp).astype(np.uint32).cumsum(0)
            out[y] = acc.astype(np.uint8).reshape(-1)
        else:
            raise ValueError("filter %d is not read here" % kind)
    return out.reshape(H, W, 3) if bpp == 3 else out


# ---- the maps of the tests: (name, array, rows_per_band) -----------------------------------------------------------------------
def run_sweep(H, W):
    """Runs of 1-5, 10-13, 257-262, 516-520 and 775 equal FILTERED bytes in turn, wrapped over the rows (first row: the filtered
    bytes are the bytes; later rows are built as prefix sums so that their differences are the wanted runs)."""
    lengths = list(range(1, 6)) + list(range(10, 14)) + list(range(257, 263)) + list(range(516, 521)) + [775]
    flat, v = [], 1
    while len(flat) < H * W:
        for n in lengths:
            flat += [v] * n
            v = v % 250 + 1 if v != 2 else 3          # never 2: a run must not merge with a filter byte by accident
    d = np.array(flat[:H * W], np.uint8).reshape(H, W)
    return np.cumsum(d.astype(np.uint32), axis=0).astype(np.uint8)


def cases():
    rng = np.random.default_rng(20261021)
    out = []
    shapes = [(1, 1, 1), (1, 3, 1), (3, 5, 2), (7, 259, 4), (16, 1031, 5), (9, 2048, 3), (5, 600, 5)]
    for H, W, rpb in shapes:
        tag = "%dx%d/%d" % (H, W, rpb)
        out.append(("constant " + tag, np.full((H, W), 7, np.uint8), rpb))
        # row 0 all 2 and every later row 2 more: each filtered row is 2 2 2 ..., one run through the filter bytes
        out.append(("one run " + tag, (2 * (1 + np.arange(H)[:, None]) + np.zeros((1, W), np.int64)).astype(np.uint8), rpb))
        out.append(("sweep " + tag, run_sweep(H, W), rpb))
        edge = np.zeros((H, W), np.uint8)               # neighbouring 255 / 0 labels: literals 0, 255 and, one row down, 1 and 255
        edge[:, W // 2:] = 255
        edge[1::2] = 255 - edge[1::2]
        edge[:, ::7] = 143
        edge[:, 3::11] = 144
        out.append(("literals " + tag, edge, rpb))
        out.append(("noise " + tag, rng.integers(0, 256, (H, W), dtype=np.uint8), rpb))
        out.append(("19 classes " + tag, rng.integers(0, 19, (H, W), dtype=np.uint8), rpb))
    # a run cut by a band boundary: rows of zeros (filtered: 2 0 0 ...) in bands that end inside what would be one run of filter bytes
    cut = np.full((6, 1), 2, np.uint8) * (1 + np.arange(6, dtype=np.uint8))[:, None]
    out.append(("run cut by a band 6x1/4", cut, 4))
    out.append(("run cut by a band 7x259/4", np.full((7, 259), 3, np.uint8), 4))
    out.append(("rgb 4x37/3", rng.integers(0, 256, (4, 37, 3), dtype=np.uint8), 3))
    out.append(("rgb blocks 4x37/3", np.repeat(rng.integers(0, 4, (4, 4, 3), dtype=np.uint8), 10, axis=1)[:, :37].copy(), 3))
    out.append(("full band 8x2047/8", rng.integers(0, 3, (8, 2047), dtype=np.uint8), 8))      # 16384 filtered bytes: the cap
    return out
