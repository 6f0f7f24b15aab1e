"""PNG files around a device-made IDAT stream (kernels.png_deflate / fs_png_deflate).

The device writes the zlib stream; what is left for the host is the part of a PNG that is a few dozen bytes: the signature, IHDR, the
IDAT chunk's length and CRC-32 (zlib.crc32 over the compressed bytes, which are small) and IEND."""
import struct
import zlib

from . import kernels as K

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)))


def png_bytes(height, width, channels, zstream):
    """The file of an 8-bit PNG of height x width pixels, channels 1 (grey, colour type 0) or 3 (RGB, colour type 2), whose one IDAT
    chunk is `zstream` (bytes-like: a complete zlib stream of the filtered scanlines)."""
    if channels not in (1, 3):
        raise ValueError("png_bytes: 1 or 3 channels, got %r" % (channels,))
    if height < 1 or width < 1:
        raise ValueError("png_bytes: bad size %r x %r" % (height, width))
    head = struct.pack(">IIBBBBB", int(width), int(height), 8, 0 if channels == 1 else 2, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", head) + _chunk(b"IDAT", bytes(zstream)) + _chunk(b"IEND", b"")


def encode_png(map, rows_per_band=None):
    """A uint8 device tensor (H, W) or (H, W, 3) -> the bytes of its PNG file, deflated on the device.  Synchronous (the stream and its
    length are read back): for tests and one-off use; PredictionWriter(device_png=True) is the pipelined form."""
    out, out_bytes = K.png_deflate(map, rows_per_band)
    n = int(out_bytes.item())
    return png_bytes(int(map.shape[0]), int(map.shape[1]), 1 if map.dim() == 2 else 3, out[:n].cpu().numpy().tobytes())

