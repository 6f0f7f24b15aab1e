"""GPU: fs_png_deflate byte for byte against the reference encoder of tests/_png_ref.py (which tests/test_png_ref_selfcheck.py ties to
zlib and PIL).  The stream is fully specified - filter, bands, tokens, bit order, checksum - so no tolerance applies.  Every stream is
written into a sentinel-filled buffer: nothing behind its last byte, and so nothing behind out[bound], may change.  The shapes are the
smallest at which each mechanism can break: one byte, a row shorter than a 16-byte load, a short last band, rows that are no multiple
of 16 bytes, more bands than one, a band of exactly the LDS cap."""
import io

import numpy as np
import pytest
import torch

from tests import _png_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
CASES = R.cases()


def _deflate(view, rpb):
    """kernels.png_deflate into guard-banded buffers -> (stream bytes, bound); asserts the guards."""
    from fasterseg_amd import kernels as K
    H = view.shape[0]
    row_bytes = view.shape[1] * (3 if view.dim() == 3 else 1)
    bound, ws = K.png_deflate_sizes(H, row_bytes, rpb)
    assert bound == R.bound(H, row_bytes, rpb)
    buf = torch.full((16 + bound + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    wsb = torch.full((ws + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    n = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    K.png_deflate(view, rpb, out=buf[16:16 + bound], workspace=wsb[:ws], out_bytes=n[1:2])
    got, count = buf.cpu().numpy(), n.cpu().numpy()
    assert count[0] == -7 and count[2] == -7 and 11 <= count[1] <= bound
    assert (got[:16] == SENTINEL).all() and (got[16 + count[1]:] == SENTINEL).all(), "bytes outside the stream were written"
    assert (wsb[ws:].cpu().numpy() == SENTINEL).all(), "bytes behind the workspace were written"
    return got[16:16 + count[1]].tobytes(), bound


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stream_is_the_reference_stream(case):
    _, a, rpb = case
    got, _ = _deflate(torch.from_numpy(a).cuda(), rpb)
    want = R.zstream(a, rpb)
    assert len(got) == len(want), (len(got), len(want))
    assert got == want, np.flatnonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[:8]


@pytest.mark.parametrize("pad", [13, "16"])
def test_pitched_views(pad):
    """Rows inside a wider buffer: pitch = W + 13 (every row at another alignment) and a pitch rounded up to 16; the view starts one
    byte into the buffer in the first form."""
    rng = np.random.default_rng(77)
    for H, W, rpb in ((7, 259, 4), (16, 1031, 5), (3, 5, 2)):
        pitch = W + 13 if pad == 13 else (W + 15) // 16 * 16
        lead = 1 if pad == 13 else 0
        host = rng.integers(0, 4, (lead + H * pitch,), dtype=np.uint8)
        view = torch.from_numpy(host).cuda()[lead:].view(H, pitch)[:, :W]
        a = host[lead:].reshape(H, pitch)[:, :W]
        got, _ = _deflate(view, rpb)
        assert got == R.zstream(a, rpb), (H, W, rpb, pitch)


def test_two_calls_give_identical_bytes_and_the_default_band():
    from fasterseg_amd import kernels as K
    rng = np.random.default_rng(3)
    a = np.repeat(np.repeat(rng.integers(0, 19, (33, 40), dtype=np.uint8), 8, axis=0), 13, axis=1)[:259, :517].copy()    # a blocky class map
    dev = torch.from_numpy(a).cuda()
    rpb = K.png_rows_per_band(259, 517)
    assert rpb == 1
    first, n1 = K.png_deflate(dev)
    second, n2 = K.png_deflate(dev)
    assert int(n1) == int(n2) and torch.equal(first[:int(n1)], second[:int(n1)])
    assert first[:int(n1)].cpu().numpy().tobytes() == R.zstream(a, rpb)


@pytest.mark.parametrize("case", [c for c in CASES if c[0].split()[0] in ("sweep", "noise", "rgb", "literals")], ids=lambda c: c[0])
def test_encode_png_decodes_to_the_input(case):
    from PIL import Image
    from fasterseg_amd.png import encode_png
    _, a, rpb = case
    data = encode_png(torch.from_numpy(a).cuda(), rpb)
    assert data == R.png_file(a, rpb)
    assert np.array_equal(R.read_png(data), a)
    with Image.open(io.BytesIO(data)) as im:
        assert im.mode == ("L" if a.ndim == 2 else "RGB") and np.array_equal(np.asarray(im), a)


def test_many_bands_per_pack_block():
    """More bands than the pack launch has blocks (1024): a block walks several bands, the last blocks none."""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 3, (1100, 9), dtype=np.uint8)
    a[400:700] = 5
    got, _ = _deflate(torch.from_numpy(a).cuda(), 1)
    assert got == R.zstream(a, 1)
