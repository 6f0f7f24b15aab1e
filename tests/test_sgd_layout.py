"""Host side of fs_sgd_momentum_multi, no launch: the descriptor optim.FlatSGD uploads, the number of blocks per tensor, and a Python model
of the kernel's chunk decode (csrc/optim.hip sgd_multi_kernel) that must cover every element of a tensor exactly once - the precedent
is tests/test_igemm2_index_model.py.  The model is tests/_sgd_ref.chunk_model; tests/test_flat_sgd_gpu.py runs the kernel on the same zoo.

Coverage is shown in two factors, which together are exact because a tiled block walks a full rectangle
(rows output channels) x (ni input channels) x (all taps):
  * the rectangles of a tensor's blocks tile the (O, I) plane exactly once (counted per (o, i));
  * inside a block, the kernel's three decodes - gradient order idx -> (row, tap, ii), the parameter rows' position `ii * taps + tap`
    staged through LDS, and the rotated pack's idx -> (row, pos) - are each one-to-one onto rows x ni x taps, with positions below the
    256 of an LDS row (decoded element by element for every (rows, ni, taps) the sweep produces).
The zoo's tensors are ALSO enumerated element by element through the whole chain, flat addresses included."""
import ctypes

import numpy as np
import pytest

from tests import _sgd_ref as R


def lib():
    from fasterseg_amd import _lib
    return _lib.lib()


class HeaderSgdTensor(ctypes.Structure):
    """include/fasterseg_hip.h, typedef struct fs_sgd_tensor, field by field"""
    _fields_ = [("p", ctypes.POINTER(ctypes.c_float)),          # float* p;
                ("g_off", ctypes.c_longlong),                   # long long g_off;
                ("numel", ctypes.c_longlong),                   # long long numel;
                ("I", ctypes.c_int),                            # int I;
                ("taps", ctypes.c_int),                         # int taps;
                ("pack_fwd", ctypes.c_void_p),                  # void* pack_fwd;
                ("pack_flip", ctypes.c_void_p)]                 # void* pack_flip;


def test_header_struct_is_the_one_written_here():
    """the ctypes structure above follows the header's declaration: same fields, same order, same C types"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fasterseg_hip.h")).read()
    body = re.search(r"typedef struct fs_sgd_tensor \{(.*?)\} fs_sgd_tensor;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [tuple(d.split()) for d in body.split(";") if d.strip()]
    assert decls == [("float*", "p"), ("long", "long", "g_off"), ("long", "long", "numel"), ("int", "I"), ("int", "taps"),
                     ("void*", "pack_fwd"), ("void*", "pack_flip")]
    assert [n for n, _ in HeaderSgdTensor._fields_] == [d[-1] for d in decls]


def test_numpy_descriptor_mirrors_the_c_struct():
    from fasterseg_amd import _lib, optim
    t = optim._TENSOR
    assert t.itemsize == lib().fs_struct_size(3) == ctypes.sizeof(HeaderSgdTensor) == ctypes.sizeof(_lib.SgdTensor)
    assert t.names == tuple(n for n, _ in HeaderSgdTensor._fields_)
    for name, ctype in HeaderSgdTensor._fields_:
        off, size = getattr(HeaderSgdTensor, name).offset, getattr(HeaderSgdTensor, name).size
        assert t.fields[name][1] == off == getattr(_lib.SgdTensor, name).offset, name
        assert t.fields[name][0].itemsize == size, name
        assert t.fields[name][0].kind == ("u" if name in ("p", "pack_fwd", "pack_flip") else "i"), name
        assert t.fields[name][0].byteorder in ("<", "=", "|")
    # a record written through numpy reads back through ctypes
    rec = np.zeros(1, t)
    rec[0] = (0x1122334455667788, -5, 1 << 40, 57, 9, 0x0102030405060708, 0x1112131415161718)
    c = HeaderSgdTensor.from_buffer_copy(rec.tobytes())
    assert (ctypes.cast(c.p, ctypes.c_void_p).value, c.g_off, c.numel, c.I, c.taps, c.pack_fwd, c.pack_flip) == tuple(int(v) for v in rec[0])


def test_chunk_elems():
    assert lib().fs_sgd_chunk_elems() == R.CHUNK == 4096


# ---- inside one block ----------------------------------------------------------------------------------------------------------------------
def block_decode(rows, ni, taps):
    """the kernel's decodes of one tiled block, element by element -> the LDS row length used.  Asserts each is one-to-one."""
    npos = ni * taps
    assert 0 < npos <= R.TILE_POS, (ni, taps)                                   # tile[16][257]: positions 0 .. 255 of a row
    assert 0 < rows <= R.TILE_O
    # phase 2: idx -> (r, tap, ii) in gradient order, reads / writes tile[r][ii * taps + tap]
    idx = np.arange(rows * npos)
    r, rem = idx // npos, idx % npos
    tap, ii = rem // ni, rem % ni
    pos = ii * taps + tap
    assert pos.max() < npos and r.max() < rows
    assert len(set(zip(r.tolist(), pos.tolist()))) == rows * npos               # every staged position updated once
    assert len(set(zip(r.tolist(), tap.tolist(), ii.tolist()))) == rows * npos  # every gradient element once
    # phase 3: idx -> (r, pos) for the rotated pack, r fastest over SGD_TO, rows beyond `rows` masked
    idx = np.arange(npos * R.TILE_O)
    r3, pos3 = idx % R.TILE_O, idx // R.TILE_O
    keep = r3 < rows
    ii3, tap3 = pos3[keep] // taps, pos3[keep] % taps
    assert ii3.max() < ni
    assert len(set(zip(r3[keep].tolist(), ii3.tolist(), (taps - 1 - tap3).tolist()))) == rows * npos
    return npos


_decoded = {}


def check_tensor(numel, I, taps, has_packs):
    """model against the library's count, (O, I) coverage, per-block decode.  -> the model"""
    model = R.chunk_model(numel, I, taps, has_packs)
    kind, chunks = model
    assert lib().fs_sgd_tensor_chunks(numel, I, taps, int(has_packs)) == len(chunks), (numel, I, taps, has_packs)
    if kind == "linear":
        assert taps == 1 and not has_packs
        assert chunks[0][0] == 0 and chunks[-1][1] == numel
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:])) and all(0 < e - b <= R.CHUNK for b, e in chunks)
        return model
    O = numel // (I * taps)
    seen = np.zeros((O, I), np.int32)
    for o0, rows, i0, ni in chunks:
        assert rows > 0 and ni > 0 and o0 + rows <= O and i0 + ni <= I
        seen[o0:o0 + rows, i0:i0 + ni] += 1
        key = (rows, ni, taps)
        if key not in _decoded:
            _decoded[key] = block_decode(*key)
        assert _decoded[key] <= R.TILE_POS
    assert (seen == 1).all(), (numel, I, taps, has_packs)
    return model


def test_sweep_counts_and_exact_coverage():
    n = 0
    for taps in (1, 3, 9, 25, 49, 256):
        for I in (1, 3, 27, 28, 29, 56, 57, 255, 256, 257):
            for O in range(1, 41):
                for has_packs in (0, 1):
                    kind, _ = check_tensor(O * I * taps, I, taps, has_packs)
                    assert kind == ("linear" if taps == 1 and not has_packs else "tiled")
                    n += 1
    print("sweep: %d tensors, %d distinct (rows, ni, taps) blocks decoded element by element" % (n, len(_decoded)))
    assert n == 6 * 10 * 40 * 2


@pytest.mark.parametrize("packs", [False, True], ids=["nopacks", "packs"])
def test_zoo_lands_on_its_branches(packs):
    """every zoo tensor takes the walk, and the ragged tiles, it is in the zoo for"""
    for shape, _, _, _, walk_plain, walk_packs, tiles, why in R.ZOO:
        numel, I, taps = R.geometry(shape)
        has = packs and R.packable(shape)
        kind, chunks = check_tensor(numel, I, taps, has)
        assert kind == (walk_packs if packs else walk_plain), (shape, why)
        if kind == "linear":
            want = tiles if isinstance(tiles, int) else -(-numel // R.CHUNK)     # a packable 1x1 without packs: `tiles` is for the packed walk
            assert len(chunks) == want == -(-numel // R.CHUNK), (shape, why)
            continue
        n_o, n_i, last_rows, last_ni = tiles
        assert len(chunks) == n_o * n_i, (shape, why)
        assert chunks[-1][1] == last_rows and chunks[-1][3] == last_ni, (shape, why, chunks[-1])
        assert chunks[0][1] == min(R.TILE_O, shape[0]) and chunks[0][3] == min(R.tile_i(taps), I)
    # the edges named in the zoo, from the tile rule itself
    it = R.tile_i
    assert it(1) == 256 and it(3) == 85 and it(9) == 28 and it(25) == 10 and it(49) == 5 and it(256) == 1
    shapes = set(R.SHAPES)
    assert {(16, 3, 3, 3), (17, 28, 3, 3), (5, 29, 3, 3), (33, 57, 3, 3), (3, 2, 16, 16), (16, 256, 1, 1), (24, 264, 1, 1)} <= shapes
    assert {(1,), (255,), (4096,), (4097,), (19, 7), (10, 12, 1, 1)} <= shapes and not R.packable((10, 12, 1, 1))


@pytest.mark.parametrize("packs", [False, True], ids=["nopacks", "packs"])
def test_zoo_flat_addresses_cover_every_element_once(packs):
    """the whole chain element by element: block -> (o, i, tap) -> the addresses the kernel forms in the parameter (OIHW), in the gradient
    / momentum / forward pack ([O][taps][I]) and in the rotated pack ([I][taps][O], tap reversed)"""
    for shape in R.SHAPES:
        numel, I, taps = R.geometry(shape)
        kind, chunks = R.chunk_model(numel, I, taps, packs and R.packable(shape))
        if kind == "linear":
            continue
        O, RSI = shape[0], taps * I
        par, grd, flp = (np.zeros(numel, np.int32) for _ in range(3))
        for o0, rows, i0, ni in chunks:
            npos = ni * taps
            idx = np.arange(rows * npos)
            r, rem = idx // npos, idx % npos
            tap, ii = rem // ni, rem % ni
            np.add.at(grd, (o0 + r) * RSI + tap * I + i0 + ii, 1)
            tid = np.arange(npos)                                                # phases 1 and 3: rows of npos contiguous parameters
            for rr in range(rows):
                np.add.at(par, (o0 + rr) * RSI + i0 * taps + tid, 1)
            idx = np.arange(npos * R.TILE_O)
            r3, pos3 = idx % R.TILE_O, idx // R.TILE_O
            keep = r3 < rows
            ii3, tap3 = pos3[keep] // taps, pos3[keep] % taps
            np.add.at(flp, ((i0 + ii3) * taps + (taps - 1 - tap3)) * O + o0 + r3[keep], 1)
        assert (par == 1).all() and (grd == 1).all() and (flp == 1).all(), shape


def test_model_addresses_are_the_reference_transposes():
    """the addresses above, applied to values, ARE packs64's transposes (one packed 3x3 filter, one value per element)"""
    import torch
    shape = (40, 32, 3, 3)
    numel, I, taps = R.geometry(shape)
    p = np.arange(numel, dtype=np.float64).reshape(shape)
    flat = p.reshape(-1)
    fwd, flip = np.full(numel, -1.0), np.full(numel, -1.0)
    O, RSI = shape[0], taps * I
    for o0, rows, i0, ni in R.chunk_model(numel, I, taps, True)[1]:
        for r in range(rows):
            for ii in range(ni):
                for tap in range(taps):
                    v = flat[(o0 + r) * RSI + i0 * taps + ii * taps + tap]
                    fwd[(o0 + r) * RSI + tap * I + i0 + ii] = v
                    flip[((i0 + ii) * taps + (taps - 1 - tap)) * O + o0 + r] = v
    want_fwd, want_flip = R.packs64(p, torch.float32)
    assert np.array_equal(fwd.astype(np.float32), want_fwd.view(np.float32).reshape(-1))
    assert np.array_equal(flip.astype(np.float32), want_flip.view(np.float32).reshape(-1))


# ---- filters the kernel cannot hold --------------------------------------------------------------------------------------------------------
def test_more_than_256_taps_is_refused():
    """taps > 256: one input channel's taps do not fit an LDS row.  The chunk function reports no blocks, and FlatSGD raises before it
    looks at the device (the parameters here live on the CPU: nothing is uploaded, nothing launched)."""
    import torch
    from fasterseg_amd.optim import MAX_TAPS, FlatSGD
    from fasterseg_amd.parallel import FlatGradientSync
    assert MAX_TAPS == R.TILE_POS
    for taps, I in ((257, 1), (289, 3), (1024, 8)):
        assert lib().fs_sgd_tensor_chunks(4 * I * taps, I, taps, 0) == 0
        assert lib().fs_sgd_tensor_chunks(8 * I * taps, I, taps, 1) == 0
        assert R.chunk_model(4 * I * taps, I, taps, False) is None
    assert lib().fs_sgd_tensor_chunks(3 * 2 * 256, 2, 256, 0) == 2               # 16 x 16 is the largest accepted
    ok = torch.nn.Parameter(torch.zeros(4, 3, 3, 3))
    big = torch.nn.Parameter(torch.zeros(2, 3, 17, 17))
    sync = FlatGradientSync([ok, big])
    with pytest.raises(ValueError, match=r"\(2, 3, 17, 17\)"):
        FlatSGD(sync, 0.1)
    wide = torch.nn.Parameter(torch.zeros(2, 1, 1, 257))
    with pytest.raises(ValueError, match=r"\(2, 1, 1, 257\)"):
        FlatSGD(FlatGradientSync([wide]), 0.1, pack_dtype=None)
    with pytest.raises(RuntimeError, match="HIP kernels only"):                  # a 16 x 16 filter passes the check and reaches the device test
        FlatSGD(FlatGradientSync([torch.nn.Parameter(torch.zeros(2, 3, 16, 16))]), 0.1)
