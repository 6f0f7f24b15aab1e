"""The launch form of the LDS-halo 3x3 kernel (fs_conv3x3_halo_plan, host only: the library loads without a GPU).

Decomposition rule: a launch-latency-sized layer takes about one workgroup's latency until workgroups exceed CUs, so the form to pick
puts at least half of the MI355X's 256 CUs in flight.  The ten 3x3 layers of the searched student (arch_1 at 1x3x1024x2048) that run on
maps of <= 32 x 64 pixels must therefore launch >= 128 workgroups, in bf16 (32-channel chunks) and fp32 (16-channel chunks); a
128 x 256 map, where the plain form already fills the chip, keeps the plain form.

The in-block K-split form with 32-channel tiles gives 128 .. 384 workgroups on eight of the ten layers and 64 on the two 128->128
@16x32 layers (16 m-tiles x 4 n-tiles); there the rule takes the 16-channel tiles (128 workgroups)."""
import ctypes

import pytest

SMALL_MAP_LAYERS = [
    # Cin, Cout, H, W
    (256, 256, 16, 32), (128, 256, 16, 32), (128, 128, 16, 32), (128, 128, 16, 32),
    (192, 192, 32, 64), (192, 128, 32, 64), (128, 128, 32, 64), (128, 128, 32, 64),
    (64, 192, 32, 64), (64, 128, 32, 64),
]


def plan(cin, cout, H, W, dtype, flags=0, stride=1, has_stats=0):
    from fasterseg_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = _lib.ConvDesc(1, H, W, cin, cout, 3, 3, stride, 1, Ho, Wo, cin, cout, dtype, flags)
    tile, ks, wg = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    status = h.fs_conv3x3_halo_plan(ctypes.byref(d), has_stats, ctypes.byref(tile), ctypes.byref(ks), ctypes.byref(wg))
    return status, tile.value, ks.value, wg.value


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
@pytest.mark.parametrize("layer", SMALL_MAP_LAYERS, ids=["%d-%d@%dx%d" % l for l in SMALL_MAP_LAYERS])
def test_small_map_layers_fill_half_the_chip(layer, dtype):
    status, tile, ks, wg = plan(*layer, dtype)
    print("layer %s: tile %d, ksplit %d, %d workgroups" % (layer, tile, ks, wg))
    assert status == 0 and ks == 1
    assert wg >= 128, "%d workgroups on 256 CUs" % wg


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "bf16"])
def test_large_map_keeps_the_plain_form(dtype):
    for cin, cout in ((32, 64), (64, 64), (128, 128), (192, 128)):
        status, tile, ks, wg = plan(cin, cout, 128, 256, dtype)
        assert status == 0 and ks == 0 and wg >= 256, (cin, cout, tile, ks, wg)


def test_forced_forms_and_training_calls():
    from fasterseg_amd import _lib
    KS, NO = _lib.FS_CONV_KSPLIT, _lib.FS_CONV_NO_KSPLIT
    assert plan(128, 128, 128, 256, 1, flags=KS)[1:] == (32, 1, 64 * 16 * 4)          # forced on a large map
    assert plan(256, 256, 16, 32, 1, flags=NO)[2] == 0                                 # forbidden on a small one
    assert plan(256, 256, 16, 32, 1, flags=0x1000)[1:3] == (32, 0)                     # a forced tile pins the plain form
    assert plan(256, 256, 16, 32, 1, has_stats=1)[2] == 0                              # BN statistics: never selected ..
    assert plan(256, 256, 16, 32, 1, flags=KS, has_stats=1)[0] == 2                    # .. and refused when forced (FS_ERR_UNSUPPORTED)
    assert plan(64, 64, 32, 64, 1, flags=KS, stride=2)[0] == 2
    assert plan(64, 64, 32, 64, 1, flags=KS | NO)[0] == 1
    assert plan(32, 64, 16, 32, 1)[2] == 0                                             # one chunk: nothing to share
    assert plan(128, 128, 16, 32, 1)[1:] == (16, 1, 128)                               # 32-channel tiles would be 64 blocks
    assert plan(128, 128, 16, 32, 1, flags=KS)[1:] == (32, 1, 64)
    assert plan(128, 128, 32, 64, 1, flags=_lib.FS_CONV_KSPLIT16)[1:] == (16, 1, 16 * 4 * 8)
