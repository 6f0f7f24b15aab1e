"""The multi-tile, software-pipelined bf16 stem (csrc/stem.hip, stem_mfma_kernel: a block walks several 4 x 64 tiles, filter fragments
split once per block, window double-buffered, the next tile's image loads in flight under the current tile's MFMAs).

It changes scheduling only, so its outputs must be the single-tile kernel's bit for bit: against tests/golden/stem_parent.npz (what
the kernel of the commit before wrote for the seeded cases of tests/_stem_cases.py, tools/make_stem_golden.py) and between grids - the
default one, 3 blocks (every block walks >= 15 tiles of the 2x3x70x520 case, alternating both window buffers many times) and 1 block."""
import pytest
import torch
import torch.nn.functional as F

from tests import _stem_cases as S
from tests._util import load_npz
from tests.test_kernels_gpu import check, q

pytestmark = pytest.mark.gpu

CASES = [(c, im) for c in S.COUTS for im in S.IMAGES]


@pytest.mark.parametrize("cout,image", CASES, ids=[S.case_id(c, im) for c, im in CASES])
def test_pipelined_stem(cout, image):
    from fasterseg_amd import _lib
    lib = _lib.lib()
    x, w, scale, shift = S.inputs(cout, image)
    ref = F.relu(F.conv2d(x, w, None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    try:
        lib.fs_debug_stem_blocks(0)
        default = S.run(cout, image)
        lib.fs_debug_stem_blocks(3)
        three = S.run(cout, image)
        lib.fs_debug_stem_blocks(1)
        one = S.run(cout, image)
    finally:
        lib.fs_debug_stem_blocks(0)
    n, ho, wo = ref.shape[0], ref.shape[2], ref.shape[3]
    got = default.view(torch.bfloat16).reshape(n, ho, wo, cout).permute(0, 3, 1, 2)
    check(got, q(ref, torch.bfloat16), torch.bfloat16, "pipelined stem")
    assert torch.equal(default, three), "3 blocks: %d values differ from the default grid" % int((default != three).sum())
    assert torch.equal(default, one), "1 block: %d values differ from the default grid" % int((default != one).sum())
    want = torch.from_numpy(load_npz("stem_parent.npz")[S.case_id(cout, image)].view("int16"))
    sample = S.golden_sample(default)
    assert sample.shape == want.shape
    assert torch.equal(sample, want), "%d of %d sampled values differ from the single-tile kernel's" % (int((sample != want).sum()), want.numel())
