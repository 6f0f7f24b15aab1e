"""Records tests/golden/stem_parent.npz: what the bf16 matrix-core stem writes for the seeded cases of tests/_stem_cases.py.

    python tools/make_stem_golden.py [out.npz]        (needs an MI355X)

Run ONCE with the library of the commit BEFORE the stem became a multi-tile, software-pipelined kernel (one 4 x 64 tile per block):
tests/test_stem_pipelined_gpu.py asks the present kernel for the same bits.  Only data is written: per case the bf16 bit patterns as
uint16, whole up to GOLDEN_FULL_BELOW elements and every GOLDEN_STRIDE-th element of the flat (N, Ho, Wo, C) order above that."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import _stem_cases as S
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "stem_parent.npz")
    arrays = {}
    for cout in S.COUTS:
        for image in S.IMAGES:
            arrays[S.case_id(cout, image)] = S.golden_sample(S.run(cout, image)).numpy().view(np.uint16)
    np.savez_compressed(out, **arrays)
    print("wrote %s: %d cases, %d values, %d bytes" % (out, len(arrays), sum(a.size for a in arrays.values()), os.path.getsize(out)))


if __name__ == "__main__":
    main()
