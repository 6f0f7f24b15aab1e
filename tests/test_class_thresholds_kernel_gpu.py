"""fs_bilinear_argmax_conf_pc and fs_score_confidence_pc against the scalar forms, bit for bit: every case of tests/_confidence_ref.CASES
(x8 strip, tight stride, several blocks, generic ratio, C = 21, down-sample, one class, two classes) in the three storage types, in guarded
output buffers.  The confidence map never depends on the table; a table of equal entries gives the scalar form's class map; a table that
differs per class gives where(conf >= table[arg], arg, ignore_label) with arg from fs_bilinear_argmax; entries >= C are never read."""
import numpy as np
import pytest
import torch

from tests import _confidence_ref as CR

pytestmark = pytest.mark.gpu

DTYPES = ("fp32", "bf16", "fp16")
GUARD = 64


def _view(buf, C, dtype):
    t = torch.from_numpy(buf).to(CR.TORCH[dtype]).cuda()
    return t.permute(0, 3, 1, 2)[:, :C]


def _guarded(shape):
    """a uint8 map inside a sentinel-filled buffer: (map view, check that nothing outside it was written)"""
    n = int(np.prod(shape))
    pad = -n % 16
    buf = torch.full((GUARD + n + pad + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def intact():
        return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + n:] == 0xA5).all())
    return buf[GUARD:GUARD + n].view(shape), intact


def _run(x, size, **kw):
    from fasterseg_amd import kernels as K
    N = x.shape[0]
    classes, c_ok = _guarded((N,) + tuple(size))
    conf, q_ok = _guarded((N,) + tuple(size))
    K.bilinear_argmax_conf(x, size, classes=classes, conf=conf, **kw)
    torch.cuda.synchronize()
    assert c_ok() and q_ok(), "a store outside the maps"
    return classes, conf


def _table(entries):
    """256 raw bytes on the device (not through class_threshold_table: the pad-lane test sets the entries >= C)"""
    t = np.zeros(256, dtype=np.uint8)
    t[:len(entries)] = entries
    return torch.from_numpy(t).cuda()


def _where(conf, arg, table, ignore):
    return torch.where(conf >= table[arg.long()], arg, torch.full_like(arg, ignore))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", sorted(CR.CASES))
def test_bilinear_argmax_conf_pc(case, dtype):
    from fasterseg_amd import kernels as K
    buf, C = CR.logits(case, dtype)
    size = CR.CASES[case][4]
    x = _view(buf, C, dtype)
    arg = K.bilinear_argmax(x, size)
    plain, conf = (t.clone() for t in _run(x, size))
    assert torch.equal(plain, arg)
    # uniform tables: both maps are the scalar launch's
    for m in (0, 128, 230):
        want_c, want_q = (t.clone() for t in _run(x, size, min_confidence=m / 255))
        got_c, got_q = _run(x, size, class_thresholds=K.class_threshold_table(np.full(C, m, dtype=np.uint8), C, "cuda"))
        assert torch.equal(got_q, want_q) and torch.equal(got_q, conf), (m, int((got_q != want_q).sum()))
        assert torch.equal(got_c, want_c), (m, int((got_c != want_c).sum()))
    # a table that differs per class: entry k is the largest byte class k has, so each class keeps its surest pixels only
    a, q = arg.cpu().numpy(), conf.cpu().numpy()
    present = [k for k in range(C) if (a == k).any()]
    top = np.zeros(C, dtype=np.uint8)
    for k in present:
        top[k] = q[a == k].max()
    table = K.class_threshold_table(top, C, "cuda")
    assert torch.equal(table.cpu(), torch.from_numpy(np.concatenate([top, np.zeros(256 - C, dtype=np.uint8)])))
    for ignore in (255, 254):
        got_c, got_q = _run(x, size, class_thresholds=table, ignore_label=ignore)
        assert torch.equal(got_q, conf)
        assert torch.equal(got_c, _where(conf, arg, table, ignore)), (ignore, int((got_c != _where(conf, arg, table, ignore)).sum()))
        if C >= 2:
            g = got_c.cpu().numpy()
            assert present == list(range(C)), "a class of the case is absent"
            for k in range(C):
                kept, dropped = int(((a == k) & (g == k)).sum()), int(((a == k) & (g == ignore)).sum())
                assert kept > 0 and dropped > 0 and kept + dropped == int((a == k).sum()), (k, kept, dropped)
            assert len(np.unique(top)) > 1 or C == 2
    # pad lanes never index the table: entries >= C at 255, the real ones at 0, and nothing is masked
    pads = _table([0] * C + [255] * (256 - C))
    got_c, got_q = _run(x, size, class_thresholds=pads)
    assert torch.equal(got_c, arg) and torch.equal(got_q, conf)
    # either output alone
    only_c, none = K.bilinear_argmax_conf(x, size, class_thresholds=table, conf=False)
    none2, only_q = K.bilinear_argmax_conf(x, size, class_thresholds=table, classes=False)
    assert none is None and none2 is None
    assert torch.equal(only_c, _where(conf, arg, table, 255)) and torch.equal(only_q, conf)


@pytest.mark.parametrize("C,cs", [(19, 20), (19, 32), (3, 4)])
@pytest.mark.parametrize("pixels", [1, 255, 4096 + 3])
def test_score_confidence_pc(pixels, C, cs):
    from fasterseg_amd import kernels as K
    rng = np.random.default_rng(pixels * 100 + cs)
    score = np.full((pixels, cs), 1e30, dtype=np.float32)
    score[:, :C] = np.exp(2.0 * rng.standard_normal((pixels, C))).astype(np.float32)
    if pixels > 4:
        score[1, :C] = 0.0                               # a row of zeros
        score[2, min(1, C - 1)] = np.inf                 # a row with an inf
        score[3, :C] = score[3, 0]                       # exact ties over the whole row: the lowest index wins
        score[4, C - 1] = score[4, :C].max()             # ... and a two-way tie of the maximum
    dev = torch.from_numpy(score).cuda()
    arg, conf = K.score_confidence(dev, C)
    if pixels > 4:
        assert int(conf[1]) == 0 and int(conf[2]) == 0 and int(arg[3]) == 0 and int(arg[2]) == min(1, C - 1)
        assert int(arg[4]) == int(np.argmax(score[4, :C]))

    def run(**kw):
        classes, c_ok = _guarded((pixels,))
        q, q_ok = _guarded((pixels,))
        K.score_confidence(dev, C, classes=classes, conf=q, **kw)
        torch.cuda.synchronize()
        assert c_ok() and q_ok(), "a store outside the maps"
        return classes, q
    for m in (0, 128, 230):
        want_c, want_q = K.score_confidence(dev, C, min_confidence=m / 255, ignore_label=254)
        got_c, got_q = run(class_thresholds=K.class_threshold_table(np.full(C, m, dtype=np.uint8), C, "cuda"), ignore_label=254)
        assert torch.equal(got_q, want_q) and torch.equal(got_q, conf) and torch.equal(got_c, want_c), m
    # per class: the median byte of each class (0 for a class no pixel has), then a seeded table of any bytes
    a, q = arg.cpu().numpy(), conf.cpu().numpy()
    med = np.array([int(np.median(q[a == k])) if (a == k).any() else 0 for k in range(C)], dtype=np.uint8)
    for entries in (med, rng.integers(0, 256, size=C).astype(np.uint8)):
        table = K.class_threshold_table(entries, C, "cuda")
        for ignore in (255, 254):
            got_c, got_q = run(class_thresholds=table, ignore_label=ignore)
            assert torch.equal(got_q, conf) and torch.equal(got_c, _where(conf, arg, table, ignore)), (entries, ignore)
    if pixels > 255:
        g = run(class_thresholds=K.class_threshold_table(med, C, "cuda"))[0].cpu().numpy()
        both = [k for k in range(C) if ((a == k) & (g == k)).any() and ((a == k) & (g == 255)).any()]
        assert len(both) >= 2, both
    got_c, got_q = run(class_thresholds=_table([0] * C + [255] * (256 - C)))
    assert torch.equal(got_c, arg) and torch.equal(got_q, conf)
    only_c, none = K.score_confidence(dev, C, class_thresholds=table, conf=False)
    none2, only_q = K.score_confidence(dev, C, class_thresholds=table, classes=False)
    assert none is None and none2 is None and torch.equal(only_c, _where(conf, arg, table, 255)) and torch.equal(only_q, conf)
