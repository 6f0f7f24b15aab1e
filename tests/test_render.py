"""CPU: the contract of the prediction rendering (fs_render_prediction, fasterseg_amd.visualize, fasterseg_amd.tester) that needs no
device: the numpy restatement of tests/_render_ref.py against the fixture the reference produced (tests/golden/render.npz, made by
tools/make_render_golden.py), the rounding of the blend over every byte pair, print_iou's text, LabelSpec's tables, the ABI wiring,
and PredictionWriter's slot / worker logic on host arrays."""
import ctypes
import importlib.util
import os
import re
import threading

import numpy as np
import pytest

import _render_ref as R
from _util import GOLD, load_json, load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = os.path.join(GOLD, "cityscapes_labels.json")


def tables():
    return load_json("cityscapes_labels.json")


# ---- the restatement against the reference's outputs ----------------------------------------------------------------------------
def test_restatement_reproduces_the_fixture():
    g, t = load_npz("render.npz"), tables()
    pal, bg = t["colors"], t["background"]
    assert np.array_equal(R.show_prediction(pal, bg, g["img"], g["pred0"]), g["show_prediction"])
    assert np.array_equal(R.show_prediction(pal, bg, g["img"], g["pred0"], 0.55), g["show_prediction_055"])
    assert np.array_equal(R.show_img(pal, bg, g["img"], g["gt"], g["pred0"]), g["show_img_1"])
    assert np.array_equal(R.show_img(pal, bg, g["img"], g["gt"], g["pred0"], g["pred1"]), g["show_img_2"])
    H, W = g["img"].shape[:2]
    assert g["show_img_2"].shape == (H, 4 * W + 3 * R.PIVOT, 3) and (g["gt"] == 255).any()
    assert not g["show_img_1"][:, W:W + R.PIVOT].any()                     # the pivot is black


def test_reference_rerun_reproduces_the_fixture():
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    spec = importlib.util.spec_from_file_location("make_render_golden", os.path.join(ROOT, "tools", "make_render_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    arrays, tab = gen.run_reference()
    g = load_npz("render.npz")
    assert sorted(arrays) == sorted(g)
    for k in g:
        assert np.array_equal(np.asarray(arrays[k]), g[k], equal_nan=(g[k].dtype.kind == "f")), k
    assert tab == tables()


# ---- rounding contract of the blend ---------------------------------------------------------------------------------------------
def test_blend_rounding_over_every_byte_pair():
    c, o = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = R.blend(c, o, 0.55).astype(np.int64)
    exact = (11 * c + 9 * o + 10) // 20                     # floor(0.55 c + 0.45 o + 0.5) in integers
    tie = (11 * c + 9 * o) % 20 == 10
    assert np.array_equal(got[~tie], exact[~tie])
    assert np.abs(got - exact)[tie].max() <= 1
    share = tie.mean()
    assert share <= 0.08, share                              # the +-1 allowance cannot swallow a real error
    assert np.array_equal(np.diagonal(got), np.arange(256))  # c == o returns o
    assert np.array_equal(R.blend(c, o, 1).astype(np.int64), c)
    assert np.float32(0.55) + np.float32(1.0 - 0.55) == np.float32(1.0)
    # the stand-in cv2.addWeighted is the same arithmetic
    a = R.addWeighted(c.astype(np.uint8), 0.55, o.astype(np.uint8), 1 - 0.55, 0)
    assert np.array_equal(a, got.astype(np.uint8))


# ---- print_iou -------------------------------------------------------------------------------------------------------------------
def test_print_iou_text_equals_the_reference(capsys):
    from fasterseg_amd.visualize import print_iou
    g, t = load_npz("render.npz"), tables()
    iu, acc, want = g["iu"], float(g["acc"]), t["print_iou"]
    assert np.isnan(iu).any()
    assert print_iou(iu, acc, t["class_names"], True, no_print=True) == want["names_no_back"]
    assert print_iou(iu, acc, None, False, no_print=True) == want["plain"]
    assert print_iou(iu, acc, t["class_names"], no_print=True) == want["names"]
    assert "mean_IU_no_back\t%.3f%%" % (np.nanmean(iu[:-1]) * 100) in want["names_no_back"]
    capsys.readouterr()
    line = print_iou(iu, acc, t["class_names"], True)
    assert capsys.readouterr().out == line + "\n"


# ---- LabelSpec -------------------------------------------------------------------------------------------------------------------
def test_label_spec_tables():
    from fasterseg_amd.visualize import LabelSpec
    t = tables()
    spec = LabelSpec.from_json(LABELS)
    assert len(spec.label_ids) == 19 and spec.background == -1 and spec.class_names == t["class_names"]
    assert spec.lut.dtype == np.uint8 and spec.lut.shape == (256,)
    assert spec.lut[:19].tolist() == t["label_ids"] and spec.lut[19] == 0 and spec.lut[255] == 0 and not spec.lut[19:].any()
    assert spec.palette.shape == (19, 3) and spec.palette.tolist() == t["colors"]
    other = LabelSpec(t["colors"], t["class_names"], t["label_ids"], background=3, fill_id=7)
    assert other.lut[19] == 7 and other.lut[255] == 7 and other.background == 3
    with pytest.raises(ValueError):
        LabelSpec(t["colors"][:-1], t["class_names"], t["label_ids"])
    with pytest.raises(ValueError):
        LabelSpec(t["colors"], t["class_names"] + ["extra"], t["label_ids"])


# ---- ABI wiring ------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_struct_size():
    from fasterseg_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "fasterseg_hip.h")).read()
    assert re.search(r"fs_status fs_render_prediction\(", header) and "typedef struct fs_render_desc" in header
    assert "visualize.py:6-41" in header and "test.py:66-69" in header
    assert "fs_render_prediction" in _lib.ALL_SYMBOLS
    build.build(verbose=False)
    handle = _lib.lib()
    assert handle.fs_struct_size(9) == ctypes.sizeof(_lib.RenderDesc) == 4 * 9 + 3 * 4 * _lib.FS_RENDER_MAX_PANELS
    assert handle.fs_struct_size(10) == -1
    struct = re.search(r"typedef struct fs_render_desc \{(.*?)\} fs_render_desc;", header, re.S).group(1)
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    names = [re.sub(r"\[.*", "", n.strip()) for decl in re.findall(r"(?:int|float) ([^;]+);", struct) for n in decl.split(",")]
    assert names == [n for n, _ in _lib.RenderDesc._fields_]


# ---- PredictionWriter on host arrays ---------------------------------------------------------------------------------------------
def _fill(arrays):
    def render(views):
        for v, a in zip(views, arrays):
            v[...] = a
    return render


def test_prediction_writer_files_are_bit_identical(tmp_path):
    from PIL import Image
    from fasterseg_amd.tester import PredictionWriter
    rng = np.random.RandomState(3)
    frames = []
    with PredictionWriter(slots=2, workers=3, device=None) as w:
        for i in range(7):                                   # more submissions than slots: submit() waits for a free slot
            H, W = 5 + i, 17 + 3 * i                         # a slot grows with the frame; odd widths: padded rows
            ids = rng.randint(0, 34, size=(H, W)).astype(np.uint8)
            viz = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
            frames.append((ids, viz))
            w.submit([(str(tmp_path / ("f%d.png" % i)), (H, W)), (str(tmp_path / ("f%d.viz.png" % i)), (H, W, 3))], _fill([ids, viz]))
    assert sorted(os.listdir(tmp_path)) == sorted(["f%d.png" % i for i in range(7)] + ["f%d.viz.png" % i for i in range(7)])
    for i, (ids, viz) in enumerate(frames):
        a, b = Image.open(tmp_path / ("f%d.png" % i)), Image.open(tmp_path / ("f%d.viz.png" % i))
        assert a.mode == "L" and b.mode == "RGB"
        assert np.array_equal(np.asarray(a), ids) and np.array_equal(np.asarray(b), viz)


def test_prediction_writer_surfaces_a_failing_encode_in_close(tmp_path):
    from fasterseg_amd.tester import PredictionWriter
    done = []

    def encode(path, array):
        if path.endswith("bad.png"):
            raise OSError("disk full: " + path)
        done.append(path)
    w = PredictionWriter(slots=1, workers=2, device=None, encode=encode)
    one = np.zeros((4, 4), dtype=np.uint8)
    for name in ("a.png", "bad.png", "c.png", "d.png"):      # one slot: the failed job must give its slot back
        w.submit([(str(tmp_path / name), (4, 4))], _fill([one]))
    with pytest.raises(OSError, match="disk full"):
        w.close()
    assert sorted(os.path.basename(p) for p in done) == ["a.png", "c.png", "d.png"]
    with pytest.raises(RuntimeError):
        w.submit([(str(tmp_path / "e.png"), (4, 4))], _fill([one]))


def test_prediction_writer_never_reuses_a_slot_before_its_file_is_closed(tmp_path):
    from fasterseg_amd.tester import PredictionWriter
    release = threading.Event()
    seen = []

    def encode(path, array):
        if path.endswith("0.png"):
            release.wait(5)                                  # the first file is still being written ...
        seen.append((os.path.basename(path), int(array[0, 0])))
    w = PredictionWriter(slots=2, workers=2, device=None, encode=encode)
    big = PredictionWriter(slots=1, workers=64, device=None)
    assert len(w._threads) == 2 and len(big._threads) == 16          # capped, whatever the host has
    big.close()
    for i in range(2):
        w.submit([(str(tmp_path / ("%d.png" % i)), (2, 2))], _fill([np.full((2, 2), i, dtype=np.uint8)]))
    t = threading.Thread(target=lambda: w.submit([(str(tmp_path / "2.png"), (2, 2))], _fill([np.full((2, 2), 2, dtype=np.uint8)])))
    t.start()                                                # ... so the third frame takes the OTHER slot once frame 1 is done
    t.join(5)
    assert not t.is_alive()
    release.set()
    w.close()
    assert sorted(seen) == [("0.png", 0), ("1.png", 1), ("2.png", 2)]
