"""Regenerates tests/golden/render.npz and tests/golden/cityscapes_labels.json from the UNMODIFIED reference (build container only).

    python tools/make_render_golden.py

The reference's tools/utils/visualize.py (show_prediction, show_img with one and two predictions and a ground truth holding 255s,
print_iou) is imported through oracle.ref_loader.reference("train") with the scratch copy's tools/ directory on sys.path, and run
with a stand-in `cv2` module in sys.modules (tests/_render_ref.py: what tests/cv2_numpy.py restates, plus addWeighted and imwrite).
Cityscapes.trans_labels, get_class_colors() and get_class_names() of tools/datasets/cityscapes give the label tables; background
is config.background of train/config_train.py:43 (-1).  Only data is written: inputs drawn here from a seed, the arrays and strings
the reference returned, and the tables.

addWeighted is restated from OpenCV 4's formula for 8-bit data, in its fp32 form with the contraction fixed (a fused multiply-add
behind a rounded product), and has NOT been checked against a cv2 build: none is installed where this runs.  Over all 65 536 byte
pairs at weight 0.55 the fused and the unfused form differ in 55 pairs, all of them exact ties of 0.55 c + 0.45 o."""
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W = 9, 21               # a few KB of fixture; odd sizes, more than one 16-pixel chunk per row
_PURGE = ("cv2", "utils", "utils.visualize", "datasets", "datasets.BaseDataset", "datasets.cityscapes", "datasets.cityscapes.cityscapes",
          "datasets.bdd", "datasets.bdd.bdd", "datasets.camvid", "datasets.camvid.camvid")


def inputs():
    rng = np.random.RandomState(20261018)
    img = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    pred0 = rng.randint(0, 19, size=(H, W)).astype(np.uint8)
    pred1 = rng.randint(0, 19, size=(H, W)).astype(np.uint8)
    gt = rng.randint(0, 19, size=(H, W)).astype(np.uint8)
    gt[rng.rand(H, W) < 0.2] = 255
    iu = rng.rand(19)
    iu[4] = np.nan                                   # a class that never occurs
    return {"img": img, "pred0": pred0, "pred1": pred1, "gt": gt, "iu": iu, "acc": np.float64(0.9123456)}


def run_reference():
    """(arrays, tables): what the reference computes from inputs(), and its Cityscapes tables with the print_iou strings."""
    import _render_ref as R
    from oracle import ref_loader
    x = inputs()
    saved = {k: sys.modules.get(k) for k in _PURGE}
    with ref_loader.reference("train") as wd:
        sys.path.insert(0, os.path.join(os.path.dirname(wd), "tools"))
        for k in _PURGE:
            sys.modules.pop(k, None)
        sys.modules["cv2"] = R.cv2_module()
        try:
            from utils import visualize as ref_vis
            from datasets.cityscapes import Cityscapes
            colors, names, ids = Cityscapes.get_class_colors(), Cityscapes.get_class_names(), list(Cityscapes.trans_labels)
            background = -1
            out = dict(x)
            out["show_prediction"] = ref_vis.show_prediction(colors, background, x["img"], x["pred0"])
            out["show_prediction_055"] = ref_vis.show_prediction(colors, background, x["img"], x["pred0"], 0.55)
            out["show_img_1"] = ref_vis.show_img(colors, background, x["img"], np.zeros((H, W)), x["gt"], x["pred0"])
            out["show_img_2"] = ref_vis.show_img(colors, background, x["img"], np.zeros((H, W)), x["gt"], x["pred0"], x["pred1"])
            lines = {"names_no_back": ref_vis.print_iou(x["iu"], float(x["acc"]), names, True, no_print=True),
                     "plain": ref_vis.print_iou(x["iu"], float(x["acc"]), None, False, no_print=True),
                     "names": ref_vis.print_iou(x["iu"], float(x["acc"]), names, False, no_print=True)}
        finally:
            for k in _PURGE:
                sys.modules.pop(k, None)
                if saved[k] is not None:
                    sys.modules[k] = saved[k]
    tables = {"class_names": list(names), "colors": [list(map(int, c)) for c in colors], "label_ids": [int(i) for i in ids],
              "background": background, "fill_id": 0, "print_iou": lines}
    return out, tables


def main():
    arrays, tables = run_reference()
    np.savez_compressed(os.path.join(GOLD, "render.npz"), **arrays)
    with open(os.path.join(GOLD, "cityscapes_labels.json"), "w") as f:
        text = json.dumps(tables, indent=1)
        f.write(re.sub(r"\[\s+((?:-?\d+,\s+)*-?\d+)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text) + "\n")
    print("wrote render.npz (%d arrays) and cityscapes_labels.json" % len(arrays))


if __name__ == "__main__":
    main()
