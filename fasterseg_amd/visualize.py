"""Predictions as pictures (drop-in for the reference's tools/utils/visualize.py: set_img_color, show_prediction, show_img,
print_iou), with the per-pixel work on the device.

The reference paints on the host: per panel one np.where pass per class and a cv2.addWeighted (visualize.py:6-41).  Here a
whole composite - the image, every prediction panel, the ground-truth panel, the black pivots - is ONE fs_render_prediction
launch (render.hip); images and class maps may be device tensors or numpy arrays, the result is a uint8 (H, Wtotal, 3) RGB
device tensor.  The package ships no label tables: callers pass colours / names / ids, or a JSON file (LabelSpec.from_json)."""
import json

import numpy as np
import torch

from . import kernels as K

PIVOT = 15                  # black columns between the panels of show_img (visualize.py:29)
_MAX = 4                    # overlay panels of one launch (FS_RENDER_MAX_PANELS)


class LabelSpec:
    """The label tables of a dataset: per train id a colour (RGB), a name and the label id of the submission format
    (train/test.py:25-46); `background` is the class that is never painted (config.background, -1: none) and `fill_id` the
    label id of every class value without an entry (the reference maps 19 -> 0)."""

    def __init__(self, colors, class_names, label_ids, background=-1, fill_id=0):
        n = len(label_ids)
        if len(colors) != n or len(class_names) != n:
            raise ValueError("LabelSpec: %d colours, %d names and %d label ids" % (len(colors), len(class_names), n))
        if not 0 < n <= 256:
            raise ValueError("LabelSpec: 1..256 classes, got %d" % n)
        self.colors = [[int(c) for c in rgb] for rgb in colors]
        self.class_names = [str(s) for s in class_names]
        self.label_ids = [int(i) for i in label_ids]
        self.background = int(background)
        self.fill_id = int(fill_id)
        self.palette = np.asarray(self.colors, dtype=np.uint8).reshape(n, 3)
        self.lut = np.full(256, self.fill_id, dtype=np.uint8)
        self.lut[:n] = np.asarray(self.label_ids, dtype=np.uint8)
        self._device = {}

    @classmethod
    def from_json(cls, path):
        """{"colors": [[r, g, b], ...], "class_names": [...], "label_ids": [...], "background": -1, "fill_id": 0}; the last two are
        optional, other keys are ignored."""
        with open(path) as f:
            d = json.load(f)
        return cls(d["colors"], d["class_names"], d["label_ids"], d.get("background", -1), d.get("fill_id", 0))

    def tables(self, device):
        """(palette (n, 3), lut (256,)) uint8 tensors on `device` (uploaded once)."""
        device = torch.device(device)
        t = self._device.get(device)
        if t is None:
            t = self._device[device] = (torch.from_numpy(self.palette).to(device), torch.from_numpy(self.lut).to(device))
        return t


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device())


def _u8(x, device):
    t = torch.as_tensor(x)
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)            # class maps arrive as int64 from np.argmax; 255 and -1 both become 255
    return t.to(device).contiguous()


def _palette(colors, device):
    if isinstance(colors, LabelSpec):
        return colors.tables(device)[0]
    return torch.from_numpy(np.ascontiguousarray(np.asarray(colors, dtype=np.uint8).reshape(-1, 3))).to(device)


def padded_rows(H, Wt, device):
    """An (H, Wt, 3) uint8 view whose rows start 16 bytes aligned (the pitch is rounded up): what the render kernel writes fastest."""
    pitch = K.round_up(3 * Wt, 16)
    return torch.empty((H, pitch), dtype=torch.uint8, device=device)[:, :3 * Wt].unflatten(1, (Wt, 3))


def compose(colors, background, img, maps, show255, weights, image_panel=False, out=None, lut=None, ids=None):
    """The panels of `maps` (and the image first, with image_panel) side by side; launches of up to 4 overlay panels chained into
    one composite.  out: an (H, Wtotal, 3) view to render into (default: a fresh padded_rows); lut / ids: the label-ID map of
    maps[0] from the first launch."""
    device = _device_of(img, *maps)
    img = _u8(img, device)
    maps = [_u8(m, device) for m in maps]
    H, W = int(img.shape[0]), int(img.shape[1])
    P = len(maps) + int(bool(image_panel))
    Wt = W * P + PIVOT * (P - 1)
    if out is None:
        out = padded_rows(H, Wt, device)
    if len(maps) > _MAX:
        out.zero_()                      # the pivot between two launches' panels belongs to neither
    pal = _palette(colors, device)
    col, first = 0, True
    for i in range(0, max(len(maps), 1), _MAX):
        span = K.render_prediction(img, maps[i:i + _MAX], pal, out, col=col, image_panel=image_panel and first, gap=PIVOT,
                                   background=background, show255=show255[i:i + _MAX], weights=weights[i:i + _MAX],
                                   lut=lut if first else None, ids=ids if first else None)
        col += span + PIVOT
        first = False
    return out


def set_img_color(colors, background, img, gt, show255=False, weight_foreground=0.55):
    """visualize.py:6-14: `img` painted by the classes of `gt` and blended with itself, IN PLACE (numpy array or device tensor)."""
    out = compose(colors, background, img, [gt], [show255], [weight_foreground])
    if torch.is_tensor(img):
        img.copy_(out)
    else:
        img[...] = out.cpu().numpy()
    return img


def show_prediction(colors, background, img, pred, weight_foreground=1):
    """visualize.py:17-21: the image painted by the prediction (weight 1: the colours replace the image where a class paints)."""
    return compose(colors, background, img, [pred], [False], [weight_foreground])


def show_img(colors, background, img, clean, gt, *pds):
    """visualize.py:24-41: image | one panel per prediction | ground truth (label 255 black), 15 black columns between them.
    `clean` is not used (nor by the reference).  One launch for up to 3 predictions."""
    maps = list(pds) + [gt]
    return compose(colors, background, img, maps, [False] * len(pds) + [True], [0.55] * len(maps), image_panel=True)


def print_iou(iu, mean_pixel_acc, class_names=None, show_no_back=False, no_print=False):
    """visualize.py:61-89, line for line the same text: one line per class, then the means (mean_IU_no_back leaves out the LAST
    class, as the reference does)."""
    iu = np.asarray(iu)
    rows = []
    for i in range(iu.size):
        head = ("Class %d:" % (i + 1)) if class_names is None else ("%d %s" % (i + 1, class_names[i]))
        rows.append("%-8s\t%.3f%%" % (head, iu[i] * 100))
    cells = [("mean_IU", np.nanmean(iu))]
    if show_no_back:
        cells.append(("mean_IU_no_back", np.nanmean(iu[:-1])))
    else:
        print(mean_pixel_acc)
    cells.append(("mean_pixel_ACC", mean_pixel_acc))
    rows.append("----------------------------     " + "\t".join("%-8s\t%.3f%%" % (k, v * 100) for k, v in cells))
    line = "\n".join(rows)
    if not no_print:
        print(line)
    return line
