"""ms per training batch of the device input pipeline (fasterseg_amd.dataloader: fs_train_batch, and fs_resize_u8 for host-resident
sources) for the benchmarked train workloads, and GB/s of its algorithmic bytes (sources read + outputs written).

Presets (the reference's configs, train_scale_array [0.75, 1, 1.25], seeded 1024 x 2048 uint8 sources, one per batch slot):
  C4  12 x (1024x2048, down_sampling 1) -> 512x1024 crops, labels at gt_down_sampling 1   (train/config_train.py)
  C3   3 x (1024x2048, down_sampling 2) -> 256x512 crops, labels at 1/8                     (search/config_search.py, pretrain)
  C5   2 x (1024x2048, down_sampling 2) -> 224x448 crops, labels at 1/8                     (search/config_search.py, search)
Per preset and residency:
  device  sources uploaded and down-sampled once (ArraySource): a batch is one fs_train_batch launch;
  host    pinned host sources (ArraySource(resident=False)): every batch uploads its B full-size sources and, at d = 2, down-samples
          them on the device before the launch.
batch_ms: device events around `--batches` consecutive batches (no synchronisation between them) / batches.
kernel_ms: fs_train_batch's own device time per launch under the library's census (level 2), with its GB/s.
Prints one JSON line per preset; --out writes them all to a file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEAN, STD = np.array([0.485, 0.456, 0.406]), np.array([0.229, 0.224, 0.225])
PRESETS = {"C4": (12, 1, 512, 1024, 1), "C3": (3, 2, 256, 512, 8), "C5": (2, 2, 224, 448, 8)}     # B, d, crop_h, crop_w, g


class Cfg:
    def __init__(self, B, d, h, w, g):
        self.batch_size, self.down_sampling, self.image_height, self.image_width, self.gt_down_sampling = B, d, h, w, g
        self.train_scale_array = [0.75, 1, 1.25]
        self.image_mean, self.image_std = MEAN, STD
        self.niters_per_epoch = None


def measure(name, resident, images, labels, batches, warmup):
    from fasterseg_amd import census as C
    from fasterseg_amd.dataloader import ArraySource, DeviceTrainLoader
    from fasterseg_amd.devtime import block_ms
    B, d, h, w, g = PRESETS[name]
    cfg = Cfg(B, d, h, w, g)
    src = ArraySource(images[:B], labels[:B], down_sampling=d, resident=resident)
    ld = DeviceTrainLoader(cfg, src, seed=0)

    def one():
        try:
            return ld.next_batch()
        except StopIteration:
            return ld.next_batch()
    ms = block_ms(one, batches, warm=warmup)
    out_bytes = B * (3 * h * w * 4 + (h // g) * (w // g) * 8)
    src_bytes = B * h * w * 4                                      # the crop's footprint: 3 image bytes + 1 label byte per pixel
    upload = 0 if resident else sum(a.nbytes + b.nbytes for a, b in zip(images[:B], labels[:B]))
    row = {"preset": name, "sources": "device" if resident else "host", "batch": B, "down_sampling": d, "crop": [h, w], "g": g,
           "batches": batches, "batch_ms": round(ms, 4), "GB": round((out_bytes + src_bytes + upload) / 1e9, 4),
           "GB_per_s": round((out_bytes + src_bytes + upload) / 1e9 / (ms / 1e3), 1)}
    with C.recording(level=2) as rec:
        for _ in range(10):
            one()
    for kname, (count, kms) in rec.kernels.items():
        if "train_batch" in kname or "resize_u8" in kname:
            b = rec.kernel_bytes.get(kname, 0.0)
            key = "kernel" if "train_batch" in kname else "resize"
            row[key + "_ms"] = round(kms / count, 4)
            row[key + "_GB_per_s"] = round(b / 1e9 / (kms / 1e3), 1) if kms > 0 else None
    del ld, src
    torch.cuda.synchronize()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--presets", default="C4,C3,C5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rs = np.random.RandomState(2024)
    images = [rs.randint(0, 256, size=(1024, 2048, 3)).astype(np.uint8) for _ in range(12)]
    labels = [rs.randint(0, 19, size=(1024, 2048)).astype(np.uint8) for _ in range(12)]
    rows = []
    for name in a.presets.split(","):
        for resident in (True, False):
            row = measure(name, resident, images, labels, a.batches, a.warmup)
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
