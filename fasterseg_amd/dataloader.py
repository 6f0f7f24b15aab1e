"""Training batches built on the device: the reference's input pipeline (search|train/dataloader.py TrainPre / get_train_loader,
tools/datasets/BaseDataset.py) without cv2 and without host-side pixels.

Sources keep decoded uint8 images (HWC RGB) and labels (HW) resident on the GPU, down-sampled once at load by fs_resize_u8
(BaseDataset._open_image).  Each batch is one fs_train_batch launch (csrc/train_input.hip): mirror, random scale, normalisation, crop /
pad and the label down-sample of TrainPre, bit-exact to the reference's arithmetic (train_plan.py builds the draws and tables).  The
per-batch upload is B sample descriptors plus source pointers from a pinned staging ring; nothing in a batch waits for the device."""
import os
import random

import numpy as np
import torch

from . import _lib, kernels, train_plan

_RING = 4                   # staging slots: a slot is rewritten only after the upload issued from it RING batches ago has completed


class _Batcher:
    """fs_train_batch plumbing of one (crop, g, mean, std): the table store mirrored on the device, the normalisation table and the
    pinned staging ring."""

    def __init__(self, crop_h, crop_w, g, mean, std, device):
        self.crop_h, self.crop_w, self.g = int(crop_h), int(crop_w), int(g)
        if self.crop_w % 4 or self.crop_h % self.g or self.crop_w % self.g:
            raise ValueError("crop %dx%d with gt_down_sampling %d: the width must be a multiple of 4 and g must divide the crop"
                             % (self.crop_h, self.crop_w, self.g))
        self.device = torch.device(device)
        self.store = train_plan.TableStore()
        self.gy, self.gx = self.store.label_tables(self.crop_h, self.crop_w, self.g)
        self.tables = torch.empty(0, dtype=torch.int32, device=self.device)
        self.on_device = 0
        self._keep = []                                   # pinned sources of table uploads (alive until their copies have run)
        self.norm = torch.from_numpy(train_plan.norm_table(mean, std)).to(self.device)
        self.slot_bytes = 0
        self.ring = []
        self.next = 0

    def _sync_tables(self):
        n = self.store.n
        if n == self.on_device:
            return
        if n > self.tables.numel():
            grown = torch.empty(max(2 * self.tables.numel(), n, 4096), dtype=torch.int32, device=self.device)
            grown[:self.on_device].copy_(self.tables[:self.on_device])
            self.tables = grown
        new = torch.from_numpy(self.store.array()[self.on_device:n].copy()).pin_memory()
        self.tables[self.on_device:n].copy_(new, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._keep = [(e, t) for e, t in self._keep if not e.query()] + [(ev, new)]
        self.on_device = n

    def _slot(self, B):
        need = int(_lib.lib().fs_train_batch_args_bytes(B))
        if need > self.slot_bytes:
            for ev, _, _ in self.ring:
                ev.synchronize()                          # only when the batch size grows: old pinned slots may still be read
            self.slot_bytes = max(need, 1024)
            self.ring = [(torch.cuda.Event(), torch.empty(self.slot_bytes, dtype=torch.uint8).pin_memory(),
                          torch.empty(self.slot_bytes, dtype=torch.uint8, device=self.device)) for _ in range(_RING)]
            self.next = 0
        slot = self.ring[self.next]
        self.next = (self.next + 1) % _RING
        slot[0].synchronize()                             # the upload from this slot RING batches ago (long done in steady state)
        return slot

    def run(self, draws, images, labels, out=None):
        """draws: [train_plan.SampleDraw], images / labels: the matching device sources -> (imgs (B, 3, H, W) fp32,
        target (B, H / g, W / g) int64), fresh from the allocator or written into out = (imgs, target)."""
        B = len(draws)
        rows = np.stack([train_plan.sample_row(d, self.store.scale_tables(d.H, d.W, d.sh, d.sw)) for d in draws])
        self._sync_tables()
        if out is None:
            imgs = torch.empty((B, 3, self.crop_h, self.crop_w), dtype=torch.float32, device=self.device)
            target = torch.empty((B, self.crop_h // self.g, self.crop_w // self.g), dtype=torch.int64, device=self.device)
        else:
            imgs, target = out
        ev, staging, args = self._slot(B)
        bd = _lib.TrainBatchDesc(B, self.crop_h, self.crop_w, self.g, self.gy, self.gx, self.on_device)
        kernels.train_batch(bd, rows, images, labels, self.tables, self.norm, staging, args, imgs, target)
        ev.record()
        return imgs, target


def _as_device_u8(a, device, channels):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype != torch.uint8 or t.dim() != (3 if channels else 2) or (channels and t.shape[2] != 3):
        raise ValueError("expected a uint8 %s array, got %s %s" % ("(H, W, 3)" if channels else "(H, W)", tuple(t.shape), t.dtype))
    return t.to(device, non_blocking=True).contiguous()


class TrainPre:
    """Drop-in for search|train/dataloader.py TrainPre: (img, gt) -> (p_img, p_gt, None) on the device.

    img: uint8 (H, W, 3) RGB (the reference's image after `img[:, :, ::-1]`), gt: uint8 (H, W) label, numpy or CUDA tensors.
    p_img: fp32 (3, image_height, image_width), p_gt: int64 (image_height // g, image_width // g).  The draws come from the global
    `random` module in the reference's order, so the same random.seed gives the same mirror, scale and crop as the reference."""

    def __init__(self, config, img_mean, img_std, device="cuda"):
        self.config = config
        self.device = torch.device(device)
        self._batcher = _Batcher(config.image_height, config.image_width, config.gt_down_sampling, img_mean, img_std, self.device)

    def __call__(self, img, gt, rng=random):
        img = _as_device_u8(img, self.device, True)
        gt = _as_device_u8(gt, self.device, False)
        if tuple(img.shape[:2]) != tuple(gt.shape):
            raise ValueError("image %s and label %s sizes differ" % (tuple(img.shape), tuple(gt.shape)))
        c = self.config
        d = train_plan.draw_sample(rng, img.shape[0], img.shape[1], c.image_height, c.image_width, c.train_scale_array)
        imgs, target = self._batcher.run([d], [img], [gt])
        return imgs[0], target[0], None


_load_tables = {}


def _down_sample(img, lbl, down_sampling):
    """BaseDataset._open_image's resize of one (image, label) pair on the device (fs_resize_u8); tables cached per source size."""
    H, W = lbl.shape
    dev = img.device
    key = (str(dev), H, W, repr(down_sampling))
    if key not in _load_tables:
        plan = train_plan.load_tables(H, W, down_sampling)
        if plan is not None:
            (h, w), lin, nn = plan
            plan = (h, w), [torch.from_numpy(a).to(dev) for a in lin + nn]
        _load_tables[key] = plan
    plan = _load_tables[key]
    if plan is None:
        return img, lbl
    (h, w), (ylin, xlin, ynn, xnn) = plan
    oimg = kernels.resize_u8(img, torch.empty((h, w, 3), dtype=torch.uint8, device=dev), ylin, xlin, nearest=False)
    olbl = kernels.resize_u8(lbl, torch.empty((h, w), dtype=torch.uint8, device=dev), ynn, xnn, nearest=True)
    return oimg, olbl


class ArraySource:
    """Decoded uint8 samples: images (H, W, 3) RGB and labels (H, W), numpy arrays or tensors.  resident=True (default): each entry
    is uploaded once, down-sampled on the device by fs_resize_u8 (down_sampling as the reference's config: an int d or an (h, w)
    pair) and kept in device memory.  resident=False: pinned host copies, uploaded (and down-sampled) each time a batch uses them."""

    def __init__(self, images, labels, down_sampling=1, device="cuda", resident=True):
        if len(images) != len(labels) or not len(images):
            raise ValueError("%d images and %d labels" % (len(images), len(labels)))
        self.device = torch.device(device)
        self.down_sampling = down_sampling
        self.resident = bool(resident)
        self._items = []
        self._sizes = []
        for img, lbl in zip(images, labels):
            if self.resident:
                img, lbl = _down_sample(_as_device_u8(img, self.device, True), _as_device_u8(lbl, self.device, False), down_sampling)
                self._sizes.append(tuple(lbl.shape))
            else:
                img, lbl = _as_device_u8(img, "cpu", True).pin_memory(), _as_device_u8(lbl, "cpu", False).pin_memory()
                self._sizes.append(train_plan.load_size(lbl.shape[0], lbl.shape[1], down_sampling))
            if tuple(img.shape[:2]) != tuple(lbl.shape):
                raise ValueError("image %s and label %s sizes differ" % (tuple(img.shape), tuple(lbl.shape)))
            self._items.append((img, lbl))

    def __len__(self):
        return len(self._items)

    def size(self, i):
        """(H, W) of sample i after down-sampling."""
        return self._sizes[i]

    def get(self, i):
        """(image, label) of sample i on the device."""
        img, lbl = self._items[i]
        if self.resident:
            return img, lbl
        return _down_sample(img.to(self.device, non_blocking=True), lbl.to(self.device, non_blocking=True), self.down_sampling)


class FileListSource(ArraySource):
    """The reference's file list (`img gt` per line, relative to img_root / gt_root; `portion` as BaseDataset._get_file_names),
    decoded with PIL (images as RGB, labels as 8-bit `L`) once at construction, then an ArraySource."""

    def __init__(self, img_root, gt_root, source, down_sampling=1, portion=None, device="cuda", resident=True):
        from PIL import Image
        self.names = train_plan.read_file_list(source, portion)
        if not self.names:
            raise ValueError("no samples in %s (portion %r)" % (source, portion))
        images, labels = [], []
        for img_name, gt_name in self.names:
            with Image.open(os.path.join(img_root, img_name)) as im:
                images.append(np.array(im.convert("RGB"), dtype=np.uint8))
            with Image.open(os.path.join(gt_root, gt_name)) as im:
                labels.append(np.array(im.convert("L"), dtype=np.uint8))
        super().__init__(images, labels, down_sampling, device, resident)


class DeviceTrainLoader:
    """Iterates batches {'data': (B, 3, image_height, image_width) fp32, 'label': (B, image_height // g, image_width // g) int64} on
    the device, the keys the reference's train loops read; B = config.batch_size.

    An epoch has world * batch_size * niters_per_epoch draws (every sample equally often, the remainder a random subset: the
    reference's BaseDataset._construct_new_file_names), in an order drawn from np.random.default_rng((seed, epoch)); rank r of world
    takes every world-th of them (train_plan.rank_share) and yields niters_per_epoch batches.  Without niters_per_epoch an epoch is
    one pass over the source and drop_last decides the short last batch.  The augmentation draws come from
    random.Random(seed * 65537 + rank) in TrainPre's order: given the seed, every batch is reproducible bit for bit.  The sample
    ORDER cannot match the reference's: there it depends on the DataLoader's shuffle and worker processes.

    next_batch(out=(imgs, target)) writes a batch into the caller's buffers (e.g. SupernetStep.static) instead of fresh ones."""

    def __init__(self, config, source, seed=0, rank=0, world=1, drop_last=True, device="cuda"):
        if not 0 <= rank < world:
            raise ValueError("rank %d of world %d" % (rank, world))
        self.config = config
        self.source = source
        self.seed, self.rank, self.world, self.drop_last = int(seed), int(rank), int(world), bool(drop_last)
        self.batch_size = int(config.batch_size)
        self.niters = getattr(config, "niters_per_epoch", None)
        self.rng = random.Random(self.seed * 65537 + self.rank)
        self.epoch = 0
        self._batcher = _Batcher(config.image_height, config.image_width, config.gt_down_sampling, config.image_mean,
                                 config.image_std, device)
        self._order = None
        self._pos = 0

    def epoch_share(self, epoch):
        """The sample indices rank `rank` draws in `epoch`."""
        n = len(self.source)
        length = n if self.niters is None else self.world * self.batch_size * int(self.niters)
        return train_plan.rank_share(train_plan.epoch_indices(n, length, self.seed, epoch), self.rank, self.world)

    def __len__(self):
        if self.niters is not None:
            return int(self.niters)
        share = len(self.epoch_share(0))
        return share // self.batch_size if self.drop_last else -(-share // self.batch_size)

    def _start_epoch(self):
        self._order = self.epoch_share(self.epoch)
        self._pos = 0

    def next_batch(self, out=None):
        """The next batch of the current epoch; StopIteration at its end (the next call starts the next epoch)."""
        if self._order is None:
            self._start_epoch()
        remaining = len(self._order) - self._pos
        if remaining <= 0 or (self.drop_last and remaining < self.batch_size) or (self.niters is not None and
                                                                                   self._pos >= int(self.niters) * self.batch_size):
            self.epoch += 1
            self._order = None
            raise StopIteration
        idx = self._order[self._pos:self._pos + self.batch_size]
        self._pos += len(idx)
        c = self.config
        draws, images, labels = [], [], []
        for i in idx:
            H, W = self.source.size(int(i))
            draws.append(train_plan.draw_sample(self.rng, H, W, c.image_height, c.image_width, c.train_scale_array))
            img, lbl = self.source.get(int(i))
            images.append(img)
            labels.append(lbl)
        imgs, target = self._batcher.run(draws, images, labels, out=out)
        return {"data": imgs, "label": target}

    def __iter__(self):
        while True:
            try:
                yield self.next_batch()
            except StopIteration:
                return


def get_train_loader(config, source=None, portion=None, seed=0, rank=0, world=1, device="cuda"):
    """search|train/dataloader.py get_train_loader on the device.  source None: a FileListSource of the config's img_root_folder,
    gt_root_folder, train_source and down_sampling, cut by `portion`; otherwise a ready source (ArraySource / FileListSource)."""
    if source is None:
        source = FileListSource(config.img_root_folder, config.gt_root_folder, config.train_source, config.down_sampling, portion,
                                device=device)
    elif portion is not None:
        raise ValueError("portion applies to the config's file list; cut a ready source before passing it")
    return DeviceTrainLoader(config, source, seed=seed, rank=rank, world=world, device=device)
