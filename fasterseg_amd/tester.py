"""Test-set inference to files (drop-in for the reference's train/test.py SegTester + tools/engine/tester.py).

The reference, per frame, copies the score map to the host, maps train ids to label ids in a Python double loop over every
pixel (test.py:66-68), paints the overlay with np.where passes (visualize.py) and calls cv2.imwrite twice.  Here the class
map never leaves the device until it is a finished picture: one fs_render_prediction launch writes the label-ID map and the
overlay into a staging slot, an asynchronous copy brings the bytes to pinned host memory, and worker threads encode the PNGs
while the next frames run (PredictionWriter).  With device_png=True the single-channel maps are deflated on the device as well
(fs_png_deflate): what crosses to the host is the finished IDAT stream and the workers only wrap it into a file."""
import os
import queue
import threading

import numpy as np
import torch

from . import kernels as K
from .evaluator import SegEvaluator
from .png import png_bytes

MAX_WORKERS = 16


def save_png(path, array, compress_level=1):
    """(H, W) uint8 -> a single-channel ('L') PNG, (H, W, 3) uint8 -> an RGB PNG."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(array)).save(path, format="PNG", compress_level=compress_level)


def _layout(shapes):
    """Byte offsets / pitches of the outputs of one submission inside a slot: every output starts 16 bytes aligned, and so does every
    row of an (H, W, 3) picture (its pitch is rounded up); an (H, W) map is dense, as fs_render_prediction writes it."""
    plan, off = [], 0
    for shape in shapes:
        row = int(shape[1]) * (3 if len(shape) == 3 else 1)
        pitch = K.round_up(row, 16) if len(shape) == 3 else row
        plan.append((off, pitch, row))
        off = K.round_up(off + pitch * int(shape[0]), 16)
    return plan, off


class _Stream:
    """A device-made IDAT stream on its way to a file: the pinned bytes, the pinned length word, the picture's size."""

    def __init__(self, height, width, data, length):
        self.height, self.width, self.data, self.length = height, width, data, length

    def file_bytes(self):
        return png_bytes(self.height, self.width, 1, self.data[:int(self.length[0])])


def write_stream(path, stream):
    with open(path, "wb") as f:
        f.write(stream.file_bytes())


class _Slot:
    """One staging slot: a device buffer the kernels render into, a pinned host buffer of the same size the finished bytes are
    copied to, and the event behind that copy.  With device=None both are one numpy array (host-side producers).  With device_png
    a second pair of buffers holds, per (H, W) output, a 16-byte length word and the compressed stream (fs_png_deflate_bound bytes),
    and one device workspace serves the outputs in turn (their launches are ordered on the stream)."""

    def __init__(self, device, device_png=False):
        self.device = device
        self.device_png = bool(device_png)
        self.dev = self.host = self.event = None
        self.size = 0
        self.zdev = self.zhost = self.zws = None
        self.zsize = self.zneed = 0
        self.raw = []                  # byte ranges of dev that publish copies

    def views(self, shapes):
        plan, need = _layout(shapes)
        if need > self.size:
            if self.device is None:
                self.dev = self.host = np.empty(need, dtype=np.uint8)
            else:
                self.dev = torch.empty(need, dtype=torch.uint8, device=self.device)
                self.host = torch.empty(need, dtype=torch.uint8, pin_memory=True)
                self.event = torch.cuda.Event()
            self.size = need
        self.need = need
        self.raw = [(0, need)]
        host = self.host if self.device is None else self.host.numpy()
        dev, hst = [], []
        for shape, (off, pitch, row) in zip(shapes, plan):
            H = int(shape[0])
            d = self.dev[off:off + H * pitch].reshape(H, pitch)[:, :row]
            h = host[off:off + H * pitch].reshape(H, pitch)[:, :row]
            if len(shape) == 3:
                d = d.reshape(H, row // 3, 3) if self.device is None else d.unflatten(1, (row // 3, 3))
                h = h.reshape(H, row // 3, 3)
            dev.append(d)
            hst.append(h)
        return dev, hst

    def deflate(self, shapes, dev, host):
        """device_png: compress every (H, W) view of `dev` into this slot's compressed area.  Returns `host` with those outputs replaced
        by their _Stream; publish then copies the streams (the whole bound: at most 9/8 of the raw map) and the raw bytes of the
        (H, W, 3) outputs only."""
        plan, _ = _layout(shapes)
        sizes = [K.png_deflate_sizes(int(sh[0]), int(sh[1]), K.png_rows_per_band(int(sh[0]), int(sh[1]))) if len(sh) == 2 else None for sh in shapes]
        need = sum(16 + K.round_up(sz[0], 16) for sz in sizes if sz)
        if need > self.zsize:
            self.zdev = torch.empty(need, dtype=torch.uint8, device=self.device)
            self.zhost = torch.empty(need, dtype=torch.uint8, pin_memory=True)
            self.zsize = need
        ws = max([sz[1] for sz in sizes if sz] + [0])
        if self.zws is None or ws > self.zws.numel():
            self.zws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self.zneed, self.raw = need, []
        zhost = self.zhost.numpy()
        out, at = [], 0
        for shape, sz, view, h, (off, pitch, _) in zip(shapes, sizes, dev, host, plan):
            if sz is None:
                self.raw.append((off, off + int(shape[0]) * pitch))
                out.append(h)
                continue
            K.png_deflate(view, out=self.zdev[at + 16:at + 16 + sz[0]], workspace=self.zws, out_bytes=self.zdev[at:at + 8].view(torch.int64))
            out.append(_Stream(int(shape[0]), int(shape[1]), zhost[at + 16:at + 16 + sz[0]], zhost[at:at + 8].view(np.int64)))
            at += 16 + K.round_up(sz[0], 16)
        return out

    def publish(self):
        """Queue the device -> pinned copy of what was rendered behind the kernels of the current stream."""
        if self.device is not None:
            for a, b in self.raw:
                self.host[a:b].copy_(self.dev[a:b], non_blocking=True)
            if self.zneed:
                self.zhost[:self.zneed].copy_(self.zdev[:self.zneed], non_blocking=True)
            self.event.record()

    def wait(self):
        if self.event is not None:
            self.event.synchronize()


class PredictionWriter:
    """PNG files written behind the device.  submit(outputs, render) takes a free slot (blocks while every slot is in flight), lets
    `render` fill the slot's device views, queues the copy to pinned memory on the current stream and returns; a worker thread
    waits for the copy, encodes the files (zlib releases the GIL) and only then frees the slot.  close() joins the workers and
    re-raises the first exception one of them met.  Threads only; `workers` is capped at 16 whatever the host has.

    device_png=True: after `render` every (H, W) output is deflated on the device (fs_png_deflate) into a compressed area of the slot;
    that area and its length word are copied to pinned memory instead of the raw map, and the worker writes png_bytes(...) of the first
    out_bytes bytes - no worker deflates an (H, W) map, and `encode` is not called for one.  The files decode to the same pixels; they
    are larger than zlib's (run-length matches and the fixed Huffman code only).  (H, W, 3) outputs - the photo-like overlays - keep
    the host encoder on purpose: distance-1 runs buy nothing on them and the file would be 9/8 of the raw picture."""

    def __init__(self, slots=4, workers=4, device="cuda", encode=None, compress_level=1, device_png=False):
        if slots < 1 or workers < 1:
            raise ValueError("PredictionWriter: at least one slot and one worker")
        if device_png and device is None:
            raise ValueError("PredictionWriter: device_png needs a device (device=None stages host arrays)")
        self.device_png = bool(device_png)
        self.encode = encode if encode is not None else (lambda path, array: save_png(path, array, compress_level))
        self._free = queue.Queue()
        for _ in range(slots):
            self._free.put(_Slot(None if device is None else torch.device(device), self.device_png))
        self._jobs = queue.Queue()
        self._error = None
        self._lock = threading.Lock()
        self._threads = [threading.Thread(target=self._work, name="fs-png-%d" % i, daemon=True) for i in range(min(int(workers), MAX_WORKERS))]
        for t in self._threads:
            t.start()

    def submit(self, outputs, render):
        """outputs: [(path, shape)], shape (H, W) or (H, W, 3); render(views) fills the uint8 views (one per output, rows 16 bytes
        aligned) - device tensors, or numpy arrays for a writer built with device=None."""
        if not self._threads:
            raise RuntimeError("PredictionWriter is closed")
        slot = self._free.get()
        try:
            shapes = [shape for _, shape in outputs]
            dev, host = slot.views(shapes)
            render(dev)
            if self.device_png:
                host = slot.deflate(shapes, dev, host)
            slot.publish()
        except BaseException:
            self._free.put(slot)
            raise
        self._jobs.put((slot, [(path, h) for (path, _), h in zip(outputs, host)]))

    def _work(self):
        while True:
            job = self._jobs.get()
            if job is None:
                self._jobs.task_done()
                return
            slot, files = job
            try:
                slot.wait()
                for path, array in files:
                    if isinstance(array, _Stream):
                        write_stream(path, array)
                    else:
                        self.encode(path, array)
            except BaseException as e:          # kept for close(): a worker must not die with a slot in its hands
                with self._lock:
                    if self._error is None:
                        self._error = e
            finally:
                self._free.put(slot)             # the files of this slot are closed: it may be rendered into again
                self._jobs.task_done()

    def flush(self):
        """Block until every submitted file is written; re-raise the first worker exception."""
        self._jobs.join()
        self._raise()

    def _raise(self):
        with self._lock:
            e, self._error = self._error, None
        if e is not None:
            raise e

    def close(self):
        threads, self._threads = self._threads, []
        for _ in threads:
            self._jobs.put(None)
        for t in threads:
            t.join()
        self._raise()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class SegTester(SegEvaluator):
    """train/test.py SegTester: per frame `<fn>.png`, the prediction as a single-channel PNG of label ids, and with show_prediction
    `<fn>.viz.png`, the image painted by the prediction (RGB), under save_dir.  labels: a visualize.LabelSpec.  evaluator_kwargs go
    to SegEvaluator (image_shape, dtype, multi_scales, is_flip, crop_size, stride_rate, uint8_input); slots / workers size the writer;
    write=False renders every frame but writes no file (timing); device_png=True deflates `<fn>.png` on the device (PredictionWriter)."""

    def __init__(self, network, class_num, image_mean, image_std, labels, save_dir, show_prediction=False, slots=4, workers=4,
                 write=True, device_png=False, **evaluator_kwargs):
        super().__init__(network, class_num, image_mean, image_std, **evaluator_kwargs)
        self.labels = labels
        self.save_dir = save_dir
        self.show_prediction = bool(show_prediction)
        self.labeled_frames = 0
        self.writer = None
        self._scratch = _Slot(self.device)
        if write:
            os.makedirs(save_dir, exist_ok=True)
            self.writer = PredictionWriter(slots=slots, workers=workers, device=self.device, device_png=device_png)

    def _render(self, img, pred, views):
        palette, lut = self.labels.tables(self.device)
        if self.show_prediction:
            K.render_prediction(img, [pred], palette, views[1], gap=0, background=self.labels.background, show255=[False], weights=[1],
                                lut=lut, ids=views[0])
        else:
            K.render_prediction(None, [pred], None, lut=lut, ids=views[0])

    def func_per_iteration(self, data):
        """data: {'data': HWC uint8 image, 'label': (H, W) labels or None, 'fn': name}.  Dispatch of test.py:55-58; the files are
        queued, the class map is returned; frames with a label are accumulated for compute_metric."""
        if len(self.multi_scales) == 1:
            pred = self.whole_eval(data['data'])
        else:
            pred = self.sliding_eval(data['data'], self.crop_size, self.stride_rate)
        H, W = int(pred.shape[0]), int(pred.shape[1])
        img = None
        outputs = [(os.path.join(self.save_dir, data['fn'] + ".png"), (H, W))]
        if self.show_prediction:
            img = torch.as_tensor(data['data']).to(self.device).contiguous()
            outputs.append((os.path.join(self.save_dir, data['fn'] + ".viz.png"), (H, W, 3)))
        if self.writer is not None:
            self.writer.submit(outputs, lambda views: self._render(img, pred, views))
        else:
            self._render(img, pred, self._scratch.views([shape for _, shape in outputs])[0])
        label = data.get('label')
        if label is not None:
            self.acc.add(pred, torch.as_tensor(label).to(self.device).contiguous())
            self.labeled_frames += 1
        return pred

    def run_online(self, dataset):
        """Every frame of an iterable of such dicts; returns when the last file is on disk.  The metric (compute_metric) when the
        frames carried labels, else None."""
        for data in dataset:
            self.func_per_iteration(data)
        if self.writer is not None:
            self.writer.flush()
        else:
            torch.cuda.synchronize(self.device)
        return self.compute_metric() if self.labeled_frames else None

    def close(self):
        if self.writer is not None:
            writer, self.writer = self.writer, None
            writer.close()


class PseudoLabeler(SegEvaluator):
    """Pseudo-labels for unlabelled frames from a trained network (the teacher, before the student's distillation run): per frame
    `<fn>.png` under save_dir, the single-channel train-id map with `ignore_label` wherever the winning class's confidence is below
    `min_confidence` - the label format dataloader.py reads - and with save_confidence `<fn>.conf.png`, the confidence byte
    floor(255 conf + 0.5).  Both maps come from SegEvaluator.predict (one launch in the single-scale mode) and go through the
    PredictionWriter; evaluator_kwargs go to SegEvaluator.  The kept pixels are counted per class on the device (fs_hist_info of the map
    against itself: the masked pixels carry ignore_label >= class_num and are skipped) and read back once, by run_online.
    write=False labels every frame but writes no file; device_png=True deflates both maps on the device (PredictionWriter)."""

    def __init__(self, network, class_num, image_mean, image_std, save_dir, min_confidence=0.9, ignore_label=255, save_confidence=False,
                 slots=4, workers=4, write=True, device_png=False, **evaluator_kwargs):
        self.min_conf = K.confidence_threshold(min_confidence)
        if K._check_ignore_label(ignore_label) < class_num:
            raise ValueError("ignore_label %d is one of the %d classes" % (ignore_label, class_num))
        super().__init__(network, class_num, image_mean, image_std, **evaluator_kwargs)
        self.min_confidence = min_confidence
        self.ignore_label = int(ignore_label)
        self.save_dir = save_dir
        self.save_confidence = bool(save_confidence)
        self.frames = 0
        self.pixels = 0
        self.writer = None
        if write:
            os.makedirs(save_dir, exist_ok=True)
            self.writer = PredictionWriter(slots=slots, workers=workers, device=self.device, device_png=device_png)

    def func_per_iteration(self, data):
        """data: {'data': HWC uint8 image, 'fn': name}.  Queues the files, counts the kept pixels, returns (classes, confidence)."""
        classes, conf = self.predict(data['data'], self.min_confidence, self.ignore_label)
        classes = classes.contiguous()
        H, W = int(classes.shape[0]), int(classes.shape[1])
        if self.writer is not None:
            outputs = [(os.path.join(self.save_dir, data['fn'] + ".png"), (H, W))]
            if self.save_confidence:
                outputs.append((os.path.join(self.save_dir, data['fn'] + ".conf.png"), (H, W)))

            def render(views):
                views[0].copy_(classes)
                if self.save_confidence:
                    views[1].copy_(conf)
            self.writer.submit(outputs, render)
        self.acc.add(classes, classes)
        self.frames += 1
        self.pixels += H * W
        return classes, conf

    def run_online(self, dataset):
        """Every frame of an iterable of such dicts; returns when the last file is on disk: {"frames", "kept": the fraction of the
        pixels that kept their class, "per_class": kept pixels per class (int64 array)} - one device-to-host read."""
        for data in dataset:
            self.func_per_iteration(data)
        if self.writer is not None:
            self.writer.flush()
        hist, labeled, _ = self.acc.result()
        return {"frames": self.frames, "kept": labeled / self.pixels if self.pixels else 0.0, "per_class": np.diag(hist).copy()}

    def close(self):
        if self.writer is not None:
            writer, self.writer = self.writer, None
            writer.close()
