"""Validation path with the per-pixel work on the device (drop-in for tools/engine/evaluator.py Evaluator + train/eval.py SegEvaluator).

Reference, per validation image (evaluator.py:205-225, 297-318; eval.py:17-28): normalise on the host, forward, exp() of the
(19, 1024, 2048) fp32 score map, copy 159 MB to the host, np.argmax, hist_info on the host.  Here: the image is normalised on
the device, the network runs from the static-plan engine in class-map mode (the final x8 up-sample and the arg-max are one
launch writing a 2 MB uint8 map), and the confusion histogram is accumulated on the device; the host reads 19 x 19 counts at
the end of the run.

Multi-scale, sliding-window and flip evaluation (evaluator.py:206-295; the eval_scale_array / eval_flip / eval_crop_size /
eval_stride_rate config fields) run on the device too: per window, fs_eval_window_input builds the network input straight from
the uint8 image (cv2's fixed-point bilinear resize, padding, normalisation, the mirrored copy), the engine runs in "lowres" mode,
fs_eval_score_accumulate adds exp(l + unflip(l_flip)) of the x8 up-sampled logits into a per-scale canvas, and
fs_eval_rescale_accumulate resizes each scale's canvas back to the image (cv2 INTER_LINEAR on float) into the total, taking the
arg-max on the last scale.  The host only plans (fasterseg_amd.eval_plan) and issues launches."""
import os

import numpy as np
import torch

from . import engine
from . import eval_plan as EP
from . import kernels as K
from .metric import HistAccumulator, compute_score


class _ImageState:
    """Device buffers of one image shape, allocated on its first frame and reused: the uploaded image, the fp32 HWC total and
    the class map, one flat fp32 canvas (grown to the largest canvas a plan needs), the per-scale plans with their tap tables."""

    def __init__(self, H, W, cs, device):
        self.img = torch.empty((H, W, 3), dtype=torch.uint8, device=device)
        self.total = torch.empty((H, W, cs), dtype=torch.float32, device=device)
        self.classes = torch.empty((H, W), dtype=torch.uint8, device=device)
        self.conf = torch.empty((H, W), dtype=torch.uint8, device=device)       # predict(): the confidence byte beside the class map
        self.canvas = torch.empty(0, dtype=torch.float32, device=device)
        self.plans = {}
        self.outputs = {}


class SegEvaluator:
    def __init__(self, network, class_num, image_mean, image_std, image_shape=(1024, 2048), dtype=torch.bfloat16, device="cuda",
                 multi_scales=(1,), is_flip=False, crop_size=None, stride_rate=5 / 6, save_path=None, show_image=False,
                 show_prediction=False, labels=None, uint8_input=False):
        self.class_num = class_num
        self.device = torch.device(device)
        self.image_mean = torch.tensor(np.asarray(image_mean, dtype=np.float32), device=self.device).view(1, 3, 1, 1)
        self.image_std = torch.tensor(np.asarray(image_std, dtype=np.float32), device=self.device).view(1, 3, 1, 1)
        self._mean = [float(v) for v in np.asarray(image_mean, dtype=np.float32)]
        self._std = [float(v) for v in np.asarray(image_std, dtype=np.float32)]
        H, W = image_shape
        self.image_shape = (H, W)
        self.dtype = dtype
        self.multi_scales = list(multi_scales)
        self.is_flip = bool(is_flip)
        self.crop_size = crop_size
        self.stride_rate = stride_rate
        assert len(self.multi_scales) >= 1
        assert len(self.multi_scales) == 1 or crop_size is not None, "multi-scale evaluation slides a crop_size window (eval_crop_size)"
        self.val_func = network.eval()
        # the whole-image class-map engine of today's single-scale, no-flip path; built up front when that is the configured path
        # uint8_input: that path hands the uint8 HWC frame to an engine whose stem normalises it (InferenceEngine(input="uint8")) - no
        # process_image, no fp32 image; the flip, padded and multi-scale paths resample and keep fs_eval_window_input
        self.uint8_input = bool(uint8_input)
        self._u8_engines = {}                       # (H, W) -> uint8 "classes" engine
        self._conf_engines = {}                     # predict(): (H, W, uint8 input, min_conf byte, ignore_label) -> "classes+confidence" engine
        self.engine = None
        if len(self.multi_scales) == 1 and not self.is_flip:
            self.engine = self._u8_engine(H, W) if self.uint8_input else \
                engine.InferenceEngine(self.val_func, (1, 3, H, W), dtype=dtype, output="classes")
        self.acc = HistAccumulator(class_num, self.device)
        self.cs = K.round_up(class_num, 4)          # fp32 canvas / total channel stride (19 -> 20)
        self._lowres = {}                           # input shape -> "lowres" engine
        self._states = {}                           # (H, W) -> _ImageState
        # train/eval.py:30-51, off by default: files per frame (data['fn']) through a tester.PredictionWriter created on first use
        self.save_path = save_path
        self.show_image = bool(show_image)
        self.show_prediction = bool(show_prediction)
        self.labels = labels                        # visualize.LabelSpec: the colours of the pictures
        self._writer = None

    def load_weights(self, network=None):
        """The weights changed (train/train.py:196-208: the model being trained is validated after the first and every tenth
        epoch, search/train_search.py:141-183 after every epoch): every engine this evaluator has built - the class-map engine
        and the "lowres" engine of each window shape - re-derives its packs and folded BatchNorms with one launch each
        (InferenceEngine.load_weights) instead of being rebuilt and re-tuned.  network=None: the module given at construction
        was updated in place; a module: it replaces val_func (same architecture, else ValueError and nothing is written).  The
        histogram accumulators and the writer are left alone."""
        if network is not None:
            network = network.eval()
        engines = ([self.engine] if self.engine is not None else []) + list(self._lowres.values())
        engines += [e for e in self._u8_engines.values() if e is not self.engine]
        engines += list(self._conf_engines.values())
        for eng in engines:
            eng.load_weights(network)
        if network is not None:
            self.val_func = network

    def process_image(self, img):
        """HWC uint8 (numpy or tensor, RGB like the reference after its BGR->RGB flip) -> normalised (1, 3, H, W) fp32 on the
        device: tools/utils/img_utils.py:178-184 normalize + the transpose of evaluator.py:346."""
        t = torch.as_tensor(img)
        t = t.to(self.device, non_blocking=True).permute(2, 0, 1).unsqueeze(0).float()
        return (t / 255.0 - self.image_mean) / self.image_std

    def val_func_process(self, input_data):
        """(1, 3, H, W) normalised image -> (H, W) uint8 class map on the device (argmax(exp(score)) = argmax(score))."""
        if self.engine is None:
            self.engine = engine.InferenceEngine(self.val_func, (1, 3) + tuple(input_data.shape[2:]), dtype=self.dtype, output="classes")
        return self.engine(input_data)[0]

    def _u8_engine(self, H, W):
        eng = self._u8_engines.get((H, W))
        if eng is None:
            eng = self._u8_engines[(H, W)] = engine.InferenceEngine(self.val_func, (1, 3, H, W), dtype=self.dtype, output="classes",
                                                                    input="uint8", image_mean=self._mean, image_std=self._std)
        return eng

    def _conf_engine(self, H, W, min_confidence, ignore_label):
        key = (H, W, self.uint8_input, K.confidence_threshold(min_confidence), K._check_ignore_label(ignore_label))
        eng = self._conf_engines.get(key)
        if eng is None:
            kw = dict(input="uint8", image_mean=self._mean, image_std=self._std) if self.uint8_input else {}
            eng = self._conf_engines[key] = engine.InferenceEngine(self.val_func, (1, 3, H, W), dtype=self.dtype, output="classes+confidence",
                                                                   min_confidence=min_confidence, ignore_label=ignore_label, **kw)
        return eng

    # ---- device buffers and engines of the multi-scale / flip paths ------------------------------------------------------
    def _lowres_engine(self, shape):
        eng = self._lowres.get(shape)
        if eng is None:
            eng = self._lowres[shape] = engine.InferenceEngine(self.val_func, shape, dtype=self.dtype, output="lowres")
        return eng

    def _upload(self, img):
        """The image as a contiguous uint8 (H, W, 3) device tensor (copied into the shape's buffer unless it already is one)."""
        t = torch.as_tensor(img)
        assert t.dim() == 3 and t.shape[2] == 3 and t.dtype == torch.uint8, "expected an HWC uint8 RGB image"
        H, W = int(t.shape[0]), int(t.shape[1])
        st = self._states.get((H, W))
        if st is None:
            st = self._states[(H, W)] = _ImageState(H, W, self.cs, self.device)
        if t.is_cuda and t.is_contiguous():
            return t, st
        st.img.copy_(t)
        return st.img, st

    def _canvas(self, st, rows, cols):
        n = rows * cols * self.cs
        if st.canvas.numel() < n:
            st.canvas = torch.empty(n, dtype=torch.float32, device=self.device)
        return st.canvas[:n].view(rows, cols, self.cs)

    def _plan(self, st, H, W, crop, stride_rate):
        key = (tuple(self.multi_scales), int(crop), float(stride_rate))
        plans = st.plans.get(key)
        if plans is None:
            plans = EP.scale_plan(H, W, self.multi_scales, crop, stride_rate)
            for p in plans:
                p.ytab = torch.from_numpy(EP.pack_taps(p.y_index, p.y_coef)).to(self.device)
                p.xtab = torch.from_numpy(EP.pack_taps(p.x_index, p.x_coef)).to(self.device)
                p.descs = [K.eval_window_desc(H, W, p.rows, p.cols, p.top, p.left, oy, ox, crop, crop, p.pad_mode, self.is_flip,
                                              self._mean, self._std) for oy, ox in p.windows]
                self._canvas(st, p.canvas_h, p.canvas_w)          # grow the canvas now, not in the frame loop
            st.plans[key] = plans
        return plans

    def _identity_taps(self, st, H, W):
        taps = st.plans.get("identity")
        if taps is None:
            taps = st.plans["identity"] = tuple(torch.from_numpy(EP.pack_taps(*EP.linear_taps(n, n, 1.0))).to(self.device) for n in (H, W))
        return taps

    # ---- evaluation modes ------------------------------------------------------------------------------------------------
    def whole_eval(self, img, output_size=None, input_size=None):
        """evaluator.py:206-225: the whole image in one pass (plus its mirror with is_flip).  input_size: the normalised image
        is padded with 0 to it (margins as pad_image_to_shape) and the score cropped back; output_size: the exp-score is
        resized to it (cv2 INTER_LINEAR) before the arg-max.  Returns the uint8 class map on the device."""
        if output_size is None and input_size is None and not self.is_flip:
            if self.uint8_input:
                img, _ = self._upload(img)
                self.engine = self._u8_engine(int(img.shape[0]), int(img.shape[1]))
                return self.engine(img)[0]
            return self.val_func_process(self.process_image(img))
        img, st = self._upload(img)
        H, W = int(img.shape[0]), int(img.shape[1])
        ih, iw = EP.two_d(input_size) if input_size is not None else (H, W)
        top, bottom, left, right = EP.pad_margins(H, W, ih, iw)
        PH, PW = H + top + bottom, W + left + right
        flip = self.is_flip
        eng = self._lowres_engine((2 if flip else 1, 3, PH, PW))
        ytab, xtab = self._identity_taps(st, H, W)
        d = K.eval_window_desc(H, W, H, W, top, left, 0, 0, PH, PW, EP.PAD_NORMALISED, flip, self._mean, self._std)
        K.eval_window_input(d, img, ytab, xtab, eng.input)
        logits = eng.run()
        rect = (top, left, H, W)
        if output_size is None:
            return K.eval_score_accumulate(logits, (PH, PW), flip, rect, classes=st.classes)
        OH, OW = EP.two_d(output_size)
        out = st.outputs.get((OH, OW))
        if out is None:
            out = st.outputs[(OH, OW)] = (torch.empty((OH, OW, self.cs), dtype=torch.float32, device=self.device),
                                          torch.empty((OH, OW), dtype=torch.uint8, device=self.device))
        canvas = self._canvas(st, H, W)
        K.eval_score_accumulate(logits, (PH, PW), flip, rect, canvas=canvas, store=True)
        K.eval_rescale_accumulate(canvas, self.class_num, (0, 0, H, W), out[0], store=True, classes=out[1])
        return out[1]

    def scale_process(self, img, plan, store, classes=None):
        """evaluator.py:243-295 for one scale of `plan` (an eval_plan.ScalePlan of this image): every window's exp-score summed
        on the scale's canvas, the score rectangle resized to the image and added into (store: written to) the image's fp32
        total; with `classes`, the arg-max of the updated total is written there and returned, else the total."""
        img, st = self._upload(img)
        crop = plan.crop
        flip = self.is_flip
        eng = self._lowres_engine((2 if flip else 1, 3, crop, crop))
        if plan.sliding:
            canvas = self._canvas(st, plan.canvas_h, plan.canvas_w)
            canvas.zero_()
            for d in plan.descs:
                K.eval_window_input(d, img, plan.ytab, plan.xtab, eng.input)
                K.eval_score_accumulate(eng.run(), (crop, crop), flip, (0, 0, crop, crop), canvas=canvas, at=(d.oy, d.ox))
            rect = (plan.top, plan.left, plan.rows, plan.cols)
        else:
            canvas = self._canvas(st, plan.rows, plan.cols)
            K.eval_window_input(plan.descs[0], img, plan.ytab, plan.xtab, eng.input)
            K.eval_score_accumulate(eng.run(), (crop, crop), flip, (plan.top, plan.left, plan.rows, plan.cols), canvas=canvas, store=True)
            rect = (0, 0, plan.rows, plan.cols)
        K.eval_rescale_accumulate(canvas, self.class_num, rect, st.total, store=store, classes=classes)
        return st.total if classes is None else classes

    def sliding_eval(self, img, crop_size, stride_rate):
        """evaluator.py:228-241: the sum over self.multi_scales of scale_process, arg-max over the classes.  Returns the uint8
        class map on the device; the summed score stays in the image's total buffer."""
        img, st = self._upload(img)
        H, W = int(img.shape[0]), int(img.shape[1])
        plans = self._plan(st, H, W, crop_size, stride_rate)
        for i, p in enumerate(plans):
            self.scale_process(img, p, store=(i == 0), classes=st.classes if i == len(plans) - 1 else None)
        return st.classes

    def predict(self, img, min_confidence=0.0, ignore_label=255, output_size=None, input_size=None):
        """The class map AND the per-pixel confidence of the configured mode: (classes, confidence), both uint8 (H, W) on the device.
        confidence = floor(255 conf + 0.5) with conf the share of the winning class in the mode's score (exp(logit), summed over the
        scales and flips the mode has); classes holds `ignore_label` where that byte is below kernels.confidence_threshold(
        min_confidence), and with min_confidence=0 it is the map whole_eval / sliding_eval return for the same image.
        One scale without flip, padding or output_size: a "classes+confidence" engine, built on first use and kept (one launch,
        fs_bilinear_argmax_conf, writes both maps); flip / input_size / output_size: the score canvas, then fs_score_confidence;
        several scales: fs_score_confidence on the image's summed total after the last scale.  The maps are buffers that the next
        call with the same image shape overwrites."""
        K.confidence_threshold(min_confidence), K._check_ignore_label(ignore_label)
        if len(self.multi_scales) > 1:
            assert output_size is None and input_size is None, "output_size / input_size belong to the single-scale mode"
            img, st = self._upload(img)
            H, W = int(img.shape[0]), int(img.shape[1])
            plans = self._plan(st, H, W, self.crop_size, self.stride_rate)
            for i, p in enumerate(plans):
                self.scale_process(img, p, store=(i == 0))
            return K.score_confidence(st.total, self.class_num, min_confidence, ignore_label, classes=st.classes, conf=st.conf)
        if output_size is None and input_size is None and not self.is_flip:
            # (one engine per image shape, threshold byte and ignore label: they are arguments of the engine's captured final launch)
            x = self._upload(img)[0] if self.uint8_input else self.process_image(img)
            H, W = (int(v) for v in (x.shape[:2] if self.uint8_input else x.shape[2:]))
            classes, conf = self._conf_engine(H, W, min_confidence, ignore_label)(x)
            return classes[0], conf[0]
        img, st = self._upload(img)
        H, W = int(img.shape[0]), int(img.shape[1])
        ih, iw = EP.two_d(input_size) if input_size is not None else (H, W)
        top, bottom, left, right = EP.pad_margins(H, W, ih, iw)
        PH, PW = H + top + bottom, W + left + right
        flip = self.is_flip
        eng = self._lowres_engine((2 if flip else 1, 3, PH, PW))
        ytab, xtab = self._identity_taps(st, H, W)
        d = K.eval_window_desc(H, W, H, W, top, left, 0, 0, PH, PW, EP.PAD_NORMALISED, flip, self._mean, self._std)
        K.eval_window_input(d, img, ytab, xtab, eng.input)
        canvas = self._canvas(st, H, W)
        K.eval_score_accumulate(eng.run(), (PH, PW), flip, (top, left, H, W), canvas=canvas, store=True)
        if output_size is None:
            return K.score_confidence(canvas, self.class_num, min_confidence, ignore_label, classes=st.classes, conf=st.conf)
        OH, OW = EP.two_d(output_size)
        out = st.outputs.get((OH, OW))
        if out is None:
            out = st.outputs[(OH, OW)] = (torch.empty((OH, OW, self.cs), dtype=torch.float32, device=self.device),
                                          torch.empty((OH, OW), dtype=torch.uint8, device=self.device))
        cout = st.outputs.get(("conf", OH, OW))
        if cout is None:
            cout = st.outputs[("conf", OH, OW)] = torch.empty((OH, OW), dtype=torch.uint8, device=self.device)
        K.eval_rescale_accumulate(canvas, self.class_num, (0, 0, H, W), out[0], store=True)
        return K.score_confidence(out[0], self.class_num, min_confidence, ignore_label, classes=out[1], conf=cout)

    def func_per_iteration(self, data):
        """data: {'data': HWC uint8 image, 'label': (H, W) labels}; accumulates on the device, returns the class map.
        Dispatch of train/eval.py:23-26: one scale -> whole_eval (the scale value is not used), more -> sliding_eval."""
        if len(self.multi_scales) == 1:
            pred = self.whole_eval(data['data'])
        else:
            pred = self.sliding_eval(data['data'], self.crop_size, self.stride_rate)
        label = torch.as_tensor(data['label']).to(self.device)
        self.acc.add(pred, label.contiguous())
        if self.save_path is not None or self.show_image or self.show_prediction:
            self._save(data, pred, label)
        return pred

    def _save(self, data, pred, label):
        """train/eval.py:30-51: `<fn>.png` under save_path (the working directory without one) - with show_image the image |
        prediction | ground-truth strip, with show_prediction the painted image, else the raw class map.  The reference writes the
        picture after the map, so where both land in one directory the picture is what the file holds; the same here."""
        from . import tester, visualize as V
        if self._writer is None:
            self._writer = tester.PredictionWriter(device=self.device)
        folder = self.save_path if self.save_path is not None else os.getcwd()
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, data['fn'] + ".png")
        H, W = int(pred.shape[0]), int(pred.shape[1])
        if not (self.show_image or self.show_prediction):
            self._writer.submit([(path, (H, W))], lambda views: views[0].copy_(pred))
            return
        if self.labels is None:
            raise ValueError("show_image / show_prediction need labels (a visualize.LabelSpec)")
        img = torch.as_tensor(data['data']).to(self.device).contiguous()
        if self.show_image:
            gt = label if label.dtype == torch.uint8 else label.to(torch.uint8)       # 255 and -1 both: 255
            Wt = 3 * W + 2 * V.PIVOT
            self._writer.submit([(path, (H, Wt, 3))], lambda views: V.compose(self.labels, self.labels.background, img, [pred, gt],
                                                                              [False, True], [0.55, 0.55], image_panel=True, out=views[0]))
        else:
            self._writer.submit([(path, (H, W, 3))], lambda views: V.compose(self.labels, self.labels.background, img, [pred], [False], [1],
                                                                             out=views[0]))

    def finish_writing(self):
        """Block until every file queued by func_per_iteration is on disk (re-raises a writer thread's exception)."""
        if self._writer is not None:
            writer, self._writer = self._writer, None
            writer.close()

    def compute_metric(self):
        hist, labeled, correct = self.acc.result()
        iu, mean_IU, mean_IU_no_back, mean_pixel_acc = compute_score(hist, correct, labeled)
        return {"iu": iu, "mean_IU": mean_IU, "mean_IU_no_back": mean_IU_no_back, "mean_pixel_acc": mean_pixel_acc,
                "hist": hist, "labeled": labeled, "correct": correct}
