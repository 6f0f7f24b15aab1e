"""The end of a search epoch (search/train_search.py:141-212, 259-303) without plots, tensorboard or tqdm: supernet validation on the
device, the searched architectures' latencies, the exported `arch_{idx}.pt` files and the latency-weight schedule.

Reference, per validation mode: `infer()` runs the evaluator once per head (`evaluator.out_idx` = 0..4, heads
["8s", "16s", "32s", "8s_32s", "16s_32s"]), and every image of every sweep is a supernet forward, exp() of the up-sampled
(19, H, W) score map, its copy to the host, np.argmax and hist_info there (tools/engine/evaluator.py:297-318,
tools/seg_opr/metric.py:7-17).  Here (SupernetEvaluator): the image is normalised on the device (fs_eval_window_input with identity
taps: the reference's numpy normalisation bit for bit), ONE `forward_lowres` gives all five heads at 1/8 resolution, and ONE
fs_heads_confusion launch up-samples, arg-maxes and counts them into five confusion histograms that stay on the device until
`run()` reads 5 x 19 x 19 counts.

share_forward (default True) is where this departs from the reference's order: its five sweeps are five forwards per image.  In the
"min" / "max" modes (and for a fixed architecture) the five forwards are identical and the shared forward gives the same counts.
The "random" and "arch_ratio" modes draw new widths (np.random.choice, Gumbel noise) on every forward: shared, the five heads see
ONE draw per image where the reference gives them five, and the host RNGs advance by a fifth as much.  share_forward=False runs
the reference's five sweeps, one head each, in its order (head after head, image after image): same draws, same counts.
"""
import os

import numpy as np
import torch

from . import eval_plan as EP
from . import functional as FN
from . import kernels as K
from .metric import compute_score
from .model_seg import Network_Multi_Path_Infer

HEAD_NAMES = ["8s", "16s", "32s", "8s_32s", "16s_32s"]        # train_search.py:128 valid_names


class SupernetEvaluator:
    """Validation of a supernet's heads over `source` (dataloader.ArraySource / FileListSource; the reference's val split is
    loaded with down_sampling=2 by BaseDataset._open_image).  run() -> [mean_IU of each head of out_indices] (evaluator.py
    run_online_multiprocess + search/eval.py compute_metric); compute_metric() -> one dict per head, shaped like
    SegEvaluator.compute_metric()."""

    def __init__(self, model, class_num, image_mean, image_std, source, out_indices=(0, 1, 2, 3, 4), dtype=torch.float32,
                 share_forward=True):
        self.model = model
        self.class_num = int(class_num)
        self.source = source
        self.out_indices = tuple(int(i) for i in out_indices)
        assert 1 <= len(self.out_indices) <= 8 and all(0 <= i < 5 for i in self.out_indices), "heads are 0..4"
        self.dtype = dtype
        self.share_forward = bool(share_forward)
        self.device = source.device
        self._mean = [float(v) for v in np.asarray(image_mean, dtype=np.float32)]
        self._std = [float(v) for v in np.asarray(image_std, dtype=np.float32)]
        n = len(self.out_indices)
        self.hist = torch.zeros(n * self.class_num * self.class_num, dtype=torch.int64, device=self.device)
        self.counts = torch.zeros(2 * n, dtype=torch.int64, device=self.device)
        self._inputs = {}                   # (H, W) -> (network input (1, 3, H, W) fp32, identity y taps, identity x taps)

    def _input(self, img):
        """The uint8 (H, W, 3) image as the normalised network input, built on the device (whole_eval's padded path of
        evaluator.py:206-225 with nothing to pad: process_image's normalize, img_utils.py:178-184)."""
        H, W = int(img.shape[0]), int(img.shape[1])
        buf = self._inputs.get((H, W))
        if buf is None:
            taps = [torch.from_numpy(EP.pack_taps(*EP.linear_taps(s, s, 1.0))).to(self.device) for s in (H, W)]
            buf = self._inputs[(H, W)] = (torch.empty((1, 3, H, W), dtype=torch.float32, device=self.device), taps[0], taps[1])
        inp, ytab, xtab = buf
        d = K.eval_window_desc(H, W, H, W, 0, 0, 0, 0, H, W, EP.PAD_NORMALISED, 0, self._mean, self._std)
        K.eval_window_input(d, img, ytab, xtab, inp)
        return inp

    def _heads(self, inp):
        prev = FN.get_compute_dtype()
        FN.set_compute_dtype(self.dtype)
        try:
            return self.model.forward_lowres(inp)
        finally:
            FN.set_compute_dtype(prev)

    def _slice(self, i):
        cc = self.class_num * self.class_num
        return self.hist[i * cc:(i + 1) * cc], self.counts[2 * i:2 * i + 2]

    def run(self):
        """One validation pass of the supernet in its current arch_idx / prun_mode: the mean_IU of each head of out_indices."""
        self.model.eval()
        self.hist.zero_()
        self.counts.zero_()
        with torch.no_grad():
            if self.share_forward:
                for i in range(len(self.source)):
                    img, lbl = self.source.get(i)
                    preds = self._heads(self._input(img))
                    K.heads_confusion([preds[o] for o in self.out_indices], lbl, self.hist, self.counts)
            else:
                for n, o in enumerate(self.out_indices):           # evaluator.out_idx = o, one sweep each (train_search.py:262-265)
                    hist, counts = self._slice(n)
                    for i in range(len(self.source)):
                        img, lbl = self.source.get(i)
                        preds = self._heads(self._input(img))
                        K.heads_confusion([preds[o]], lbl, hist, counts)
        return [m["mean_IU"] for m in self.compute_metric()]

    def compute_metric(self):
        """One dict per head of out_indices (iu, mean_IU, mean_IU_no_back, mean_pixel_acc, hist, labeled, correct); one read of the
        device counts."""
        C = self.class_num
        hist = self.hist.cpu().numpy().reshape(-1, C, C)
        counts = self.counts.cpu().numpy().reshape(-1, 2)
        out = []
        for h, (labeled, correct) in zip(hist, counts):
            iu, mean_IU, mean_IU_no_back, mean_pixel_acc = compute_score(h, int(correct), int(labeled))
            out.append({"iu": iu, "mean_IU": mean_IU, "mean_IU_no_back": mean_IU_no_back, "mean_pixel_acc": mean_pixel_acc,
                        "hist": h, "labeled": int(labeled), "correct": int(correct)})
        return out


def supernet_infer(model, evaluator, fps=True):
    """train_search.py:259-271 infer(): the five heads' mIoUs, plus the current architecture's two FPS with fps=True."""
    model.eval()
    mIoUs = evaluator.run()
    if fps:
        fps0, fps1 = arch_fps(model)
        return mIoUs, fps0, fps1
    return mIoUs


def arch_fps(model, input_size=(1, 3, 1024, 2048)):
    """train_search.py:274-303 arch_logging() without its plots: the derived network of the current arch_idx, its latency with the
    last branches [2, 0], then [2, 1] built on the SAME object (the reference's order; the second structure inherits state from the
    first - a fresh [2, 1] network gives another number), each from the latency lookup table.  The reference moves the network to
    the GPU before each forward_latency; a table lookup does not need it (an entry missing from the table is measured on the GPU
    either way).  Returns (fps0, fps1) = 1000 / latency."""
    names = model._arch_names[model.arch_idx]
    arch = lambda n: getattr(model, n).detach().cpu().clone()
    net = Network_Multi_Path_Infer(
        [arch(n) for n in names["alphas"]], [None] + [arch(n) for n in names["betas"]], [arch(n) for n in names["ratios"]],
        num_classes=model._num_classes, layers=model._layers, Fch=model._Fch, width_mult_list=model._width_mult_list,
        stem_head_width=model._stem_head_width[model.arch_idx])
    net.build_structure([2, 0])
    net.eval()
    latency0, _ = net.forward_latency(input_size[1:])
    net.build_structure([2, 1])
    net.eval()
    latency1, _ = net.forward_latency(input_size[1:])
    return 1000. / latency0, 1000. / latency1


def validate_epoch(model, evaluator, pretrain):
    """The validation block of an epoch (train_search.py:141-183).  pretrain == True: {"min": mIoUs} and, with more than one width,
    "max" and "random" too (prun_mode left at the last one, as there); otherwise prun_mode = None and, per architecture index,
    (mIoUs, fps0, fps1) in a list (arch_idx left at the last one).  The model comes back in train mode: the reference's next epoch
    starts with model.train() (train_search.py:216), the steps here set it only when they are built."""
    try:
        with torch.no_grad():
            if pretrain == True:                # noqa: E712  (the reference's test: a path string is not True)
                results = {}
                modes = ["min"] + (["max", "random"] if len(model._width_mult_list) > 1 else [])
                for mode in modes:
                    model.prun_mode = mode
                    results[mode] = supernet_infer(model, evaluator, fps=False)
            else:
                results = []
                model.prun_mode = None
                for idx in range(len(model._arch_names)):
                    model.arch_idx = idx
                    results.append(supernet_infer(model, evaluator))
    finally:
        model.train()
    return results


def arch_states(model, results, pretrain, per_arch=False):
    """The `arch_{idx}.pt` dicts of train_search.py:185-202: each architecture's alpha / beta / ratio tensors plus mIoU02, mIoU12
    (heads "8s_32s", "16s_32s"), latency02 and latency12 (ms).  `results` is validate_epoch's search-mode list.  The reference
    writes them only when `pretrain` is a path string (the search phase; [] otherwise), and fills the four numbers of EVERY
    architecture from the variables its validation loop left behind, i.e. the LAST evaluated architecture's (the shipped arch_0 and
    arch_1 carry identical numbers).  per_arch=True gives each architecture its own numbers instead.  The numbers are stored as Python
    floats, so a plain torch.load (weights_only) reads the files back."""
    if not isinstance(pretrain, str):
        return []
    states = []
    for idx, arch_name in enumerate(model._arch_names):
        mIoUs, fps0, fps1 = results[idx] if per_arch else results[-1]
        state = {}
        for name in arch_name["alphas"] + arch_name["betas"] + arch_name["ratios"]:
            state[name] = getattr(model, name).detach().clone()
        # Python floats: the evaluator's mIoUs are numpy scalars (np.nanmean), which torch.load's default weights_only=True refuses
        state["mIoU02"] = float(mIoUs[3])
        state["mIoU12"] = float(mIoUs[4])
        state["latency02"] = float(1000. / fps0)
        state["latency12"] = float(1000. / fps1)
        states.append(state)
    return states


def save_arch(directory, states, epoch):
    """torch.save of each state as arch_{idx}_{epoch}.pt and arch_{idx}.pt (train_search.py:201-202); returns the paths."""
    paths = []
    for idx, state in enumerate(states):
        for name in ("arch_%d_%d.pt" % (idx, epoch), "arch_%d.pt" % idx):
            path = os.path.join(directory, name)
            torch.save(state, path)
            paths.append(path)
    return paths


def update_latency_weight(architect, fps, FPS_min, FPS_max):
    """train_search.py:204-212: for every architecture with a positive latency weight, halve it when either of its two FPS
    (fps[idx] = (fps0, fps1)) reaches FPS_max[idx], else double it when either is at or below FPS_min[idx].  Returns the list."""
    w = architect.latency_weight
    for idx in range(len(w)):
        if w[idx] > 0:
            if (int(fps[idx][0] >= FPS_max[idx]) + int(fps[idx][1] >= FPS_max[idx])) >= 1:
                w[idx] /= 2
            elif (int(fps[idx][0] <= FPS_min[idx]) + int(fps[idx][1] <= FPS_min[idx])) > 0:
                w[idx] *= 2
    return w
