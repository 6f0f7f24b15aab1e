"""Host reference of the align_corners=True bilinear up-sample as the NCHW logits writers of csrc/resize.hip compute it: tap indices and
weights in fp32 exactly as make_tap does (scale = (in-1)/(out-1), src = scale * dst, i0 = (int)src, l1 = src - i0, l0 = 1 - l1, every
step rounded to fp32), the blend of the four stored values in fp64."""
import numpy as np


def taps(in_size, out_size):
    """(i0, i1, l0, l1) per output index; the weights are the fp32 values, returned as float64"""
    f = np.float32
    scale = f(in_size - 1) / f(out_size - 1) if out_size > 1 else f(0)
    src = (scale * np.arange(out_size, dtype=np.float32)).astype(np.float32)
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def upsample(x, size):
    """x: (N, C, Hi, Wi) array of the stored values -> (N, C, Ho, Wo) float64"""
    x = np.asarray(x, dtype=np.float64)
    h0, h1, a0, a1 = taps(x.shape[2], size[0])
    w0, w1, b0, b1 = taps(x.shape[3], size[1])
    top = x[:, :, h0][:, :, :, w0] * b0 + x[:, :, h0][:, :, :, w1] * b1
    bot = x[:, :, h1][:, :, :, w0] * b0 + x[:, :, h1][:, :, :, w1] * b1
    return top * a0[:, None] + bot * a1[:, None]
