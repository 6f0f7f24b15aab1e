"""Tensor-level wrappers over the C ABI: torch tensors in, raw pointers + sizes out.

Activation convention: a feature map is a torch tensor of logical shape (N, C, H, W) whose memory is NHWC with a
channel stride cs >= C (strides (H*W*cs, 1, W*cs, cs)); channel slices of a wider buffer are therefore valid
operands and torch.cat becomes "write into a slice".  torch is used only for memory, streams and autograd plumbing.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FS_BF16, FS_CONV_RELU, FS_CONV_RELU_TAIL, FS_CONV_TRANSPOSED, FS_F16, FS_F32, ConvDesc, ResizeDesc, ZoomDesc, call

_DT = {torch.float32: FS_F32, torch.bfloat16: FS_BF16, torch.float16: FS_F16}
# what trains: float16 is an inference storage type (the C ABI refuses it in every training entry point)
TRAIN_DTYPES = (torch.float32, torch.bfloat16)
DTYPE_NAMES = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def dtype_code(dt):
    try:
        return _DT[dt]
    except KeyError:
        raise TypeError("fasterseg_amd kernels support float32, bfloat16 and (inference only) float16, got %s" % dt)


def elem_size(dt):
    """Bytes per element of a storage type (a torch dtype or an fs_dtype code)."""
    if not isinstance(dt, torch.dtype):
        if dt not in _DT.values():
            raise TypeError("unknown fs_dtype code %r" % (dt,))
        return 4 if dt == FS_F32 else 2
    dtype_code(dt)
    return 4 if dt == torch.float32 else 2


def vec_of(dt):
    """Elements per 16-byte vector."""
    return 16 // elem_size(dt)


def require_train_dtype(dt, what):
    if dt not in TRAIN_DTYPES:
        raise TypeError("%s: training runs in float32 or bfloat16, got %s (float16 is an inference-engine storage type)" % (what, dt))


def round_up(v, m):
    return (v + m - 1) // m * m


def _stream():
    """hipStream_t of torch's current stream.  torch.cuda.current_stream() costs ~15 us per call (it re-reads an environment
    variable to resolve the device index), which was a quarter of an eager supernet step; the raw C accessors are ~0.3 us."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _ZeroPool:
    """Arena of pre-zeroed fp32 scratch (BN statistic / reduction accumulators, dot outputs).  A train step needs
    thousands of 100-byte zero buffers; taking them from one arena that is cleared with a single memset per step
    (reset(), called by parallel.FlatGradientSync.prepare) removes one fill launch per request.  Views are only valid
    until the next reset; outside an active step (or when the arena is full) requests fall back to torch.zeros."""

    def __init__(self, capacity=1 << 24):
        self.capacity = capacity
        self.buf = None
        self.off = 0
        self.active = False
        self.cap_buf = None          # arena owned by the hipGraph being captured (begin_capture / end_capture)
        self.cap_off = 0

    def begin_capture(self, device, capacity=1 << 22):
        """Call as the FIRST thing inside a graph capture: one captured fill re-zeroes the arena on every replay, and the
        requests of the captured pass are slices of it instead of one fill launch each (~1.5 k per supernet pass)."""
        self.cap_buf = torch.zeros(capacity, dtype=torch.float32, device=device)
        self.cap_off = 0

    def end_capture(self):
        """Returns the arena; the caller keeps it alive as long as the graph."""
        buf, self.cap_buf = self.cap_buf, None
        return buf

    def reset(self, device):
        if self.buf is None or self.buf.device != torch.device(device):
            self.buf = torch.zeros(self.capacity, dtype=torch.float32, device=device)
        elif self.off:
            self.buf[:self.off].zero_()
        self.off = 0
        self.active = True

    def stop(self):
        self.active = False

    def take(self, n, device, align=4):
        """n zeroed floats; `align` (floats, power of two): alignment of the view's first element inside the arena (the arena itself is
        allocator-aligned: 512 bytes)."""
        if self.cap_buf is not None and torch.cuda.is_current_stream_capturing():
            off = (self.cap_off + align - 1) & ~(align - 1)
            if off + n <= self.cap_buf.numel():
                self.cap_off = off + ((n + 3) & ~3)
                return self.cap_buf[off:off + n]
        if (not self.active or self.buf is None or self.buf.device != torch.device(device)
                or torch.cuda.is_current_stream_capturing()):      # a captured graph must own (and re-zero) its scratch
            return torch.zeros(n, dtype=torch.float32, device=device)
        off = (self.off + align - 1) & ~(align - 1)
        if off + n > self.capacity:
            return torch.zeros(n, dtype=torch.float32, device=device)
        self.off = off + ((n + 3) & ~3)         # keep 16-byte alignment
        return self.buf[off:off + n]


zero_pool = _ZeroPool()


def zeros_f32(n, device):
    return zero_pool.take(n, device)


def empty_nhwc(N, C, H, W, dtype, device, cs=None, zero=False):
    """(N,C,H,W) view over a fresh NHWC buffer with channel stride cs (default: C rounded up to the vector width)."""
    cs = cs or round_up(C, vec_of(dtype))
    make = torch.zeros if zero else torch.empty
    buf = make((N, H, W, cs), dtype=dtype, device=device)
    return buf.permute(0, 3, 1, 2)[:, :C]


def channel_stride(t):
    """Channel stride of an NHWC view, or None if `t` is not laid out that way."""
    if t.dim() != 4:
        return None
    N, C, H, W = t.shape
    sN, sC, sH, sW = t.stride()
    cs = sW
    if C > 1 and sC != 1:
        return None
    if cs < C:
        return None
    if (H > 1 and sH != W * cs) or (N > 1 and sN != H * W * cs):
        return None
    return cs


def is_nhwc(t, dtype=None):
    if not t.is_cuda or t.dtype not in _DT or (dtype is not None and t.dtype != dtype):
        return False
    cs = channel_stride(t)
    if cs is None:
        return False
    v = vec_of(t.dtype)
    return cs % v == 0 and t.data_ptr() % 16 == 0


def require_nhwc(t, what="tensor"):
    if not is_nhwc(t):
        raise ValueError("%s must be an NHWC-strided CUDA tensor (shape %s, strides %s, dtype %s)" %
                         (what, tuple(t.shape), t.stride(), t.dtype))
    return channel_stride(t)


def to_nhwc(x, dtype):
    """Any (N,C,H,W) CUDA tensor -> NHWC view of `dtype` (fs_nchw_to_nhwc for contiguous fp32 NCHW inputs)."""
    if is_nhwc(x, dtype):
        return x
    N, C, H, W = x.shape
    if is_nhwc(x):            # NHWC but other dtype: widen/narrow through NCHW fp32
        x = to_nchw(x)
    src = x.detach().to(torch.float32).contiguous()
    cpad = round_up(C, vec_of(dtype))
    out = empty_nhwc(N, C, H, W, dtype, x.device, cs=cpad)
    call("fs_nchw_to_nhwc", _stream(), N, C, H, W, _p(src), _p(out), cpad, cpad, dtype_code(dtype))
    return out


def to_nchw(x):
    """NHWC view -> contiguous NCHW fp32."""
    cs = require_nhwc(x, "x")
    N, C, H, W = x.shape
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    call("fs_nhwc_to_nchw", _stream(), N, C, H, W, _p(x), cs, dtype_code(x.dtype), _p(out))
    return out


# ---------------------------------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------------------------------
def pack_weight(w, dtype, cout=None, cin=None, flip=False, rows=None):
    """OIHW fp32 (optionally the leading [:cout,:cin] slice, slimmable_ops.py:42) -> packed [Cout][R][S][Cin] `dtype`.
    flip=True gives the data-gradient filter [Cin][R][S][Cout] rotated by 180 degrees.  `rows` zero-pads the leading
    dimension (used for the 19-class classifier)."""
    O, I, R, S = w.shape
    cout = O if cout is None else cout
    cin = I if cin is None else cin
    assert w.dtype == torch.float32 and w.stride(3) == 1 and w.stride(2) == S, "filter must be fp32 with contiguous taps"
    lead, inner = (cin, cout) if flip else (cout, cin)
    nrows = lead if rows is None else rows
    make = torch.zeros if nrows != lead else torch.empty
    out = make((nrows, R, S, inner), dtype=dtype, device=w.device)
    call("fs_pack_weight", _stream(), _p(w), w.stride(0), w.stride(1), cout, cin, R, S, dtype_code(dtype), int(flip), _p(out))
    return out


def unpack_weight_grad(dw_packed, grad, cout, cin, accumulate=False):
    """packed fp32 [cout][R][S][cin] -> grad[:cout,:cin] of an OIHW fp32 tensor."""
    R, S = grad.shape[2], grad.shape[3]
    call("fs_unpack_weight_grad", _stream(), _p(dw_packed), cout, cin, R, S, _p(grad), grad.stride(0), grad.stride(1),
         int(accumulate))


# ---------------------------------------------------------------------------------------------------
# convolution
# ---------------------------------------------------------------------------------------------------
WORKSPACE_BYTES = 16 << 20          # FS_CONV_WORKSPACE_BYTES
WS_COUNTER_BYTES = 65536            # FS_WS_COUNTER_BYTES: the workspace's tail holds zero-initialised arrival counters
_workspaces = {}


def stream_workspace(device):
    """(address, bytes) of the split-K scratch buffer of the current stream: convs that share a workspace must be ordered,
    which holds for everything issued on one stream (inside a capture too: one buffer per forked lane)."""
    raw = torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    ws = _workspaces.get(raw)
    if ws is None:
        ws = _workspaces[raw] = torch.empty(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
        ws[-WS_COUNTER_BYTES:].zero_()         # arrival counters of the deterministic reductions: zero once, every kernel leaves them zero
    return ws.data_ptr(), WORKSPACE_BYTES


def conv_desc(x_shape, x_cs, cout, R, S, stride, pad, y_cs, dtype, flags=0, out_hw=None):
    N, Cin, H, W = x_shape
    if out_hw is None:
        Ho = (H + 2 * pad - R) // stride + 1
        Wo = (W + 2 * pad - S) // stride + 1
    else:
        Ho, Wo = out_hw
    return ConvDesc(N, H, W, Cin, cout, R, S, stride, pad, Ho, Wo, x_cs, y_cs, dtype_code(dtype), flags)


def conv2d(x, w_packed, cout, R, S, stride, pad, scale=None, shift=None, relu=False, out=None, stats=None,
           transposed=False, out_hw=None, w_strides=None, workspace=True, vres=None):
    """y = relu?(conv(x, w) * scale + shift); `out` may be a channel slice of a wider NHWC buffer.  w_strides = (row, tap)
    element strides when the filter is the leading block of a wider packed bank; workspace=False keeps the whole contraction
    in one block per tile (no cross-block split-K).  vres = (H, W, relu): the convolution reads x bilinearly resampled
    (align_corners=True, optional ReLU after the interpolation) to H x W without materialising that map."""
    x_cs = require_nhwc(x, "x")
    N, Cin, H, W = x.shape
    flags = (FS_CONV_RELU if relu else 0) | (FS_CONV_TRANSPOSED if transposed else 0)
    d = conv_desc((N, Cin, vres[0], vres[1]) if vres else x.shape, x_cs, cout, R, S, stride, pad, 0, x.dtype, flags, out_hw)
    if vres:
        d.vr_H, d.vr_W, d.vr_relu = H, W, int(bool(vres[2]))
    if out is None:
        out = empty_nhwc(N, cout, d.Ho, d.Wo, x.dtype, x.device)
    else:
        assert tuple(out.shape) == (N, cout, d.Ho, d.Wo) and out.dtype == x.dtype, (tuple(out.shape), (N, cout, d.Ho, d.Wo))
    d.y_cs = channel_stride(out)
    assert d.y_cs is not None
    if w_strides is not None:
        d.w_os, d.w_ts = w_strides
    ws, ws_bytes = stream_workspace(x.device) if workspace else (None, 0)
    call("fs_conv2d_fwd_ws", _stream(), ctypes.byref(d), _p(x), _p(w_packed), _p(scale), _p(shift), _p(out), _p(stats), ws,
         ws_bytes)
    return out


def pack_weight_frag(w, dtype, cout=None, cin=None):
    """OIHW fp32 3x3 filter (optionally the leading [:cout,:cin] block) -> MFMA-fragment-ordered bank for conv3x3_halo."""
    O, I, R, S = w.shape
    assert (R, S) == (3, 3) and w.dtype == torch.float32 and w.stride(3) == 1 and w.stride(2) == 3
    cout = O if cout is None else cout
    cin = I if cin is None else cin
    n = _lib.lib().fs_packed_weight_frag_elems(cout, cin, dtype_code(dtype))
    out = torch.empty(n, dtype=dtype, device=w.device)
    call("fs_pack_weight_frag", _stream(), _p(w), w.stride(0), w.stride(1), cout, cin, dtype_code(dtype), _p(out))
    return out


def conv3x3_halo(x, w_frag, cout, scale=None, shift=None, relu=False, out=None, stats=None, stride=1, tile=0, ksplit=None, vres=None):
    """3x3 / pad 1 conv at stride 1 or 2 through the halo-tiled kernel (same epilogue contract as conv2d); tile = forced
    output-channel tile (32 / 64 / 128, 0: heuristic); ksplit = True / 16 / False forces the K-split form with 32- / 16-channel tiles / forbids it (None: the
    library's rule, fs_conv3x3_halo_plan); vres = (H, W, relu): the convolution reads x bilinearly resampled to H x W
    (align_corners=True, optional ReLU after the interpolation) while it stages it, stride 1 only."""
    x_cs = require_nhwc(x, "x")
    N, Cin, H, W = x.shape
    flags = (FS_CONV_RELU if relu else 0) | {0: 0, 32: 0x1000, 64: 0x2000, 128: 0x3000}[tile]
    flags |= 0 if ksplit is None else (_lib.FS_CONV_KSPLIT16 if ksplit == 16 else _lib.FS_CONV_KSPLIT if ksplit else _lib.FS_CONV_NO_KSPLIT)
    d = conv_desc((N, Cin, vres[0], vres[1]) if vres else x.shape, x_cs, cout, 3, 3, stride, 1, 0, x.dtype, flags)
    if vres:
        d.vr_H, d.vr_W, d.vr_relu = H, W, int(bool(vres[2]))
    if out is None:
        out = empty_nhwc(N, cout, d.Ho, d.Wo, x.dtype, x.device)
    d.y_cs = channel_stride(out)
    call("fs_conv3x3_s1_fwd", _stream(), ctypes.byref(d), _p(x), _p(w_frag), _p(scale), _p(shift), _p(out), _p(stats))
    return out


def conv3x3_halo_plan(d, has_stats=False):
    """(tile, ksplit, workgroups) of the launch fs_conv3x3_s1_fwd makes for descriptor `d` (host only, no device needed)."""
    tile, ks, wg = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    call("fs_conv3x3_halo_plan", ctypes.byref(d), int(bool(has_stats)), ctypes.byref(tile), ctypes.byref(ks), ctypes.byref(wg))
    return tile.value, ks.value, wg.value


def conv_pw_desc(x_shape, x_cs, c3, cout, y_cs, dtype, relu=False, relu_post=False, rows=0):
    """fs_conv_pw_desc of a 3x3 / stride-1 conv (-> c3 channels) with a 1x1 conv (-> cout) behind it; rows = 4 / 8 pins the rows per block."""
    N, Cin, H, W = x_shape
    flags = (_lib.FS_PW_RELU_3X3 if relu else 0) | (_lib.FS_PW_RELU_POST if relu_post else 0) | {0: 0, 4: _lib.FS_PW_ROWS4, 8: _lib.FS_PW_ROWS8}[rows]
    return _lib.ConvPwDesc(N, H, W, Cin, c3, cout, x_cs, y_cs, dtype_code(dtype), flags)


def conv3x3_pw_plan(d):
    """(rows per block, workgroups, LDS bytes per block) of the launch fs_conv3x3_pw_fwd makes for `d` (host only, no device needed)."""
    rows, wg, lds = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()
    call("fs_conv3x3_pw_plan", ctypes.byref(d), ctypes.byref(rows), ctypes.byref(wg), ctypes.byref(lds))
    return rows.value, wg.value, lds.value


def conv3x3_pw(x, w_frag, c3, scale, shift, relu, w_post, cout, scale_post=None, shift_post=None, relu_post=False, out=None, rows=0):
    """3x3 / stride 1 / pad 1 conv -> 1x1 conv in one launch (conv3x3_pw.hip) with the arithmetic of the separate launches.  w_frag: the
    fragment pack of the 3x3, w_post: the dense fs_pack_weight bank of the 1x1; `out` may be a channel slice of a wider NHWC buffer."""
    x_cs = require_nhwc(x, "x")
    N, Cin, H, W = x.shape
    if out is None:
        out = empty_nhwc(N, cout, H, W, x.dtype, x.device)
    else:
        assert tuple(out.shape) == (N, cout, H, W) and out.dtype == x.dtype, (tuple(out.shape), (N, cout, H, W))
    d = conv_pw_desc(x.shape, x_cs, c3, cout, channel_stride(out), x.dtype, relu, relu_post, rows)
    call("fs_conv3x3_pw_fwd", _stream(), ctypes.byref(d), _p(x), _p(w_frag), _p(scale), _p(shift), _p(w_post), _p(scale_post), _p(shift_post),
         _p(out))
    return out


def zoom_desc(x_shape, x_cs, cmid, cout, down, up, y_cs, dtype):
    N, Cin, H, W = x_shape
    h, w = (H // 2, W // 2) if down else (H, W)
    Ho, Wo = (2 * h, 2 * w) if up else (h, w)
    return ZoomDesc(N, H, W, Cin, cmid, cout, h, w, Ho, Wo, x_cs, y_cs, dtype_code(dtype), int(bool(down)), int(bool(up)))


def zoom_cell_supported(d):
    return bool(_lib.lib().fs_zoom_cell_supported(ctypes.byref(d)))


def zoom_cell(x, w1_frag, scale1, shift1, w2_frag, scale2, shift2, cmid, cout, down=True, up=True, out=None):
    """A whole zoomed-conv cell in one launch (zoom_cell.hip): [1/2 bilinear] -> conv3x3*s1+b1, ReLU -> conv3x3*s2+b2 ->
    [x2 bilinear] -> ReLU.  Filters in fragment order (pack_weight_frag)."""
    x_cs = require_nhwc(x, "x")
    d = zoom_desc(x.shape, x_cs, cmid, cout, down, up, 0, x.dtype)
    if out is None:
        out = empty_nhwc(d.N, cout, d.Ho, d.Wo, x.dtype, x.device)
    else:
        assert tuple(out.shape) == (d.N, cout, d.Ho, d.Wo) and out.dtype == x.dtype
    d.y_cs = channel_stride(out)
    call("fs_zoom_cell_fwd", _stream(), ctypes.byref(d), _p(x), _p(w1_frag), _p(scale1), _p(shift1), _p(w2_frag), _p(scale2),
         _p(shift2), _p(out))
    return out


def conv2d_wgrad(x, dy, R, S, stride, pad, cout=None):
    """fp32 packed weight gradient [Cout][R][S][Cin] of conv(x) w.r.t. its filter."""
    x_cs = require_nhwc(x, "x")
    dy_cs = require_nhwc(dy, "dy")
    N, Cin, H, W = x.shape
    cout = dy.shape[1] if cout is None else cout
    d = conv_desc(x.shape, x_cs, cout, R, S, stride, pad, dy_cs, x.dtype, 0, (dy.shape[2], dy.shape[3]))
    dw = torch.zeros((cout, R, S, Cin), dtype=torch.float32, device=x.device)
    ws, ws_bytes = stream_workspace(x.device)       # deterministic slab reduction (fs_conv2d_wgrad alone would use fp32 atomics)
    call("fs_conv2d_wgrad_ws", _stream(), ctypes.byref(d), _p(x), _p(dy), _p(dw), R * S * Cin, 1, Cin, ws, ws_bytes)
    return dw


def conv2d_wgrad_into(x, dy, R, S, stride, pad, grad, cout=None):
    """Accumulate the weight gradient straight into `grad[:cout, :Cin]`, a logically-OIHW fp32 tensor whose taps have a
    uniform stride (OIHW-contiguous, or physically [O][R][S][I] = coalesced atomics): a parameter's .grad or a fresh zero
    tensor.  No packed temporary, no unpack pass."""
    x_cs = require_nhwc(x, "x")
    dy_cs = require_nhwc(dy, "dy")
    N, Cin, H, W = x.shape
    cout = dy.shape[1] if cout is None else cout
    assert grad.dtype == torch.float32 and grad.stride(2) == S * grad.stride(3) and grad.shape[0] >= cout and grad.shape[1] >= Cin
    d = conv_desc(x.shape, x_cs, cout, R, S, stride, pad, dy_cs, x.dtype, 0, (dy.shape[2], dy.shape[3]))
    ws, ws_bytes = stream_workspace(x.device)       # slab partials + arrival counters: bit-reproducible, no fp32 atomics
    call("fs_conv2d_wgrad_ws", _stream(), ctypes.byref(d), _p(x), _p(dy), _p(grad), grad.stride(0), grad.stride(1), grad.stride(3), ws, ws_bytes)
    return grad


def conv_stem(x_nchw, w_packed, cout, scale, shift, relu, dtype, out=None):
    N, C, H, W = x_nchw.shape
    assert C == 3 and x_nchw.dtype == torch.float32 and x_nchw.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = empty_nhwc(N, cout, Ho, Wo, dtype, x_nchw.device)
    call("fs_conv_stem_fwd", _stream(), N, H, W, cout, _p(x_nchw), _p(w_packed), _p(scale), _p(shift), _p(out),
         channel_stride(out), dtype_code(dtype), int(relu))
    return out


def conv_stem_u8(img_nhwc, w_packed, cout, scale, shift, relu, dtype, mean, std, out=None):
    """fs_conv_stem_u8_fwd: the stem on a uint8 (N, H, W, 3) RGB frame, normalised as ((float)u / 255 - mean[c]) / std[c] while it is
    staged.  The frame may start at any byte (a slice of a larger buffer); W % 4 == 0 and a 4-byte aligned start take the tiled kernels."""
    N, H, W, C = img_nhwc.shape
    assert C == 3 and img_nhwc.dtype == torch.uint8 and img_nhwc.is_contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = empty_nhwc(N, cout, Ho, Wo, dtype, img_nhwc.device)
    # (float16 goes through the three-type entry point: fs_conv_stem_u8_fwd keeps its published fp32 / bf16 contract)
    call("fs_conv_stem_u8_infer_fwd" if dtype == torch.float16 else "fs_conv_stem_u8_fwd", _stream(), N, H, W, cout, _p(img_nhwc), _p(w_packed), _p(scale), _p(shift), _p(out),
         channel_stride(out), dtype_code(dtype), int(relu), *([float(v) for v in mean] + [float(v) for v in std]))
    return out


# ---------------------------------------------------------------------------------------------------
# bilinear (align_corners=True)
# ---------------------------------------------------------------------------------------------------
def bilinear(x, size, relu=False, out=None, out_nchw=0, channels=None):
    """out_nchw: 0 -> NHWC view; 1 -> contiguous NCHW fp32; 2 -> contiguous NCHW in x.dtype.
    `channels` overrides C (reading the first C channels of a padded buffer)."""
    x_cs = channel_stride(x)
    N, C, Hi, Wi = x.shape
    C = C if channels is None else channels
    Ho, Wo = int(size[0]), int(size[1])
    if out_nchw:
        odt = torch.float32 if out_nchw == 1 else x.dtype
        if out is None:
            out = torch.empty((N, C, Ho, Wo), dtype=odt, device=x.device)
        y_cs = 0
    else:
        require_nhwc(x, "x")
        if out is None:
            out = empty_nhwc(N, C, Ho, Wo, x.dtype, x.device)
        y_cs = channel_stride(out)
    d = ResizeDesc(N, Hi, Wi, Ho, Wo, C, x_cs, y_cs, dtype_code(x.dtype), int(relu), int(out_nchw))
    call("fs_bilinear_fwd", _stream(), ctypes.byref(d), _p(x), _p(out))
    return out


def _logits_resize_desc(x, size):
    x_cs = channel_stride(x)
    assert x_cs is not None, "logits must be an NHWC view"
    N, C, Hi, Wi = x.shape
    return ResizeDesc(N, Hi, Wi, int(size[0]), int(size[1]), C, x_cs, 0, dtype_code(x.dtype), 0, 0)


def _u8_map(t, shape, device, what):
    if t is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    assert t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == tuple(shape), "%s: a contiguous uint8 %s" % (what, tuple(shape))
    return t


def bilinear_argmax(x, size, classes=None):
    """fs_bilinear_argmax: NHWC logits view (N, C, h, w) -> uint8 (N, Ho, Wo) arg-max of the align_corners=True up-sample to `size`."""
    d = _logits_resize_desc(x, size)
    classes = _u8_map(classes, (d.N, d.Ho, d.Wo), x.device, "classes")
    call("fs_bilinear_argmax", _stream(), ctypes.byref(d), _p(x), _p(classes))
    return classes


def confidence_threshold(t):
    """min_confidence in [0, 1] -> the byte the kernels compare with: ceil(255 t) (0 -> 0: nothing is masked, 0.9 -> 230, 1 -> 255; the
    float product, so that k / 255 gives k for every byte k)."""
    import math
    t = float(t)
    if not 0.0 <= t <= 1.0:        # a NaN fails both comparisons
        raise ValueError("min_confidence must be in [0, 1], got %r" % (t,))
    return int(math.ceil(255.0 * t))


def _check_ignore_label(ignore_label):
    if isinstance(ignore_label, bool) or int(ignore_label) != ignore_label or not 0 <= int(ignore_label) <= 255:
        raise ValueError("ignore_label must be an integer in 0..255, got %r" % (ignore_label,))
    return int(ignore_label)


def class_threshold_bytes(thresholds, class_num):
    """Per-class thresholds -> uint8 numpy (256,), entry k for class k, entries >= class_num 0.  `thresholds`: one value or class_num
    values; a uint8 array is taken as the bytes the kernels compare with, anything else as floats in [0, 1] through
    confidence_threshold.  A wrong length or a value out of range: ValueError."""
    class_num = int(class_num)
    if not 1 <= class_num <= 256:
        raise ValueError("class_num must be in 1..256, got %r" % (class_num,))
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    a = np.asarray(thresholds)
    if a.ndim > 1 or a.dtype == object or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError("class_thresholds: one value or %d values, floats in [0, 1] or a uint8 array of bytes" % class_num)
    if a.ndim == 1 and a.shape[0] != class_num:
        raise ValueError("class_thresholds: %d values for %d classes" % (a.shape[0], class_num))
    if a.dtype == np.uint8:
        values = a.astype(np.uint8)
    else:
        try:
            values = np.array([confidence_threshold(v) for v in a.reshape(-1)], dtype=np.uint8)
        except ValueError:
            raise ValueError("class_thresholds: every value must be in [0, 1] (bytes go in a uint8 array), got %r" % (thresholds,))
    table = np.zeros(256, dtype=np.uint8)
    table[:class_num] = values if a.ndim == 1 else values.reshape(())
    return table


def class_threshold_table(thresholds, class_num, device):
    """The 256-byte device table the _pc launches read (class_threshold_bytes on the device)."""
    return torch.from_numpy(class_threshold_bytes(thresholds, class_num)).to(device)


def _threshold_args(min_confidence, class_thresholds, device):
    """(entry-point suffix, threshold argument) of a confidence launch: the scalar byte, or the device table with the _pc symbol"""
    if class_thresholds is None:
        return "", confidence_threshold(min_confidence)
    if confidence_threshold(min_confidence) != 0:
        raise ValueError("class_thresholds and min_confidence exclude each other (got min_confidence=%r)" % (min_confidence,))
    t = class_thresholds
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.numel() == 256 and t.is_contiguous() and t.device == device):
        raise ValueError("class_thresholds must be the uint8[256] tensor of class_threshold_table on %s" % (device,))
    return "_pc", _p(t)


def bilinear_argmax_conf(x, size, min_confidence=0.0, ignore_label=255, classes=None, conf=None, class_thresholds=None):
    """fs_bilinear_argmax_conf: NHWC logits view (N, C, h, w) -> (classes, conf), both uint8 (N, Ho, Wo): the arg-max of the up-sample with
    `ignore_label` where the confidence byte is below confidence_threshold(min_confidence), and the byte q = floor(255 p + 0.5) of the
    winner's softmax probability.  classes=False / conf=False: that map is not written (None is returned in its place).
    class_thresholds (a class_threshold_table): fs_bilinear_argmax_conf_pc, class k is kept where q >= table[k]."""
    d = _logits_resize_desc(x, size)
    ig = _check_ignore_label(ignore_label)
    pc, th = _threshold_args(min_confidence, class_thresholds, x.device)
    shape = (d.N, d.Ho, d.Wo)
    classes = None if classes is False else _u8_map(classes, shape, x.device, "classes")
    conf = None if conf is False else _u8_map(conf, shape, x.device, "conf")
    call("fs_bilinear_argmax_conf" + pc, _stream(), ctypes.byref(d), _p(x), _p(classes), _p(conf), th, ig)
    return classes, conf


def score_confidence(score, C, min_confidence=0.0, ignore_label=255, classes=None, conf=None, class_thresholds=None):
    """fs_score_confidence on a contiguous fp32 score buffer (..., cs) of summed exp-scores: per pixel the first maximum over the first C
    channels and its share of their sum as a byte -> (classes, conf), uint8 of shape score.shape[:-1].  classes=False / conf=False and
    class_thresholds (fs_score_confidence_pc) as in bilinear_argmax_conf."""
    assert score.dtype == torch.float32 and score.is_contiguous() and score.dim() >= 2
    ig = _check_ignore_label(ignore_label)
    pc, th = _threshold_args(min_confidence, class_thresholds, score.device)
    shape = tuple(score.shape[:-1])
    classes = None if classes is False else _u8_map(classes, shape, score.device, "classes")
    conf = None if conf is False else _u8_map(conf, shape, score.device, "conf")
    call("fs_score_confidence" + pc, _stream(), _p(score), score.numel() // score.shape[-1], int(score.shape[-1]), int(C), _p(classes), _p(conf),
         th, ig)
    return classes, conf


def confidence_hist(classes, conf, C, gt=None, hist=None):
    """fs_confidence_hist: adds the (class, confidence byte) counts of two uint8 maps of one shape into `hist`, an int64 (2, C, 256) device
    tensor (created zeroed when None) and returns it.  Plane 0 alone without labels; with gt (uint8 / int32 / int64, the maps' shape):
    plane 0 where the class is the label, plane 1 where it is not, pixels labelled outside [0, C) skipped.  The maps may be views at any
    byte offset as long as they are contiguous."""
    assert classes.dtype == torch.uint8 and conf.dtype == torch.uint8 and classes.is_contiguous() and conf.is_contiguous()
    assert classes.shape == conf.shape, (classes.shape, conf.shape)
    if hist is None:
        hist = torch.zeros((2, int(C), 256), dtype=torch.int64, device=classes.device)
    assert hist.dtype == torch.int64 and hist.is_contiguous() and tuple(hist.shape) == (2, int(C), 256), "hist: a contiguous int64 (2, C, 256)"
    gt_bytes = 0
    if gt is not None:
        assert gt.shape == classes.shape and gt.is_contiguous(), "labels: the maps' shape, contiguous"
        try:
            gt_bytes = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}[gt.dtype]
        except KeyError:
            raise TypeError("labels must be uint8, int32 or int64, got %s" % gt.dtype)
    call("fs_confidence_hist", _stream(), _p(classes), _p(conf), _p(gt), gt_bytes, classes.numel(), int(C), _p(hist))
    return hist


def bilinear_bwd(dy, y_out, in_shape, relu, dtype, out_nchw=0, dx_cs=None):
    """Gradient w.r.t. the input of `bilinear`; dy NHWC (or contiguous NCHW fp32 when out_nchw)."""
    N, C, Hi, Wi = in_shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    dx = empty_nhwc(N, C, Hi, Wi, dtype, dy.device, cs=dx_cs, zero=bool(out_nchw))
    if out_nchw:
        assert dy.is_contiguous() and dy.dtype == torch.float32
        y_cs = 0
    else:
        y_cs = require_nhwc(dy, "dy")
        if relu:
            assert channel_stride(y_out) == y_cs, "y_out and dy must share a channel stride"
    d = ResizeDesc(N, Hi, Wi, Ho, Wo, C, channel_stride(dx), y_cs, dtype_code(dtype), int(relu), int(out_nchw))
    if out_nchw and Ho >= 2 * Hi and Wo >= 2 * Wi:          # logits up-sample: separable two-pass gather
        d.out_nchw = 1
        ws = torch.empty((N, C, Ho, Wi), dtype=torch.float32, device=dy.device)
        call("fs_bilinear_bwd_nchw", _stream(), ctypes.byref(d), _p(dy), _p(ws), _p(dx))
        return dx
    call("fs_bilinear_bwd", _stream(), ctypes.byref(d), _p(dy), _p(y_out) if relu else None, _p(dx))
    return dx


# ---------------------------------------------------------------------------------------------------
# batch norm / elementwise
# ---------------------------------------------------------------------------------------------------
def _pix(t):
    return t.shape[0] * t.shape[2] * t.shape[3]


def bn_finalize(stats, count, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked=None):
    C = stats.numel() // 2
    mean, invstd, scale, shift = torch.empty((4, C), dtype=torch.float32, device=stats.device).unbind(0)
    call("fs_bn_finalize", _stream(), C, int(count), _p(stats), _p(gamma), _p(beta), float(eps), float(momentum),
         _p(running_mean), _p(running_var), _p(mean), _p(invstd), _p(scale), _p(shift), _p(num_batches_tracked))
    return mean, invstd, scale, shift


def bn_train_apply(x, stats, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, relu):
    """fs_bn_finalize + fs_affine_act in one launch: returns (y, saved) with saved = [mean | invstd | scale | shift]."""
    x_cs = require_nhwc(x, "x")
    C = x.shape[1]
    y = empty_nhwc(x.shape[0], C, x.shape[2], x.shape[3], x.dtype, x.device)
    saved = torch.empty(4 * C, dtype=torch.float32, device=x.device)
    call("fs_bn_train_apply", _stream(), _pix(x), C, _p(x), x_cs, _p(stats), _p(gamma), _p(beta), float(eps), float(momentum),
         _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(saved), _p(y), channel_stride(y), dtype_code(x.dtype),
         int(relu))
    return y, saved


def affine_act(x, scale, shift, relu, out=None):
    x_cs = require_nhwc(x, "x")
    if out is None:
        out = empty_nhwc(*x.shape[:1], x.shape[1], x.shape[2], x.shape[3], x.dtype, x.device)
    call("fs_affine_act", _stream(), _pix(x), x.shape[1], _p(x), x_cs, _p(scale), _p(shift), _p(out), channel_stride(out),
         dtype_code(x.dtype), int(relu))
    return out


def channel_stats(x, stats=None):
    x_cs = require_nhwc(x, "x")
    if stats is None:
        stats = zeros_f32(2 * x.shape[1], x.device)
    ws, ws_bytes = stream_workspace(x.device)       # block partials added up in block order: bit-reproducible, no float atomics
    call("fs_channel_stats_ws", _stream(), _pix(x), x.shape[1], 1, _p(x), x_cs, dtype_code(x.dtype), _p(stats), ws, ws_bytes)
    return stats


def bn_backward(z, dy, y_out, mean, invstd, gamma, relu, dgamma_acc=None, dbeta_acc=None):
    """Returns (dz, dgamma, dbeta) for y = relu?(gamma*(z-mean)*invstd + beta); with dgamma_acc/dbeta_acc (fp32 [C]) the two
    parameter gradients are also accumulated into those buffers by the apply pass."""
    z_cs, dy_cs = require_nhwc(z, "z"), require_nhwc(dy, "dy")
    C = z.shape[1]
    y_cs = require_nhwc(y_out, "y_out") if relu else 0
    red = zeros_f32(2 * C, z.device)
    dt = dtype_code(z.dtype)
    ws, ws_bytes = stream_workspace(z.device)
    call("fs_bn_bwd_reduce_ws", _stream(), _pix(z), C, 1, _p(z), z_cs, _p(dy), dy_cs, _p(y_out) if relu else None, y_cs, _p(mean),
         _p(invstd), 0, dt, int(relu), _p(red), ws, ws_bytes)
    dz = empty_nhwc(z.shape[0], C, z.shape[2], z.shape[3], z.dtype, z.device)
    call("fs_bn_bwd_apply", _stream(), _pix(z), C, _p(z), z_cs, _p(dy), dy_cs, _p(y_out) if relu else None, y_cs, _p(mean),
         _p(invstd), _p(gamma), _p(red), _pix(z), dt, int(relu), _p(dz), channel_stride(dz), _p(dgamma_acc), _p(dbeta_acc))
    return dz, red[C:], red[:C]


BN_COL_MAX_PIXELS = 512        # csrc/units.hip: maps up to this many pixels per group take the one-launch column-owner BatchNorm


def bn_act_train(z, gamma, beta, eps, momentum, running_mean, running_var, num_batches_tracked, relu, groups=1):
    """Train-mode BatchNorm(+ReLU) of z with `groups` independent equal parts of the batch (fs_bn_act_train_fwd):
    returns (y, saved) with saved = [groups][mean | invstd | scale | shift]."""
    z_cs = require_nhwc(z, "z")
    C = z.shape[1]
    y = empty_nhwc(z.shape[0], C, z.shape[2], z.shape[3], z.dtype, z.device)
    saved = torch.empty(groups * 4 * C, dtype=torch.float32, device=z.device)
    pixels = _pix(z)
    stats = zeros_f32(groups * 2 * C, z.device) if pixels // groups > BN_COL_MAX_PIXELS else None
    call("fs_bn_act_train_fwd", _stream(), pixels, C, groups, _p(z), z_cs, _p(gamma), _p(beta), float(eps), float(momentum),
         _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(stats), _p(saved), _p(y), channel_stride(y),
         dtype_code(z.dtype), int(relu), *stream_workspace(z.device))
    return y, saved


def bn_act_train_bwd(z, dy, y_out, saved, gamma, relu, groups=1, dgamma_acc=None, dbeta_acc=None):
    """(dz, dgamma, dbeta) of bn_act_train; dgamma/dbeta are summed over the groups."""
    z_cs, dy_cs = require_nhwc(z, "z"), require_nhwc(dy, "dy")
    C = z.shape[1]
    y_cs = require_nhwc(y_out, "y_out") if relu else 0
    red = zeros_f32((groups + 1 if groups > 1 else 1) * 2 * C, z.device)
    dz = empty_nhwc(z.shape[0], C, z.shape[2], z.shape[3], z.dtype, z.device)
    call("fs_bn_act_train_bwd", _stream(), _pix(z), C, groups, _p(z), z_cs, _p(dy), dy_cs, _p(y_out) if relu else None, y_cs,
         _p(saved), _p(gamma), _p(red), dtype_code(z.dtype), int(relu), _p(dz), channel_stride(dz), _p(dgamma_acc), _p(dbeta_acc),
         *stream_workspace(z.device))
    return dz, red[C:2 * C], red[:C]


def copy_channels(x, out):
    call("fs_copy_channels", _stream(), _pix(x), x.shape[1], _p(x), require_nhwc(x, "x"), _p(out), require_nhwc(out, "out"),
         dtype_code(x.dtype))
    return out


def axpy(x, alpha, out, accumulate):
    """out (+)= alpha * x, alpha a 1-element fp32 device tensor."""
    call("fs_axpy_channels", _stream(), _pix(x), x.shape[1], _p(x), require_nhwc(x, "x"), _p(alpha), _p(out),
         require_nhwc(out, "out"), dtype_code(x.dtype), int(accumulate))
    return out


def dot(x, y):
    out = zeros_f32(1, x.device)
    call("fs_dot", _stream(), _pix(x), x.shape[1], _p(x), require_nhwc(x, "x"), _p(y), require_nhwc(y, "y"),
         dtype_code(x.dtype), _p(out))
    return out


def _operand_arrays(tensors):
    n = len(tensors)
    ptrs = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in tensors])
    strides = (ctypes.c_int * n)(*[0 if t is None else t.stride(3) for t in tensors])
    return n, ptrs, strides


def weighted_sum(xs, coef, out=None):
    """out = sum_k coef[k] * xs[k]; xs are NHWC views of one shape/dtype, coef a contiguous fp32 device vector."""
    x0 = xs[0]
    for t in xs:
        require_nhwc(t, "operand")
    n, ptrs, strides = _operand_arrays(xs)
    if out is None:
        out = empty_nhwc(*x0.shape, x0.dtype, x0.device)
    call("fs_weighted_sum", _stream(), _pix(x0), x0.shape[1], n, ptrs, strides, coef.data_ptr(), out.data_ptr(), out.stride(3),
         dtype_code(x0.dtype))
    return out


def weighted_sum_bwd(dy, coef, need, outs=None):
    """[coef[k] * dy if need[k] else None for k] (written into `outs` when given)."""
    dy_cs = require_nhwc(dy, "dy")
    if outs is None:
        outs = [empty_nhwc(*dy.shape, dy.dtype, dy.device) if nd else None for nd in need]
    n, ptrs, strides = _operand_arrays(outs)
    call("fs_weighted_sum_bwd", _stream(), _pix(dy), dy.shape[1], n, dy.data_ptr(), dy_cs, coef.data_ptr(), ptrs, strides,
         dtype_code(dy.dtype))
    return outs


def weighted_sum_dots(dy, xs):
    """fp32 vector [<dy, x_k>]."""
    dy_cs = require_nhwc(dy, "dy")
    n, ptrs, strides = _operand_arrays(xs)
    out = zeros_f32(n, dy.device)             # the step's zero arena (one fill per step / graph replay) instead of one fill launch per call
    call("fs_weighted_sum_dots", _stream(), _pix(dy), dy.shape[1], n, dy.data_ptr(), dy_cs, ptrs, strides, dtype_code(dy.dtype),
         out.data_ptr())
    return out


def cat_channels(tensors):
    """torch.cat(dim=1) for NHWC views (model_seg.py:307-331): one fs_copy_channels per operand."""
    N, _, H, W = tensors[0].shape
    total = sum(t.shape[1] for t in tensors)
    out = empty_nhwc(N, total, H, W, tensors[0].dtype, tensors[0].device)
    off = 0
    for t in tensors:
        copy_channels(t, out[:, off:off + t.shape[1]])
        off += t.shape[1]
    return out


def eval_window_desc(H, W, rows, cols, top, left, oy, ox, crop_h, crop_w, pad_mode, flip, mean, std):
    """fs_eval_window_desc: window (oy, ox) of the canvas holding the (rows, cols) resize of an (H, W) image at (top, left)."""
    return _lib.EvalWindowDesc(H, W, rows, cols, top, left, oy, ox, crop_h, crop_w, pad_mode, int(flip),
                               (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std]))


def eval_window_input(d, img, ytab, xtab, out):
    """fs_eval_window_input: uint8 (H, W, 3) image -> resized / padded / normalised window in out (1 + flip, 3, crop_h, crop_w) fp32.
    ytab / xtab: int32 (rows, 2) / (cols, 2) tap tables (eval_plan.pack_taps)."""
    assert img.dtype == torch.uint8 and img.is_contiguous() and tuple(img.shape) == (d.H, d.W, 3)
    assert ytab.dtype == torch.int32 and tuple(ytab.shape) == (d.rows, 2) and xtab.dtype == torch.int32 and tuple(xtab.shape) == (d.cols, 2)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape[1:]) == (3, d.crop_h, d.crop_w) and out.shape[0] >= 1 + d.flip
    call("fs_eval_window_input", _stream(), ctypes.byref(d), _p(img), _p(ytab.contiguous()), _p(xtab.contiguous()), _p(out))
    return out


def eval_score_accumulate(logits, size, flip, rect, canvas=None, at=(0, 0), store=False, classes=None):
    """fs_eval_score_accumulate on the "lowres" engine output `logits` (N, C, h, w) NHWC view whose x8 up-sample is the window `size`:
    over the window rectangle rect = (y0, x0, rows, cols), exp(l0 (+ l1 mirrored)) added (stored) into the fp32 HWC canvas
    (Hc, Wc, cs) at `at`, or, with `classes` ((rows, cols) uint8), the arg-max of l0 (+ l1 mirrored)."""
    N, C, h, w = logits.shape
    cs = channel_stride(logits)
    assert cs is not None, "logits must be an NHWC view"
    d = _lib.LogitsDesc(N, h, w, C, cs, int(size[0]), int(size[1]), dtype_code(logits.dtype))
    y0, x0, rows, cols = (int(v) for v in rect)
    if classes is not None:
        assert classes.dtype == torch.uint8 and classes.is_contiguous() and classes.numel() == rows * cols
        call("fs_eval_score_accumulate", _stream(), ctypes.byref(d), _p(logits), int(flip), y0, x0, rows, cols, None, 0, 0, 0, 0, 0, 0,
             _p(classes))
        return classes
    assert canvas.dtype == torch.float32 and canvas.is_contiguous() and canvas.dim() == 3
    Hc, Wc, ccs = canvas.shape
    call("fs_eval_score_accumulate", _stream(), ctypes.byref(d), _p(logits), int(flip), y0, x0, rows, cols, _p(canvas), Hc, Wc, ccs,
         int(at[0]), int(at[1]), int(bool(store)), None)
    return canvas


def eval_rescale_accumulate(canvas, C, rect, total, store=False, classes=None):
    """fs_eval_rescale_accumulate: total (H, W, cs) fp32 (+)= cv2 INTER_LINEAR resize of the canvas (Hc, Wc, cs) rectangle
    rect = (y0, x0, rows, cols); with `classes` ((H, W) uint8) also the arg-max of the updated total over C classes."""
    assert canvas.dtype == torch.float32 and canvas.is_contiguous() and canvas.dim() == 3
    assert total.dtype == torch.float32 and total.is_contiguous() and total.dim() == 3 and total.shape[2] == canvas.shape[2]
    Hc, Wc, cs = canvas.shape
    H, W = total.shape[:2]
    if classes is not None:
        assert classes.dtype == torch.uint8 and classes.is_contiguous() and classes.numel() == H * W
    y0, x0, rows, cols = (int(v) for v in rect)
    call("fs_eval_rescale_accumulate", _stream(), _p(canvas), Hc, Wc, cs, int(C), y0, x0, rows, cols, _p(total), H, W, int(bool(store)),
         _p(classes))
    return total


def heads_confusion(heads, gt, hist, counts):
    """fs_heads_confusion: K <= 8 low-resolution heads (N, C, h, w) NHWC views of one dtype and geometry, each bilinearly up-sampled
    (align_corners=True) to the labels' (H, W) and arg-maxed, counted into hist (K, C, C) / (K * C * C) and counts (K, 2) / (2 K)
    int64 accumulators on the device: hist[k, gt, pred] += 1, counts[k] += (labeled, correct).  gt: (N, H, W) or (H, W) uint8 /
    int32 / int64 labels (255, -1 or >= C: ignored)."""
    heads = list(heads)
    K = len(heads)
    assert 1 <= K <= _lib.FS_MAX_HEADS, "1..%d heads" % _lib.FS_MAX_HEADS
    N, C, h, w = heads[0].shape
    cs = []
    for t in heads:
        assert tuple(t.shape) == (N, C, h, w) and t.dtype == heads[0].dtype and t.is_cuda, "the heads must share shape, dtype and device"
        c = channel_stride(t)
        assert c is not None, "heads must be NHWC views"
        cs.append(c)
    gt_bytes = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}.get(gt.dtype)
    assert gt_bytes is not None, "labels must be uint8, int32 or int64, got %s" % gt.dtype
    assert gt.is_cuda and gt.is_contiguous() and ((gt.dim() == 3 and gt.shape[0] == N) or (gt.dim() == 2 and N == 1)), \
        "labels: (N, H, W), or (H, W) for N = 1"
    H, W = int(gt.shape[-2]), int(gt.shape[-1])
    for t, n in ((hist, K * C * C), (counts, 2 * K)):
        assert t.dtype == torch.int64 and t.is_cuda and t.is_contiguous() and t.numel() == n, "accumulators: int64, contiguous"
    d = _lib.HeadsDesc(K, N, h, w, C, H, W, dtype_code(heads[0].dtype), (ctypes.c_int * _lib.FS_MAX_HEADS)(*cs))
    ptrs = (ctypes.c_void_p * K)(*[t.data_ptr() for t in heads])
    call("fs_heads_confusion", _stream(), ctypes.byref(d), ptrs, _p(gt), gt_bytes, _p(hist), _p(counts))
    return hist, counts


def train_batch(bd, samples, images, labels, tables, norm, staging, args, out_img, out_lbl):
    """fs_train_batch: samples int32 (B, 16) host array of fs_train_sample rows, images / labels: B device uint8 tensors ((H, W, 3) /
    (H, W)), tables int32 device tensor of bd.n_tables entries or more, norm (3, 256) fp32, staging / args: pinned host / device uint8
    tensors of fs_train_batch_args_bytes(B) bytes or more -> out_img (B, 3, crop_h, crop_w) fp32, out_lbl (B, crop_h / g, crop_w / g)
    int64.  The caller keeps `staging` untouched until the upload issued on the current stream has completed."""
    B = bd.B
    assert samples.dtype == np.int32 and samples.flags.c_contiguous and samples.shape == (B, 16) and len(images) == len(labels) == B
    for im, lb, row in zip(images, labels, samples):
        assert im.dtype == torch.uint8 and im.is_contiguous() and tuple(im.shape) == (int(row[0]), int(row[1]), 3), "bad source image"
        assert lb.dtype == torch.uint8 and lb.is_contiguous() and tuple(lb.shape) == (int(row[0]), int(row[1])), "bad source label"
    assert tables.dtype == torch.int32 and tables.numel() >= bd.n_tables and norm.dtype == torch.float32 and norm.numel() == 768
    nbytes = _lib.lib().fs_train_batch_args_bytes(B)
    assert staging.numel() >= nbytes and args.numel() >= nbytes and args.is_cuda and not staging.is_cuda
    assert out_img.dtype == torch.float32 and out_img.is_contiguous() and tuple(out_img.shape) == (B, 3, bd.crop_h, bd.crop_w)
    assert out_lbl.dtype == torch.int64 and out_lbl.is_contiguous() and tuple(out_lbl.shape) == (B, bd.crop_h // bd.g, bd.crop_w // bd.g)
    ptrs = (ctypes.c_void_p * (2 * B))(*[t.data_ptr() for t in images], *[t.data_ptr() for t in labels])
    call("fs_train_batch", _stream(), ctypes.byref(bd), samples.ctypes.data, ptrs, ctypes.addressof(ptrs) + B * ctypes.sizeof(ctypes.c_void_p),
         _p(tables), _p(norm), ctypes.c_void_p(staging.data_ptr()), _p(args), _p(out_img), _p(out_lbl))
    return out_img, out_lbl


def resize_u8(src, out, ytab, xtab, nearest):
    """fs_resize_u8: uint8 (H, W[, C]) -> out (h, w[, C]); linear: ytab / xtab int32 (h, 2) / (w, 2) taps, nearest: int32 (h,) / (w,)."""
    assert src.dtype == torch.uint8 and src.is_contiguous() and out.dtype == torch.uint8 and out.is_contiguous()
    assert src.dim() == out.dim() and src.dim() in (2, 3) and src.shape[2:] == out.shape[2:]
    H, W = src.shape[:2]
    h, w = out.shape[:2]
    C = src.shape[2] if src.dim() == 3 else 1
    assert ytab.dtype == torch.int32 and xtab.dtype == torch.int32
    assert ytab.shape[0] == h and xtab.shape[0] == w and ytab.numel() == h * (1 if nearest else 2) and xtab.numel() == w * (1 if nearest else 2)
    call("fs_resize_u8", _stream(), _p(src), H, W, C, _p(out), h, w, _p(ytab.contiguous()), _p(xtab.contiguous()), int(bool(nearest)))
    return out


def render_prediction(image, maps, palette, composite=None, col=0, image_panel=False, gap=15, background=-1, show255=(), weights=(),
                      lut=None, ids=None):
    """fs_render_prediction: image (H, W, 3) uint8 and up to 4 class maps (H, W) uint8 -> the panels of one launch written into
    `composite` ((H, Wc, 3) uint8, strides (pitch, 3, 1)) from pixel column `col` on: the untouched image first with image_panel, then
    one overlay per map (set_img_color with show255[i] and weight_foreground weights[i]), `gap` black columns between the panels;
    with `ids` ((H, W) uint8) also ids = lut[maps[0]] (lut: 256 uint8).  palette: (n, 3) uint8 RGB, n <= 256.  Without weights
    (no overlay panel) `maps` holds the one map of the ids; without any panel composite and image may be None.  Returns the pixel
    columns written (0 without a composite)."""
    maps = list(maps)
    panels = len(weights)
    assert len(show255) == panels <= _lib.FS_RENDER_MAX_PANELS, "one show255 and one weight per overlay panel, 4 at the most"
    assert len(maps) == panels or (panels == 0 and len(maps) == 1 and ids is not None), "one class map per overlay panel (or the one of the ids)"
    assert composite is not None or (panels == 0 and not image_panel), "panels need a composite"
    H, W = (int(v) for v in maps[0].shape) if maps else (int(v) for v in image.shape[:2])
    for m in maps:
        assert m.dtype == torch.uint8 and m.is_cuda and m.is_contiguous() and tuple(m.shape) == (H, W), "class maps: (H, W) uint8, contiguous"
    P = panels + int(bool(image_panel))
    span = W * P + int(gap) * (P - 1) if P else 0
    d = _lib.RenderDesc(H, W, panels, int(bool(image_panel)), int(gap), 0, 0, int(background), int(ids is not None))
    dst = None
    if P:
        assert image.dtype == torch.uint8 and image.is_cuda and image.is_contiguous() and tuple(image.shape) == (H, W, 3), "image: (H, W, 3) uint8"
        assert composite.dtype == torch.uint8 and composite.is_cuda and composite.dim() == 3 and composite.shape[0] == H and \
            composite.shape[2] == 3 and composite.stride(1) == 3 and composite.stride(2) == 1, "composite: (H, Wc, 3) uint8 rows"
        assert 0 <= col and col + span <= composite.shape[1], "the panels do not fit the composite"
        d.dst_pitch = int(composite.stride(0)) if H > 1 else max(int(composite.stride(0)), 3 * span)
        dst = ctypes.c_void_p(composite.data_ptr() + 3 * int(col))
    if panels:
        assert palette.dtype == torch.uint8 and palette.is_cuda and palette.is_contiguous() and palette.dim() == 2 and palette.shape[1] == 3
        d.n_colors = int(palette.shape[0])
        for i in range(panels):
            d.show255[i] = int(bool(show255[i]))
            d.alpha[i] = float(weights[i])
            d.beta[i] = 1.0 - float(weights[i])          # the subtraction in double, as the reference's (1 - weight_foreground)
    if ids is not None:
        assert ids.dtype == torch.uint8 and ids.is_cuda and ids.is_contiguous() and tuple(ids.shape) == (H, W)
        assert lut.dtype == torch.uint8 and lut.is_cuda and lut.is_contiguous() and lut.numel() == 256
    ptrs = (ctypes.c_void_p * _lib.FS_RENDER_MAX_PANELS)(*[m.data_ptr() for m in maps])
    call("fs_render_prediction", _stream(), ctypes.byref(d), _p(image) if P else None, ptrs, _p(palette) if panels else None, _p(lut),
         dst, _p(ids))
    return span


def png_rows_per_band(rows, row_bytes):
    """Default band height of png_deflate: the largest that still cuts the map into at least 256 bands (one workgroup each: a chip's
    worth) when it has that many rows, and whose filtered bytes fit a workgroup's LDS (FS_PNG_BAND_MAX_BYTES).  4 at 1024 x 2048."""
    fit = _lib.FS_PNG_BAND_MAX_BYTES // (int(row_bytes) + 1)
    if fit < 1:
        raise ValueError("png_deflate: a row of %d bytes is above the %d filtered bytes of a band" % (row_bytes, _lib.FS_PNG_BAND_MAX_BYTES))
    return max(1, min((int(rows) - 1) // 255, fit))


def png_deflate_sizes(rows, row_bytes, rows_per_band):
    """(bytes of `out`: fs_png_deflate_bound, bytes of the workspace) of a geometry."""
    h = _lib.lib()
    return int(h.fs_png_deflate_bound(rows, row_bytes, rows_per_band)), int(h.fs_png_deflate_workspace_bytes(rows, row_bytes, rows_per_band))


def png_deflate(map, rows_per_band=None, out=None, workspace=None, out_bytes=None):
    """fs_png_deflate: a uint8 device tensor (H, W) or (H, W, 3), unit stride inside a row and any row pitch, -> the zlib stream of its
    PNG IDAT chunk (Up filter, fixed-Huffman bands of run-length matches: the header states the bytes).  Returns (out, out_bytes): a
    uint8 buffer of at least the bound and an int64 (1,) device tensor holding the stream's length; both, and the workspace (uint8, 16-byte
    aligned), are created when not passed.  Two launches on the current stream, nothing is read back."""
    assert map.dtype == torch.uint8 and map.is_cuda and map.dim() in (2, 3) and map.numel() > 0, "map: a uint8 device tensor (H, W) or (H, W, 3)"
    H, W = int(map.shape[0]), int(map.shape[1])
    if map.dim() == 3:
        assert map.shape[2] == 3 and map.stride(2) == 1 and map.stride(1) == 3, "an (H, W, 3) map has dense rows"
        row_bytes = 3 * W
    else:
        assert map.stride(1) == 1 or W == 1, "an (H, W) map has unit stride inside a row"
        row_bytes = W
    pitch = int(map.stride(0)) if H > 1 else row_bytes
    assert pitch >= row_bytes, "rows overlap"
    if rows_per_band is None:
        rows_per_band = png_rows_per_band(H, row_bytes)
    bound, ws = png_deflate_sizes(H, row_bytes, int(rows_per_band))
    if out is None:
        out = torch.empty(bound, dtype=torch.uint8, device=map.device)
    if workspace is None:
        workspace = torch.empty(ws, dtype=torch.uint8, device=map.device)
    if out_bytes is None:
        out_bytes = torch.empty(1, dtype=torch.int64, device=map.device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and workspace.dtype == torch.uint8 and workspace.is_contiguous()
    assert out_bytes.dtype == torch.int64 and out_bytes.numel() == 1
    call("fs_png_deflate", _stream(), _p(map), H, row_bytes, pitch, int(rows_per_band), _p(out), out.numel(), _p(out_bytes), _p(workspace),
         workspace.numel())
    return out, out_bytes


def deterministic_on():
    """Is the library in its bit-reproducible mode (fs_set_deterministic / FS_DETERMINISTIC=1)?"""
    return bool(_lib.lib().fs_get_deterministic())


class deterministic:
    """with deterministic(): ...  -  bit-reproducible mode of the library for the duration (fs_set_deterministic): ordered partial sums
    instead of float atomics in the weight-gradient slabs and the BatchNorm reductions of large maps (slower, see the header)."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        from . import _lib
        self.prev = _lib.lib().fs_get_deterministic()
        _lib.lib().fs_set_deterministic(int(self.on))
        return self

    def __exit__(self, *exc):
        from . import _lib
        _lib.lib().fs_set_deterministic(self.prev)
