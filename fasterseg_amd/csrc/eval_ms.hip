// Multi-scale / sliding-window / flip evaluation on the device (gfx950).
//
// The reference evaluator does all of this on the host (tools/engine/evaluator.py:228-318): cv2.resize of the uint8 image per
// scale, normalisation and padding in numpy, exp() of every window's score, a float64 accumulator, a 19-channel float cv2.resize
// of each scale's score back to the image size and np.argmax.  Here, around the engine's network passes:
//   fs_eval_window_input        uint8 HWC image -> one network input window (fp32 NCHW, + the mirrored window in batch slot 1):
//                               cv2's fixed-point bilinear resize at scale s, the canvas padding and the normalisation in one
//                               pass; the resized image is never materialised;
//   fs_eval_score_accumulate    the engine's 1/8-resolution NHWC logits -> x8 align_corners=True up-sample (slot 1 read at the
//                               mirrored column) -> exp(l0 + l1) added into (or stored to) an fp32 HWC canvas, or the uint8
//                               arg-max of l0 + l1 for the single-scale flip path;
//   fs_eval_rescale_accumulate  canvas rectangle -> cv2's float INTER_LINEAR resize to (H, W) added into (or stored to) the fp32
//                               total, and on the last scale the uint8 arg-max of the updated total.
// No float atomics: the windows of a scale are issued one after another on one stream, so every canvas pixel is a plain
// read-modify-write and the result is bitwise reproducible.
#include "logits_up.h"

namespace fs {

namespace {

template <typename T> struct LoadQuad {                // logits_up.h's quad as an f32x4
    static __device__ __forceinline__ f32x4 load(const T* p) {
        float t[4];
        Quad<T>::load(p, t);
        return f32x4{t[0], t[1], t[2], t[3]};
    }
};

__device__ __forceinline__ long long grid_stride() { return (long long)gridDim.x * blockDim.x; }

// cv2's 8-bit INTER_LINEAR of one channel from its four taps: horizontal in int32, then the vertical step of OpenCV 4's
// VResizeLinear (INTER_RESIZE_COEF_BITS = 11): (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
__device__ __forceinline__ int resize_u8(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    const int d0 = s00 * a0 + s01 * a1;
    const int d1 = s10 * a0 + s11 * a1;
    const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// cv2 INTER_LINEAR taps for float data: fx = (float)((d + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx, edge clamp with fx = 0
struct FTap {
    int i0, i1;
    float a0, a1;
};
__device__ __forceinline__ FTap cv_tap(double scale, int d, int in_size) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= in_size - 1) { s = in_size - 1; f = 0.f; }
    FTap t;
    t.i0 = s;
    t.i1 = min(s + 1, in_size - 1);
    t.a0 = 1.f - f;
    t.a1 = f;
    return t;
}

}  // namespace

// one lane: 4 consecutive columns of one window row, 3 channels -> 3 float4 stores per batch slot
__global__ __launch_bounds__(256) void eval_window_input_kernel(fs_eval_window_desc d, const unsigned char* __restrict__ img,
                                                                const int2* __restrict__ ytab, const int2* __restrict__ xtab,
                                                                float* __restrict__ out) {
    const int wq = d.crop_w >> 2;
    const long long total = (long long)d.crop_h * wq;
    const long long plane = (long long)d.crop_h * d.crop_w;
    float pad[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) pad[c] = d.pad_mode == 0 ? (0.f / 255.f - d.mean[c]) / d.std[c] : 0.f;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += grid_stride()) {
        const int wx0 = (int)(idx % wq) * 4;
        const int wy = (int)(idx / wq);
        const int ry = d.oy + wy - d.top;                  // row of the resized image; outside [0, rows): padding
        float v[3][4];
        if (ry < 0 || ry >= d.rows) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][q] = pad[c];
        } else {
            const int2 ty = ytab[ry];
            const int sy0 = min(max(ty.x, 0), d.H - 1);
            const int sy1 = min(sy0 + 1, d.H - 1);
            const int b0 = ty.y & 0xffff, b1 = (ty.y >> 16) & 0xffff;
            const unsigned char* r0 = img + (long long)sy0 * d.W * 3;
            const unsigned char* r1 = img + (long long)sy1 * d.W * 3;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rx = d.ox + wx0 + q - d.left;
                if (rx < 0 || rx >= d.cols) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][q] = pad[c];
                    continue;
                }
                const int2 tx = xtab[rx];
                const int sx0 = min(max(tx.x, 0), d.W - 1);
                const int sx1 = min(sx0 + 1, d.W - 1);
                const int a0 = tx.y & 0xffff, a1 = (tx.y >> 16) & 0xffff;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int u = resize_u8(r0[sx0 * 3 + c], r0[sx1 * 3 + c], r1[sx0 * 3 + c], r1[sx1 * 3 + c], a0, a1, b0, b1);
                    v[c][q] = ((float)u / 255.f - d.mean[c]) / d.std[c];   // SegEvaluator.process_image, IEEE division
                }
            }
        }
        float* o = out + (long long)wy * d.crop_w + wx0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4 s;
            s[0] = v[c][0]; s[1] = v[c][1]; s[2] = v[c][2]; s[3] = v[c][3];
            *reinterpret_cast<f32x4*>(o + c * plane) = s;
        }
        if (d.flip) {                                      // slot 1: the window mirrored, x -> crop_w - 1 - x
            float* m = out + 3 * plane + (long long)wy * d.crop_w + (d.crop_w - 4 - wx0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 s;
                s[0] = v[c][3]; s[1] = v[c][2]; s[2] = v[c][1]; s[3] = v[c][0];
                *reinterpret_cast<f32x4*>(m + c * plane) = s;
            }
        }
    }
}

struct ScoreArgs {
    int h, w, C, cs, Wo, flip;
    float rh, rw;
    int y0, x0, rows, cols;
    int canvas_w, canvas_cs, cy, cx, store;
};

// one lane: one pixel of the window rectangle, all classes 4 at a time.  The up-sample is fs_bilinear_argmax's (make_tap, same
// expression); slot 1 is evaluated at the mirrored column, i.e. score_flip.flip(-1) of evaluator.py:313-315.
template <typename T, bool ARGMAX>
__global__ __launch_bounds__(256) void eval_score_kernel(ScoreArgs a, const T* __restrict__ x, float* __restrict__ canvas,
                                                         unsigned char* __restrict__ classes) {
    const long long total = (long long)a.rows * a.cols;
    const long long slot = (long long)a.h * a.w * a.cs;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += grid_stride()) {
        const int cc = (int)(idx % a.cols);
        const int rr = (int)(idx / a.cols);
        const int ox = a.x0 + cc;
        const Tap th = make_tap(a.rh, a.y0 + rr, a.h);
        const Tap tw = make_tap(a.rw, ox, a.w);
        const Tap tm = make_tap(a.rw, a.Wo - 1 - ox, a.w);
        const T* r0 = x + (long long)th.i0 * a.w * a.cs;
        const T* r1 = x + (long long)th.i1 * a.w * a.cs;
        float best = -INFINITY;
        int arg = 0;
        for (int c0 = 0; c0 < a.C; c0 += 4) {
            const f32x4 p00 = LoadQuad<T>::load(r0 + (long long)tw.i0 * a.cs + c0), p01 = LoadQuad<T>::load(r0 + (long long)tw.i1 * a.cs + c0);
            const f32x4 p10 = LoadQuad<T>::load(r1 + (long long)tw.i0 * a.cs + c0), p11 = LoadQuad<T>::load(r1 + (long long)tw.i1 * a.cs + c0);
            f32x4 l;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                l[k] = th.l0 * (tw.l0 * p00[k] + tw.l1 * p01[k]) + th.l1 * (tw.l0 * p10[k] + tw.l1 * p11[k]);
            if (a.flip) {
                const T* m0 = r0 + slot;
                const T* m1 = r1 + slot;
                const f32x4 q00 = LoadQuad<T>::load(m0 + (long long)tm.i0 * a.cs + c0), q01 = LoadQuad<T>::load(m0 + (long long)tm.i1 * a.cs + c0);
                const f32x4 q10 = LoadQuad<T>::load(m1 + (long long)tm.i0 * a.cs + c0), q11 = LoadQuad<T>::load(m1 + (long long)tm.i1 * a.cs + c0);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    l[k] += th.l0 * (tm.l0 * q00[k] + tm.l1 * q01[k]) + th.l1 * (tm.l0 * q10[k] + tm.l1 * q11[k]);
            }
            if constexpr (ARGMAX) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < a.C && l[k] > best) {     // strict: the first maximum wins (np.argmax)
                        best = l[k];
                        arg = c0 + k;
                    }
            } else {
                float* cv = canvas + ((long long)(a.cy + rr) * a.canvas_w + (a.cx + cc)) * a.canvas_cs + c0;
                f32x4 e;
#pragma unroll
                for (int k = 0; k < 4; ++k) e[k] = c0 + k < a.C ? expf(l[k]) : 0.f;
                if (!a.store) e += *reinterpret_cast<const f32x4*>(cv);
                *reinterpret_cast<f32x4*>(cv) = e;
            }
        }
        if constexpr (ARGMAX) classes[idx] = (unsigned char)arg;
    }
}

struct RescaleArgs {
    int canvas_w, cs, C, y0, x0, rows, cols, H, W, store;
    double scale_y, scale_x;            // cv2's 1 / (dsize / ssize)
};

// one lane: one output pixel, all channels 4 at a time: total (+)= resize(canvas rectangle); optional arg-max of the new total
__global__ __launch_bounds__(256) void eval_rescale_kernel(RescaleArgs a, const float* __restrict__ canvas, float* __restrict__ total,
                                                           unsigned char* __restrict__ classes) {
    const long long n = (long long)a.H * a.W;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += grid_stride()) {
        const int ox = (int)(idx % a.W);
        const int oy = (int)(idx / a.W);
        const FTap ty = cv_tap(a.scale_y, oy, a.rows);
        const FTap tx = cv_tap(a.scale_x, ox, a.cols);
        const float* r0 = canvas + ((long long)(a.y0 + ty.i0) * a.canvas_w + a.x0) * a.cs;
        const float* r1 = canvas + ((long long)(a.y0 + ty.i1) * a.canvas_w + a.x0) * a.cs;
        float* t = total + idx * a.cs;
        float best = -INFINITY;
        int arg = 0;
        for (int c0 = 0; c0 < a.cs; c0 += 4) {
            const f32x4 s00 = *reinterpret_cast<const f32x4*>(r0 + (long long)tx.i0 * a.cs + c0);
            const f32x4 s01 = *reinterpret_cast<const f32x4*>(r0 + (long long)tx.i1 * a.cs + c0);
            const f32x4 s10 = *reinterpret_cast<const f32x4*>(r1 + (long long)tx.i0 * a.cs + c0);
            const f32x4 s11 = *reinterpret_cast<const f32x4*>(r1 + (long long)tx.i1 * a.cs + c0);
            f32x4 v;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d0 = s00[k] * tx.a0 + s01[k] * tx.a1;    // horizontal, then vertical (cv2 resizeGeneric_)
                const float d1 = s10[k] * tx.a0 + s11[k] * tx.a1;
                v[k] = d0 * ty.a0 + d1 * ty.a1;
            }
            if (!a.store) v += *reinterpret_cast<const f32x4*>(t + c0);
            *reinterpret_cast<f32x4*>(t + c0) = v;
            if (classes) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < a.C && v[k] > best) {     // strict: the first maximum wins (np.argmax)
                        best = v[k];
                        arg = c0 + k;
                    }
            }
        }
        if (classes) classes[idx] = (unsigned char)arg;
    }
}

}  // namespace fs

using namespace fs;

static inline bool aligned(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

static inline unsigned grid_for(long long total) {
    long long g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    if (g < 1) g = 1;
    return (unsigned)g;
}

extern "C" fs_status fs_eval_window_input(void* stream, const fs_eval_window_desc* d, const unsigned char* img, const int* ytab,
                                          const int* xtab, float* input) {
    FS_REQUIRE(d && img && ytab && xtab && input, FS_ERR_INVALID, "fs_eval_window_input: null argument");
    FS_REQUIRE(d->H > 0 && d->W > 0 && d->rows > 0 && d->cols > 0 && d->crop_h > 0 && d->crop_w > 0, FS_ERR_INVALID,
               "fs_eval_window_input: bad dimension (image %dx%d, resized %dx%d, window %dx%d)", d->H, d->W, d->rows, d->cols,
               d->crop_h, d->crop_w);
    FS_REQUIRE(d->crop_w % 4 == 0, FS_ERR_UNSUPPORTED, "fs_eval_window_input: window width %d must be a multiple of 4", d->crop_w);
    FS_REQUIRE(d->pad_mode == 0 || d->pad_mode == 1, FS_ERR_INVALID, "fs_eval_window_input: pad_mode must be 0 or 1");
    FS_REQUIRE(d->flip == 0 || d->flip == 1, FS_ERR_INVALID, "fs_eval_window_input: flip must be 0 or 1");
    FS_REQUIRE(d->std[0] != 0.f && d->std[1] != 0.f && d->std[2] != 0.f, FS_ERR_INVALID, "fs_eval_window_input: zero std");
    FS_REQUIRE(aligned(input, 16) && aligned(ytab, 8) && aligned(xtab, 8), FS_ERR_INVALID, "fs_eval_window_input: misaligned operand");
    const long long total = (long long)d->crop_h * (d->crop_w / 4);
    FS_NOTE_BYTES((double)d->crop_h * d->crop_w * 3 * 4 * (1 + d->flip) + (double)d->rows * d->cols * 3);
    FS_LAUNCH(eval_window_input_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, *d, img,
              reinterpret_cast<const int2*>(ytab), reinterpret_cast<const int2*>(xtab), input);
    return check_launch("fs_eval_window_input");
}

extern "C" fs_status fs_eval_score_accumulate(void* stream, const fs_logits_desc* d, const void* logits, int flip, int y0, int x0,
                                              int rows, int cols, float* canvas, int canvas_h, int canvas_w, int canvas_cs, int cy,
                                              int cx, int store, unsigned char* classes) {
    FS_REQUIRE(d && logits, FS_ERR_INVALID, "fs_eval_score_accumulate: null argument");
    FS_REQUIRE(flip == 0 || flip == 1, FS_ERR_INVALID, "fs_eval_score_accumulate: flip must be 0 or 1");
    FS_REQUIRE(d->N >= 1 + flip && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0 && d->C > 0, FS_ERR_INVALID,
               "fs_eval_score_accumulate: bad logits descriptor (N=%d, %dx%d -> %dx%d, C=%d, flip=%d)", d->N, d->h, d->w, d->H, d->W,
               d->C, flip);
    FS_REQUIRE(dtype_ok(d->dtype), FS_ERR_INVALID, "fs_eval_score_accumulate: bad dtype");
    FS_REQUIRE(d->cs % 4 == 0 && d->cs >= ((d->C + 3) / 4) * 4, FS_ERR_INVALID,
               "fs_eval_score_accumulate: the logits' channel stride must be a multiple of 4 covering C (got %d for C=%d)", d->cs, d->C);
    FS_REQUIRE(rows > 0 && cols > 0 && y0 >= 0 && x0 >= 0 && y0 + rows <= d->H && x0 + cols <= d->W, FS_ERR_INVALID,
               "fs_eval_score_accumulate: rectangle (%d, %d) + %dx%d outside the %dx%d window", y0, x0, rows, cols, d->H, d->W);
    FS_REQUIRE(aligned(logits, 4 * elem_size(d->dtype)), FS_ERR_INVALID, "fs_eval_score_accumulate: misaligned logits");
    ScoreArgs a;
    a.h = d->h; a.w = d->w; a.C = d->C; a.cs = d->cs; a.Wo = d->W; a.flip = flip;
    a.rh = d->H > 1 ? (float)(d->h - 1) / (float)(d->H - 1) : 0.f;
    a.rw = d->W > 1 ? (float)(d->w - 1) / (float)(d->W - 1) : 0.f;
    a.y0 = y0; a.x0 = x0; a.rows = rows; a.cols = cols;
    a.canvas_w = canvas_w; a.canvas_cs = canvas_cs; a.cy = cy; a.cx = cx; a.store = store ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned g = grid_for((long long)rows * cols);
    const double logit_bytes = (double)d->h * d->w * d->cs * elem_size(d->dtype) * (1 + flip);
    if (classes) {
        FS_REQUIRE(d->C <= 256, FS_ERR_UNSUPPORTED, "fs_eval_score_accumulate: C=%d classes do not fit a uint8 class map", d->C);
        FS_NOTE_BYTES(logit_bytes + (double)rows * cols);
        FS_DTYPE_SWITCH(d->dtype, T, FS_LAUNCH((eval_score_kernel<T, true>), dim3(g), dim3(256), 0, st, a, (const T*)logits, canvas, classes));
        return check_launch("fs_eval_score_accumulate");
    }
    FS_REQUIRE(canvas, FS_ERR_INVALID, "fs_eval_score_accumulate: neither a canvas nor a class map");
    FS_REQUIRE(canvas_cs % 4 == 0 && canvas_cs >= ((d->C + 3) / 4) * 4, FS_ERR_INVALID,
               "fs_eval_score_accumulate: the canvas channel stride must be a multiple of 4 covering C (got %d for C=%d)", canvas_cs, d->C);
    FS_REQUIRE(cy >= 0 && cx >= 0 && cy + rows <= canvas_h && cx + cols <= canvas_w, FS_ERR_INVALID,
               "fs_eval_score_accumulate: rectangle %dx%d at (%d, %d) outside the %dx%d canvas", rows, cols, cy, cx, canvas_h, canvas_w);
    FS_REQUIRE(aligned(canvas, 16), FS_ERR_INVALID, "fs_eval_score_accumulate: misaligned canvas");
    FS_NOTE_BYTES(logit_bytes + (double)rows * cols * ((d->C + 3) / 4) * 16 * (store ? 1 : 2));
    FS_DTYPE_SWITCH(d->dtype, T, FS_LAUNCH((eval_score_kernel<T, false>), dim3(g), dim3(256), 0, st, a, (const T*)logits, canvas, classes));
    return check_launch("fs_eval_score_accumulate");
}

extern "C" fs_status fs_eval_rescale_accumulate(void* stream, const float* canvas, int canvas_h, int canvas_w, int cs, int C, int y0,
                                                int x0, int rows, int cols, float* total, int H, int W, int store,
                                                unsigned char* classes) {
    FS_REQUIRE(canvas && total, FS_ERR_INVALID, "fs_eval_rescale_accumulate: null argument");
    FS_REQUIRE(C > 0 && cs % 4 == 0 && cs >= ((C + 3) / 4) * 4, FS_ERR_INVALID,
               "fs_eval_rescale_accumulate: channel stride %d must be a multiple of 4 covering C=%d", cs, C);
    FS_REQUIRE(rows > 0 && cols > 0 && H > 0 && W > 0 && y0 >= 0 && x0 >= 0 && y0 + rows <= canvas_h && x0 + cols <= canvas_w,
               FS_ERR_INVALID, "fs_eval_rescale_accumulate: rectangle (%d, %d) + %dx%d outside the %dx%d canvas, or empty output %dx%d",
               y0, x0, rows, cols, canvas_h, canvas_w, H, W);
    FS_REQUIRE(!classes || C <= 256, FS_ERR_UNSUPPORTED, "fs_eval_rescale_accumulate: C=%d classes do not fit a uint8 class map", C);
    FS_REQUIRE(aligned(canvas, 16) && aligned(total, 16), FS_ERR_INVALID, "fs_eval_rescale_accumulate: misaligned operand");
    RescaleArgs a;
    a.canvas_w = canvas_w; a.cs = cs; a.C = C; a.y0 = y0; a.x0 = x0; a.rows = rows; a.cols = cols; a.H = H; a.W = W;
    a.store = store ? 1 : 0;
    a.scale_y = 1.0 / ((double)H / (double)rows);
    a.scale_x = 1.0 / ((double)W / (double)cols);
    const long long n = (long long)H * W;
    FS_NOTE_BYTES((double)rows * cols * cs * 4 + (double)n * cs * 4 * (store ? 1 : 2) + (classes ? (double)n : 0.0));
    FS_LAUNCH(eval_rescale_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a, canvas, total, classes);
    return check_launch("fs_eval_rescale_accumulate");
}
