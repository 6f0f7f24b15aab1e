// The evaluator's up-sampled class values, written once (gfx950): the align_corners=True bilinear up-sample of padded NHWC logits to
// the class values of one output pixel, or of one 1 x 8 strip at x8, with what the kernels around it share.
//
// The contract.  A class value is bilerp(th, tw, p00, p01, p10, p11) (common.h) of taps th = make_tap(rh, oh, Hi) and
// tw = make_tap(rw, ow, Wi): top = fma(tw.l1, p01, tw.l0 * p00), bot = fma(tw.l1, p11, tw.l0 * p10), v = fma(th.l1, bot, th.l0 * top),
// every fma explicit, so no contraction inside the blend is left to the compiler.  The weights depend on the pixel alone and the
// operation order on nothing, so classes with equal taps get equal bits: an exact tie goes to the lowest class index under the
// consumers' strict `>` (np.argmax).  The strip form reads the same source values as the generic form, from registers instead of
// memory, and blends them with the same expression: both give one pixel the same bits.
// Who relies on it: fs_bilinear_argmax (eval.hip) and fs_heads_confusion (eval_heads.hip: its counts are those of fs_bilinear_argmax +
// fs_hist_info head by head) take their class values from the bodies below.  confidence.hip still carries its own copy of the same
// expressions (with min_conf == 0 its class map is the one fs_bilinear_argmax writes): it must stay equal to these to the bit.
// resize.hip, loss_up.hip and eval_ms.hip take the quad loader only; their blends are deliberately their own.
#pragma once
#include "common.h"

namespace fs {

// four consecutive channels as fp32: one 16-byte (fp32) or 8-byte (bf16, fp16) load
template <typename T> struct Quad;
template <> struct Quad<float> {
    static __device__ __forceinline__ void load(const float* p, float* o) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    }
};
template <> struct Quad<bf16_t> {
    static __device__ __forceinline__ void load(const bf16_t* p, float* o) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
        o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
    }
};
template <> struct Quad<f16_t> {
    static __device__ __forceinline__ void load(const f16_t* p, float* o) { f16_load4(p, o); }
};

// ---- generic geometry: one output pixel, a channel quad at a time ---------------------------------------------------------------
// Staging: the four taps of channels c0 .. c0 + 3 as p[tap][k], tap = 00, 01, 10, 11; r0 / r1 are the source rows th.i0 / th.i1 (pad
// lanes readable).  Value: class c0 + k from them.  The consumer takes the values one by one, as it does in the strip form: handed all
// four at once, bilinear_argmax_kernel<float> compiled to 106 VGPRs instead of 104 and ran 4 % slower.
template <typename T>
__device__ __forceinline__ void quad_stage(const T* r0, const T* r1, int cs, const Tap& tw, int c0, float (&p)[4][4]) {
    Quad<T>::load(r0 + (long long)tw.i0 * cs + c0, p[0]);
    Quad<T>::load(r0 + (long long)tw.i1 * cs + c0, p[1]);
    Quad<T>::load(r1 + (long long)tw.i0 * cs + c0, p[2]);
    Quad<T>::load(r1 + (long long)tw.i1 * cs + c0, p[3]);
}
__device__ __forceinline__ float quad_value(const float (&p)[4][4], const Tap& th, const Tap& tw, int k) {
    return bilerp(th, tw, p[0][k], p[1][k], p[2][k], p[3][k]);
}

// ---- x8 geometry (Wo == 8 * Wi, Wi >= 2): one 1 x 8 output strip --------------------------------------------------------------------
// 8 consecutive output columns span less than one source column step, so their taps come from at most three source columns: the
// 2 rows x 3 columns x CQ * 4 channels are loaded once (30 vector loads at CQ = 5 instead of 160 for the same pixels in the generic
// form) and every column selects its taps from registers.  The channel stride must cover CQ * 4 channels.
template <typename T, int CQ>
__device__ __forceinline__ void strip_stage(const T* __restrict__ x, int cs, int n, int oh, int ow0, int Hi, int Wi, float rh, float rw,
                                            Tap& th, int& bx, float (&top)[3][CQ * 4], float (&bot)[3][CQ * 4]) {
    th = make_tap(rh, oh, Hi);
    bx = make_tap(rw, ow0, Wi).i0;
    const T* r0 = x + ((long long)n * Hi + th.i0) * Wi * cs;
    const T* r1 = x + ((long long)n * Hi + th.i1) * Wi * cs;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int col = min(bx + k, Wi - 1);
#pragma unroll
        for (int q = 0; q < CQ; ++q) {
            Quad<T>::load(r0 + (long long)col * cs + q * 4, &top[k][q * 4]);
            Quad<T>::load(r1 + (long long)col * cs + q * 4, &bot[k][q * 4]);
        }
    }
}

// one output column of a staged strip: its tap and where the tap's two source columns sit among the three staged ones
struct StripCol {
    Tap tw;
    bool a1;                // left tap is source column bx + 1 (else bx)
    int rel1;               // right tap: bx, bx + 1 or bx + 2
};
__device__ __forceinline__ StripCol strip_col(float rw, int ow, int Wi, int bx) {
    StripCol s;
    s.tw = make_tap(rw, ow, Wi);
    s.a1 = (s.tw.i0 - bx) >= 1;
    s.rel1 = s.tw.i1 - bx;
    return s;
}
// class value c of that column
template <int CQ>
__device__ __forceinline__ float strip_value(const float (&top)[3][CQ * 4], const float (&bot)[3][CQ * 4], const Tap& th, const StripCol& s,
                                             int c) {
    const float p00 = s.a1 ? top[1][c] : top[0][c];
    const float p10 = s.a1 ? bot[1][c] : bot[0][c];
    const float p01 = s.rel1 >= 2 ? top[2][c] : (s.rel1 == 1 ? top[1][c] : top[0][c]);
    const float p11 = s.rel1 >= 2 ? bot[2][c] : (s.rel1 == 1 ? bot[1][c] : bot[0][c]);
    return bilerp(th, s.tw, p00, p01, p10, p11);
}

// ---- a block's uint32 counters in LDS, flushed with 64-bit global atomics ---------------------------------------------------------
__device__ __forceinline__ void lds_zero(unsigned int* local, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) local[i] = 0;
    __syncthreads();
}
// after a block barrier the non-zero counters are added: local[0, n) to dst and, where a kernel keeps n2 more behind them, those to dst2
__device__ __forceinline__ void lds_flush(const unsigned int* local, int n, unsigned long long* dst, int n2 = 0,
                                          unsigned long long* dst2 = nullptr) {
    __syncthreads();
    for (int i = threadIdx.x; i < n + n2; i += blockDim.x) {
        const unsigned int v = local[i];
        if (v) atomicAdd(i < n ? dst + i : dst2 + (i - n), (unsigned long long)v);
    }
}

// ---- host: what a bilinear class-map entry point checks and decides (fs_bilinear_argmax; confidence.hip has the same checks) -------
inline bool ptr_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

struct ClassMapLaunch {
    float rh, rw;
    bool strip;             // the x8 strip kernel (CQ = 5: it loads 20 channels of every source pixel), else the generic one
    unsigned grid;          // blocks of 256 lanes: one lane per strip, else per 4 output columns
};
// Validates the descriptor and the operands of `name` and fills `l`.  x must be aligned to x_align bytes; conf is null for the entry
// point without a confidence map (ignore_label is then 0).
static inline fs_status class_map_launch(const char* name, const fs_resize_desc* d, const void* x, uintptr_t x_align,
                                         const unsigned char* classes, const unsigned char* conf, int ignore_label, ClassMapLaunch* l) {
    FS_REQUIRE(d->N > 0 && d->Hi > 0 && d->Wi > 0 && d->Ho > 0 && d->Wo > 0 && d->C > 0 && d->C <= 256, FS_ERR_INVALID,
               "%s: bad dimension (C must be in 1..256 for a uint8 class map)", name);
    FS_REQUIRE(dtype_ok(d->dtype), FS_ERR_INVALID, "%s: bad dtype", name);
    FS_REQUIRE(d->x_cs >= ((d->C + 3) / 4) * 4 && d->x_cs % 4 == 0, FS_ERR_INVALID,
               "%s: the logits' channel stride must be padded to a multiple of 4 (got %d for C=%d)", name, d->x_cs, d->C);
    FS_REQUIRE(d->Wo % 4 == 0, FS_ERR_UNSUPPORTED, "%s: output width %d must be a multiple of 4", name, d->Wo);
    FS_REQUIRE(ignore_label >= 0 && ignore_label <= 255, FS_ERR_INVALID, "%s: ignore_label %d outside 0..255", name, ignore_label);
    FS_REQUIRE(ptr_aligned(x, x_align) && ptr_aligned(classes, 4) && ptr_aligned(conf, 4), FS_ERR_INVALID, "%s: misaligned operand", name);
    l->rh = d->Ho > 1 ? (float)(d->Hi - 1) / (float)(d->Ho - 1) : 0.f;
    l->rw = d->Wo > 1 ? (float)(d->Wi - 1) / (float)(d->Wo - 1) : 0.f;
    l->strip = d->Wo == 8 * d->Wi && d->Wi >= 2 && d->C <= 20 && d->x_cs >= 20 && ptr_aligned(classes, 8) && ptr_aligned(conf, 8);
    const long long lanes = (long long)d->N * d->Ho * (d->Wo / (l->strip ? 8 : 4));
    const long long g = (lanes + 255) / 256;
    l->grid = (unsigned)(g > 16384 ? 16384 : g);
    return FS_OK;
}

}  // namespace fs
