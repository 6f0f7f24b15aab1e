// Per-pixel confidence next to the class map (gfx950): the share of the winning class in the evaluator's exp-score, one byte per pixel.
//
//   fs_bilinear_argmax_conf   fs_bilinear_argmax (eval.hip) that keeps one more byte: the up-sampled class values of a pixel are all in
//                             registers when its class index is written, so conf = 1 / sum_{c<C} exp(v_c - v_max) - the softmax
//                             probability of the arg-max class - costs C exponentials and no memory traffic beyond its own byte.
//   fs_score_confidence       the same decision on an fp32 score buffer (pixels, cs) of summed exp-scores (the evaluator's canvas /
//                             total of the flip, padded and multi-scale modes): class = first maximum, conf = max / sum.
// Both store q = floor(255 conf + 0.5) and, in the class map, `ignore_label` where q < min_conf.
//   fs_bilinear_argmax_conf_pc / fs_score_confidence_pc   the same kernels (one body, the threshold's type is the template policy) with one
//                             threshold per class: a pixel of arg-max class k is kept iff q >= min_conf_by_class[k], a 256-byte device
//                             table read at run time - one byte load per pixel through L1; the strip kernel issues it as soon as the
//                             class is known, under the exponentials - so a captured launch follows later writes to the table.
//                             Entries >= C are never indexed: arg < C always.
//   fs_confidence_hist        uint64 hist[2][C][256] of (predicted class, confidence byte), split by right / wrong against labels: what
//                             the per-class thresholds are chosen from (fasterseg_amd/calibration.py).  Integer atomics only.
//
// The up-sample is eval.hip's to the bit: the same make_tap / bilerp expression (common.h) and the same strict compare, so with
// min_conf == 0 the class map is the one fs_bilinear_argmax writes.  Operation order of the confidence, all fp32:
//   a_c = v_c - v_max          (one rounding; a_max == 0 exactly, so its term is exactly 1 and sum >= 1)
//   e_c = v_exp_f32(a_c * log2 e)   (one rounding of the product, the hardware exponential: 1 ulp)
//   s   = e_0 + e_1 + ... over c < C in index order (pad lanes never enter), conf = v_rcp_f32(s), q = (int)fma(255, conf, 0.5)
// No atomics, plain vector stores, wave64 blocks of 256.
#include "common.h"

namespace fs {

template <typename T> struct ConfQuad;
template <> struct ConfQuad<float> {
    static __device__ __forceinline__ void load(const float* p, float* o) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3];
    }
};
template <> struct ConfQuad<bf16_t> {
    static __device__ __forceinline__ void load(const bf16_t* p, float* o) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
        o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
    }
};
template <> struct ConfQuad<f16_t> {
    static __device__ __forceinline__ void load(const f16_t* p, float* o) { f16_load4(p, o); }
};

constexpr float LOG2E = 1.4426950408889634f;

// exp(v - best) for v <= best: the subtraction, the log2 e product, v_exp_f32
__device__ __forceinline__ float exp_below(float v, float best) { return __builtin_amdgcn_exp2f((v - best) * LOG2E); }

// conf in [0, 1] -> the stored byte; a NaN (NaN logits) is stored as 0
__device__ __forceinline__ uint32_t conf_byte(float conf) {
    const float t = __builtin_fmaf(255.f, conf, 0.5f);
    return (uint32_t)(int)fminf(fmaxf(t, 0.f), 255.f);
}

// the threshold of a pixel whose arg-max is class k: the scalar forms pass the int, the _pc forms the 256-byte device table
__device__ __forceinline__ int min_conf_of(int min_conf, int) { return min_conf; }
__device__ __forceinline__ int min_conf_of(const unsigned char* by_class, int k) { return by_class[k]; }

// one lane: 4 consecutive output columns of one output row.  Two passes over the classes: the arg-max of bilinear_argmax_kernel, then the
// same values again (same loads, same expression, same bits) for the sum - C may be 256, the values cannot stay in registers.
template <typename T, typename TH>
__global__ __launch_bounds__(256) void bilinear_argmax_conf_kernel(int N, int Hi, int Wi, int Ho, int Wo, int C, float rh, float rw,
                                                                   const T* __restrict__ x, int x_cs, unsigned char* __restrict__ y,
                                                                   unsigned char* __restrict__ conf, TH min_conf, int ignore_label) {
    const int wq = Wo >> 2;
    const long long total = (long long)N * Ho * wq;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int ow0 = (int)(t % wq) * 4; t /= wq;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const Tap th = make_tap(rh, oh, Hi);
        const T* r0 = x + ((long long)n * Hi + th.i0) * Wi * x_cs;
        const T* r1 = x + ((long long)n * Hi + th.i1) * Wi * x_cs;
        Tap tw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) tw[q] = make_tap(rw, ow0 + q, Wi);
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        float sum[4] = {0.f, 0.f, 0.f, 0.f};
        int arg[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            for (int c0 = 0; c0 < C; c0 += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float p00[4], p01[4], p10[4], p11[4];
                    ConfQuad<T>::load(r0 + (long long)tw[q].i0 * x_cs + c0, p00);
                    ConfQuad<T>::load(r0 + (long long)tw[q].i1 * x_cs + c0, p01);
                    ConfQuad<T>::load(r1 + (long long)tw[q].i0 * x_cs + c0, p10);
                    ConfQuad<T>::load(r1 + (long long)tw[q].i1 * x_cs + c0, p11);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float v = bilerp(th, tw[q], p00[k], p01[k], p10[k], p11[k]);
                        if (pass == 0) {
                            if (c0 + k < C && v > best[q]) {       // strict: the first maximum wins (np.argmax)
                                best[q] = v;
                                arg[q] = c0 + k;
                            }
                        } else if (c0 + k < C) {
                            sum[q] += exp_below(v, best[q]);
                        }
                    }
                }
            }
        }
        uint32_t cls = 0, cq = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t b = conf_byte(__builtin_amdgcn_rcpf(sum[q]));
            cq |= b << (8 * q);
            cls |= (uint32_t)((int)b >= min_conf_of(min_conf, arg[q]) ? arg[q] : ignore_label) << (8 * q);
        }
        const long long o = ((long long)n * Ho + oh) * Wo + ow0;
        if (y) *reinterpret_cast<uint32_t*>(y + o) = cls;
        if (conf) *reinterpret_cast<uint32_t*>(conf + o) = cq;
    }
}

// x8 case, bilinear_argmax8_kernel's 1 x 8 strip: the 2 rows x 3 columns x 20 channels are loaded once, each of the 8 pixels keeps its
// 20 up-sampled values in registers for the sum.
template <typename T, int CQ, typename TH>       // CQ = ceil(C / 4) <= 5
__global__ __launch_bounds__(256) void bilinear_argmax_conf8_kernel(int N, int Hi, int Wi, int Ho, int Wo, int C, float rh, float rw,
                                                                    const T* __restrict__ x, int x_cs, unsigned char* __restrict__ y,
                                                                    unsigned char* __restrict__ conf, TH min_conf, int ignore_label) {
    const int w8 = Wo >> 3;
    const long long total = (long long)N * Ho * w8;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int ow0 = (int)(t % w8) * 8; t /= w8;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const Tap th = make_tap(rh, oh, Hi);
        const int bx = make_tap(rw, ow0, Wi).i0;
        const T* r0 = x + ((long long)n * Hi + th.i0) * Wi * x_cs;
        const T* r1 = x + ((long long)n * Hi + th.i1) * Wi * x_cs;
        float top[3][CQ * 4], bot[3][CQ * 4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int col = min(bx + k, Wi - 1);
#pragma unroll
            for (int q = 0; q < CQ; ++q) {
                ConfQuad<T>::load(r0 + (long long)col * x_cs + q * 4, &top[k][q * 4]);
                ConfQuad<T>::load(r1 + (long long)col * x_cs + q * 4, &bot[k][q * 4]);
            }
        }
        unsigned long long cls8 = 0, q8 = 0;
        // the pixel loop stays rolled: unrolled, the 8 pixels' values and exponentials sit beside the 120 staged taps (256 VGPRs, ~280
        // spilled SGPRs, 1 wave / SIMD); rolled it is 161 VGPRs, no spill, 3 waves / SIMD
#pragma unroll 1
        for (int dx = 0; dx < 8; ++dx) {
            const Tap tw = make_tap(rw, ow0 + dx, Wi);
            const bool a1 = (tw.i0 - bx) >= 1;              // left tap is source column bx + 1 (else bx)
            const int rel1 = tw.i1 - bx;                    // right tap: bx, bx + 1 or bx + 2
            float val[CQ * 4];
            float best = -INFINITY;
            int arg = 0;
#pragma unroll
            for (int c = 0; c < CQ * 4; ++c) {
                const float p00 = a1 ? top[1][c] : top[0][c];
                const float p10 = a1 ? bot[1][c] : bot[0][c];
                const float p01 = rel1 >= 2 ? top[2][c] : (rel1 == 1 ? top[1][c] : top[0][c]);
                const float p11 = rel1 >= 2 ? bot[2][c] : (rel1 == 1 ? bot[1][c] : bot[0][c]);
                // a pad lane becomes -inf: it never wins the strict compare and its term below is exp2(-inf) = +0, which leaves the sum's bits
                val[c] = c < C ? bilerp(th, tw, p00, p01, p10, p11) : -INFINITY;
                if (val[c] > best) {
                    best = val[c];
                    arg = c;
                }
            }
            // the table form's byte load is issued here, as soon as the class is known: the 20 exponentials below cover its latency
            const int th = min_conf_of(min_conf, arg);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < CQ * 4; ++c) sum += exp_below(val[c], best);
            const uint32_t b = conf_byte(__builtin_amdgcn_rcpf(sum));
            const uint32_t cls = (uint32_t)((int)b >= th ? arg : ignore_label);
            cls8 |= (unsigned long long)cls << (8 * dx);
            q8 |= (unsigned long long)b << (8 * dx);
        }
        const long long o = ((long long)n * Ho + oh) * Wo + ow0;
        if (y) *reinterpret_cast<unsigned long long*>(y + o) = cls8;
        if (conf) *reinterpret_cast<unsigned long long*>(conf + o) = q8;
    }
}

// one lane: one pixel of an fp32 score buffer, its classes 4 at a time
template <typename TH>
__global__ __launch_bounds__(256) void score_confidence_kernel(const float* __restrict__ score, long long pixels, int cs, int C,
                                                               unsigned char* __restrict__ classes, unsigned char* __restrict__ conf,
                                                               TH min_conf, int ignore_label) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < pixels; idx += (long long)gridDim.x * blockDim.x) {
        const float* s = score + idx * cs;
        float best = -INFINITY, sum = 0.f;
        int arg = 0;
        for (int c0 = 0; c0 < C; c0 += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(s + c0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < C) {
                    sum += v[k];
                    if (v[k] > best) {                     // strict: the first maximum wins, as fs_eval_rescale_accumulate
                        best = v[k];
                        arg = c0 + k;
                    }
                }
        }
        const bool usable = sum > 0.f && sum <= 3.402823466e+38f;          // a zero, infinite or NaN sum: q = 0
        const uint32_t b = usable ? conf_byte(best / sum) : 0u;
        if (classes) classes[idx] = (unsigned char)((int)b >= min_conf_of(min_conf, arg) ? arg : ignore_label);
        if (conf) conf[idx] = (unsigned char)b;
    }
}

// hist[plane][k][q] over the pixels of one launch segment; plane = 0 without labels, else 0 where k == gt and 1 where k != gt; pixels with
// k >= C or a label outside [0, C) are skipped.  Counters are privatised per block in LDS (uint32; the host bounds a launch to HIST_SEGMENT
// pixels, so none can wrap) and the non-zero ones flushed with 64-bit global atomics, as hist_info_kernel (eval.hip) does.
// Contention: a class map's neighbours share their key (road / building / sky at byte 255 on a real frame), and one LDS atomic per pixel
// would serialise on a handful of addresses.  A lane therefore takes runs of HIST_RUN consecutive pixels (one 16-byte load per map) and
// keeps (key, count) of its current run of equal keys in registers, across its grid-stride steps too: an atomic is issued only when the key
// changes, and once at the end.  A one-bin input costs one LDS atomic per lane for the whole launch.
constexpr int HIST_RUN = 16;
constexpr long long HIST_SEGMENT = 1ll << 30;

template <typename G, bool LABELLED>
__global__ __launch_bounds__(256) void confidence_hist_kernel(const unsigned char* __restrict__ classes, const unsigned char* __restrict__ conf,
                                                              const G* __restrict__ gt, long long n, int head, int C,
                                                              unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned int local[];            // (LABELLED ? 2 : 1) * C * 256
    const int plane = C * 256;
    const int bins = (LABELLED ? 2 : 1) * plane;
    for (int i = threadIdx.x; i < bins; i += blockDim.x) local[i] = 0;
    __syncthreads();
    int cur = -1;                                      // the key of the lane's current run (-1: skipped pixels) and its length
    unsigned int cnt = 0;
    auto put = [&](int k, int q, long long g) {
        int key = -1;
        if (k < C) {
            if (!LABELLED) key = k * 256 + q;
            else if (g >= 0 && g < C) key = (k != (int)g ? plane : 0) + k * 256 + q;
        }
        if (key == cur) {
            ++cnt;
        } else {
            if (cur >= 0) atomicAdd(&local[cur], cnt);
            cur = key;
            cnt = 1;
        }
    };
    // [0, head): the pixels before the class map's first 16-byte boundary; [head + 16 chunks, n): the rest of the last run.  At most 15 each,
    // one per lane of block 0.
    const long long chunks = (n - head) / HIST_RUN;
    const long long tail0 = head + chunks * HIST_RUN;
    if (blockIdx.x == 0) {
        const long long t = threadIdx.x;
        if (t < head) put(classes[t], conf[t], LABELLED ? (long long)gt[t] : 0);
        if (tail0 + t < n) put(classes[tail0 + t], conf[tail0 + t], LABELLED ? (long long)gt[tail0 + t] : 0);
    }
    for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < chunks; c += (long long)gridDim.x * blockDim.x) {
        const long long base = head + c * HIST_RUN;
        const uint4 kv = *reinterpret_cast<const uint4*>(classes + base);      // aligned: that is what `head` is for
        uint4 qv;                                                              // conf and gt need not share that alignment
        __builtin_memcpy(&qv, conf + base, sizeof(qv));
        G gv[LABELLED ? HIST_RUN : 1];
        if (LABELLED) __builtin_memcpy(gv, gt + base, sizeof(gv));
        const uint32_t kw[4] = {kv.x, kv.y, kv.z, kv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int j = 0; j < HIST_RUN; ++j)
            put((int)((kw[j >> 2] >> (8 * (j & 3))) & 255u), (int)((qw[j >> 2] >> (8 * (j & 3))) & 255u), LABELLED ? (long long)gv[j] : 0);
    }
    if (cur >= 0) atomicAdd(&local[cur], cnt);
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += blockDim.x)
        if (local[i]) atomicAdd(&hist[i], (unsigned long long)local[i]);
}

}  // namespace fs

using namespace fs;

static inline bool conf_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// the scalar and the per-class form of an entry point share everything but the threshold: TH = int or the device table
template <typename TH>
static fs_status bilinear_argmax_conf_launch(const char* name, void* stream, const fs_resize_desc* d, const void* x, unsigned char* classes,
                                             unsigned char* conf, TH min_conf, int ignore_label) {
    FS_REQUIRE(d->N > 0 && d->Hi > 0 && d->Wi > 0 && d->Ho > 0 && d->Wo > 0 && d->C > 0 && d->C <= 256, FS_ERR_INVALID,
               "%s: bad dimension (C must be in 1..256 for a uint8 class map)", name);
    FS_REQUIRE(dtype_ok(d->dtype), FS_ERR_INVALID, "%s: bad dtype", name);
    FS_REQUIRE(d->x_cs >= ((d->C + 3) / 4) * 4 && d->x_cs % 4 == 0, FS_ERR_INVALID,
               "%s: the logits' channel stride must be padded to a multiple of 4 (got %d for C=%d)", name, d->x_cs, d->C);
    FS_REQUIRE(d->Wo % 4 == 0, FS_ERR_UNSUPPORTED, "%s: output width %d must be a multiple of 4", name, d->Wo);
    FS_REQUIRE(ignore_label >= 0 && ignore_label <= 255, FS_ERR_INVALID, "%s: ignore_label %d outside 0..255", name, ignore_label);
    FS_REQUIRE(conf_aligned(x, 4 * (uintptr_t)elem_size(d->dtype)) && conf_aligned(classes, 4) && conf_aligned(conf, 4), FS_ERR_INVALID,
               "%s: misaligned operand", name);
    const float rh = d->Ho > 1 ? (float)(d->Hi - 1) / (float)(d->Ho - 1) : 0.f;
    const float rw = d->Wo > 1 ? (float)(d->Wi - 1) / (float)(d->Wo - 1) : 0.f;
    hipStream_t st = (hipStream_t)stream;
    const double out_bytes = (double)d->N * d->Ho * d->Wo * ((classes ? 1 : 0) + (conf ? 1 : 0));
    FS_NOTE_BYTES((double)d->N * d->Hi * d->Wi * d->C * elem_size(d->dtype) + out_bytes);
    // the x8 logits up-sample, under fs_bilinear_argmax's conditions: the kernel loads 20 channels of every source pixel
    if (d->Wo == 8 * d->Wi && d->Wi >= 2 && d->C <= 20 && d->x_cs >= 20 && conf_aligned(classes, 8) && conf_aligned(conf, 8)) {
        const long long total8 = (long long)d->N * d->Ho * (d->Wo / 8);
        long long g8 = (total8 + 255) / 256;
        if (g8 > 16384) g8 = 16384;
        FS_DTYPE_SWITCH(d->dtype, T, FS_LAUNCH((bilinear_argmax_conf8_kernel<T, 5, TH>), dim3((unsigned)g8), dim3(256), 0, st, d->N, d->Hi,
                                               d->Wi, d->Ho, d->Wo, d->C, rh, rw, (const T*)x, d->x_cs, classes, conf, min_conf, ignore_label));
        return check_launch(name);
    }
    const long long total = (long long)d->N * d->Ho * (d->Wo / 4);
    long long g = (total + 255) / 256;
    if (g > 16384) g = 16384;
    FS_DTYPE_SWITCH(d->dtype, T, FS_LAUNCH((bilinear_argmax_conf_kernel<T, TH>), dim3((unsigned)g), dim3(256), 0, st, d->N, d->Hi, d->Wi, d->Ho,
                                           d->Wo, d->C, rh, rw, (const T*)x, d->x_cs, classes, conf, min_conf, ignore_label));
    return check_launch(name);
}

extern "C" fs_status fs_bilinear_argmax_conf(void* stream, const fs_resize_desc* d, const void* x, unsigned char* classes,
                                             unsigned char* conf, int min_conf, int ignore_label) {
    FS_REQUIRE(d && x, FS_ERR_INVALID, "fs_bilinear_argmax_conf: null argument");
    FS_REQUIRE(classes || conf, FS_ERR_INVALID, "fs_bilinear_argmax_conf: null argument (neither a class map nor a confidence map)");
    FS_REQUIRE(min_conf >= 0 && min_conf <= 255, FS_ERR_INVALID, "fs_bilinear_argmax_conf: min_conf %d outside 0..255", min_conf);
    return bilinear_argmax_conf_launch<int>("fs_bilinear_argmax_conf", stream, d, x, classes, conf, min_conf, ignore_label);
}

extern "C" fs_status fs_bilinear_argmax_conf_pc(void* stream, const fs_resize_desc* d, const void* x, unsigned char* classes,
                                                unsigned char* conf, const unsigned char* min_conf_by_class, int ignore_label) {
    FS_REQUIRE(d && x, FS_ERR_INVALID, "fs_bilinear_argmax_conf_pc: null argument");
    FS_REQUIRE(classes || conf, FS_ERR_INVALID, "fs_bilinear_argmax_conf_pc: null argument (neither a class map nor a confidence map)");
    FS_REQUIRE(min_conf_by_class, FS_ERR_INVALID, "fs_bilinear_argmax_conf_pc: null min_conf_by_class table (256 device bytes)");
    return bilinear_argmax_conf_launch<const unsigned char*>("fs_bilinear_argmax_conf_pc", stream, d, x, classes, conf, min_conf_by_class,
                                                             ignore_label);
}

template <typename TH>
static fs_status score_confidence_launch(const char* name, void* stream, const float* score, long long pixels, int cs, int C,
                                         unsigned char* classes, unsigned char* conf, TH min_conf, int ignore_label) {
    FS_REQUIRE(pixels >= 0, FS_ERR_INVALID, "%s: pixels %lld is negative", name, pixels);
    FS_REQUIRE(cs > 0 && cs % 4 == 0, FS_ERR_INVALID, "%s: channel stride %d must be a positive multiple of 4", name, cs);
    FS_REQUIRE(C >= 1 && C <= cs, FS_ERR_INVALID, "%s: C=%d outside 1..cs=%d", name, C, cs);
    FS_REQUIRE(C <= 256, FS_ERR_UNSUPPORTED, "%s: C=%d classes do not fit a uint8 class map", name, C);
    FS_REQUIRE(ignore_label >= 0 && ignore_label <= 255, FS_ERR_INVALID, "%s: ignore_label %d outside 0..255", name, ignore_label);
    FS_REQUIRE(conf_aligned(score, 16), FS_ERR_INVALID, "%s: misaligned score buffer", name);
    if (pixels == 0) return FS_OK;
    long long g = (pixels + 255) / 256;
    if (g > 16384) g = 16384;
    FS_NOTE_BYTES((double)pixels * ((C + 3) / 4) * 16 + (double)pixels * ((classes ? 1 : 0) + (conf ? 1 : 0)));
    FS_LAUNCH(score_confidence_kernel<TH>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, score, pixels, cs, C, classes, conf, min_conf,
              ignore_label);
    return check_launch(name);
}

extern "C" fs_status fs_score_confidence(void* stream, const float* score, long long pixels, int cs, int C, unsigned char* classes,
                                         unsigned char* conf, int min_conf, int ignore_label) {
    FS_REQUIRE(score, FS_ERR_INVALID, "fs_score_confidence: null argument");
    FS_REQUIRE(classes || conf, FS_ERR_INVALID, "fs_score_confidence: null argument (neither a class map nor a confidence map)");
    FS_REQUIRE(min_conf >= 0 && min_conf <= 255, FS_ERR_INVALID, "fs_score_confidence: min_conf %d outside 0..255", min_conf);
    return score_confidence_launch<int>("fs_score_confidence", stream, score, pixels, cs, C, classes, conf, min_conf, ignore_label);
}

extern "C" fs_status fs_score_confidence_pc(void* stream, const float* score, long long pixels, int cs, int C, unsigned char* classes,
                                            unsigned char* conf, const unsigned char* min_conf_by_class, int ignore_label) {
    FS_REQUIRE(score, FS_ERR_INVALID, "fs_score_confidence_pc: null argument");
    FS_REQUIRE(classes || conf, FS_ERR_INVALID, "fs_score_confidence_pc: null argument (neither a class map nor a confidence map)");
    FS_REQUIRE(min_conf_by_class, FS_ERR_INVALID, "fs_score_confidence_pc: null min_conf_by_class table (256 device bytes)");
    return score_confidence_launch<const unsigned char*>("fs_score_confidence_pc", stream, score, pixels, cs, C, classes, conf,
                                                         min_conf_by_class, ignore_label);
}

template <typename G>
static void confidence_hist_launch(hipStream_t st, const unsigned char* classes, const unsigned char* conf, const G* gt, long long n, int C,
                                   unsigned long long* hist) {
    // a lane takes at least two runs where there are that many, so that a block's flush (one 64-bit atomic per non-zero bin) is paid for
    // by 8192 pixels; at most 1024 blocks
    const int head = (int)((16 - (reinterpret_cast<uintptr_t>(classes) & 15)) & 15);
    const long long chunks = n > head ? (n - head) / HIST_RUN : 0;
    long long g = (chunks + 511) / 512;
    if (g > 1024) g = 1024;
    if (g < 1) g = 1;
    const int h = (int)(n < head ? n : head);
    if (gt) {
        FS_LAUNCH((confidence_hist_kernel<G, true>), dim3((unsigned)g), dim3(256), (size_t)2 * C * 256 * sizeof(unsigned int), st, classes, conf, gt,
                  n, h, C, hist);
    } else {
        FS_LAUNCH((confidence_hist_kernel<unsigned char, false>), dim3((unsigned)g), dim3(256), (size_t)C * 256 * sizeof(unsigned int), st, classes,
                  conf, (const unsigned char*)nullptr, n, h, C, hist);
    }
}

extern "C" fs_status fs_confidence_hist(void* stream, const unsigned char* classes, const unsigned char* conf, const void* gt, int gt_bytes,
                                        long long n, int C, unsigned long long* hist) {
    FS_REQUIRE(n >= 0, FS_ERR_INVALID, "fs_confidence_hist: n %lld is negative", n);
    FS_REQUIRE(hist, FS_ERR_INVALID, "fs_confidence_hist: null hist");
    FS_REQUIRE(C >= 1, FS_ERR_INVALID, "fs_confidence_hist: C=%d is not positive", C);
    FS_REQUIRE(C <= 32, FS_ERR_UNSUPPORTED, "fs_confidence_hist: C=%d not in 1..32 (two planes of 32 x 256 counters fill a block's 64 KB of LDS)", C);
    FS_REQUIRE(!gt || gt_bytes == 1 || gt_bytes == 4 || gt_bytes == 8, FS_ERR_INVALID,
               "fs_confidence_hist: labels must be uint8, int32 or int64 (gt_bytes %d)", gt_bytes);
    FS_REQUIRE(!gt || conf_aligned(gt, (uintptr_t)gt_bytes), FS_ERR_INVALID, "fs_confidence_hist: misaligned labels");
    FS_REQUIRE(conf_aligned(hist, 8), FS_ERR_INVALID, "fs_confidence_hist: misaligned hist");
    if (n == 0) return FS_OK;                              // an empty map contributes nothing (pointers may be null)
    FS_REQUIRE(classes && conf, FS_ERR_INVALID, "fs_confidence_hist: null classes / conf");
    hipStream_t st = (hipStream_t)stream;
    FS_NOTE_BYTES((double)n * (2 + (gt ? gt_bytes : 0)));
    // one launch per HIST_SEGMENT pixels: no block can count past 2^30 in a 32-bit counter, whatever n is
    for (long long off = 0; off < n; off += HIST_SEGMENT) {
        const long long m = n - off < HIST_SEGMENT ? n - off : HIST_SEGMENT;
        if (!gt || gt_bytes == 1)
            confidence_hist_launch<unsigned char>(st, classes + off, conf + off, gt ? (const unsigned char*)gt + off : nullptr, m, C, hist);
        else if (gt_bytes == 4)
            confidence_hist_launch<int>(st, classes + off, conf + off, (const int*)gt + off, m, C, hist);
        else
            confidence_hist_launch<long long>(st, classes + off, conf + off, (const long long*)gt + off, m, C, hist);
    }
    return check_launch("fs_confidence_hist");
}

