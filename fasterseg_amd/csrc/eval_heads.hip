// Supernet validation on the device (gfx950): the five heads of one forward -> five confusion histograms in one launch.
//
// The reference validates the supernet with one evaluator sweep per head (search/train_search.py:259-271 infer(): evaluator.out_idx
// = 0..4), and every image of every sweep pays exp() of the up-sampled (19, H, W) score map, its copy to the host, np.argmax and
// hist_info there (tools/engine/evaluator.py:297-318 val_func_process, tools/seg_opr/metric.py:7-17 hist_info).  The five heads
// come out of one forward (model_search.py _tail), so here one forward feeds one launch that, per output pixel and per head,
//   - evaluates the align_corners=True bilinear up-sample of the head's low-resolution NHWC logits (logits_up.h: the class values
//     of eval.hip's kernels, under the bit contract stated there),
//   - takes the arg-max over the C classes (strict >: the first maximum wins, as np.argmax),
//   - counts the pixel into the head's hist[k][C * gt + pred] and counts[k] = {labeled, correct} when 0 <= gt < C
//     (255 / -1 / >= C: ignored), which is what fs_bilinear_argmax + fs_hist_info compute head by head.
// Nothing else is written: blockIdx.y is the head, and each block counts into an LDS histogram of its head (C * C + 2 uint32)
// flushed with one device-scope integer atomicAdd per non-zero bin.  Integer sums do not depend on arrival order: the result is
// bit-exact and reproducible.
#include <algorithm>

#include "logits_up.h"

namespace fs {

// blocks per head at most (grid.x); every block flushes its head's C * C + 2 bins once.  On a 512 x 1024 image 256 gives each lane
// one 8-pixel strip; 64 and 32 (4x and 8x fewer flush atomics, 4 and 8 strips per lane) measured slower.
constexpr int kHeadsBlocks = 256;

struct HeadsArgs {
    const void* p[FS_MAX_HEADS];
    int cs[FS_MAX_HEADS];
};

// head k's pointer / stride with a uniform k: selects instead of a dynamic index into the by-value argument (no scratch copy)
__device__ __forceinline__ const void* head_ptr(const HeadsArgs& a, int k) {
    const void* r = a.p[0];
#pragma unroll
    for (int i = 1; i < FS_MAX_HEADS; ++i) if (k == i) r = a.p[i];
    return r;
}
__device__ __forceinline__ int head_cs(const HeadsArgs& a, int k) {
    int r = a.cs[0];
#pragma unroll
    for (int i = 1; i < FS_MAX_HEADS; ++i) if (k == i) r = a.cs[i];
    return r;
}

// the label of pixel i as a class index, -1 when it is not counted (255, -1, >= C); gt_bytes is uniform
__device__ __forceinline__ int label_at(const void* gt, int gt_bytes, long long i, int C) {
    long long g;
    if (gt_bytes == 1) g = (long long)static_cast<const unsigned char*>(gt)[i];
    else if (gt_bytes == 4) g = (long long)static_cast<const int*>(gt)[i];
    else g = static_cast<const long long*>(gt)[i];
    return (g >= 0 && g < C) ? (int)g : -1;
}

// x8 case (the heads' own up-sample, model_search.py _tail): one lane = one 1 x 8 output strip of one row of head blockIdx.y; the 8
// columns take their taps from at most three source columns, so the head's 2 rows x 3 columns x 4*CQ channels are loaded once.
// Those 24 * CQ values live in registers: CQ <= 5 (C <= 20, the 19 Cityscapes classes) keeps the kernel under 200 VGPRs; wider
// class counts take the generic kernel.
template <typename T, int CQ>       // CQ = ceil(C / 4) <= 5
__global__ __launch_bounds__(256) void heads_confusion8_kernel(HeadsArgs a, int N, int Hi, int Wi, int Ho, int Wo, int C, float rh,
                                                               float rw, const void* __restrict__ gt, int gt_bytes,
                                                               unsigned long long* __restrict__ hist, unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned int local[];
    const int k = blockIdx.y;
    lds_zero(local, C * C + 2);
    const T* x = static_cast<const T*>(head_ptr(a, k));
    const int cs = head_cs(a, k);
    const int w8 = Wo >> 3;
    const long long total = (long long)N * Ho * w8;
    unsigned int labeled = 0, correct = 0;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int ow0 = (int)(t % w8) * 8; t /= w8;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const long long pix = ((long long)n * Ho + oh) * Wo + ow0;
        int lab[8];
        unsigned int nlab = 0;
#pragma unroll
        for (int dx = 0; dx < 8; ++dx) {
            lab[dx] = label_at(gt, gt_bytes, pix + dx, C);
            nlab += lab[dx] >= 0;
        }
        if (nlab == 0) continue;                            // no counted pixel in the strip: nothing to evaluate
        labeled += nlab;
        Tap th;
        int bx;
        float top[3][CQ * 4], bot[3][CQ * 4];
        strip_stage<T, CQ>(x, cs, n, oh, ow0, Hi, Wi, rh, rw, th, bx, top, bot);
#pragma unroll
        for (int dx = 0; dx < 8; ++dx) {
            const StripCol s = strip_col(rw, ow0 + dx, Wi, bx);
            float best = -INFINITY;
            int arg = 0;
#pragma unroll
            for (int c = 0; c < CQ * 4; ++c) {
                const float val = strip_value<CQ>(top, bot, th, s, c);
                if (c < C && val > best) {
                    best = val;
                    arg = c;
                }
            }
            if (lab[dx] >= 0) {
                atomicAdd(&local[lab[dx] * C + arg], 1u);
                correct += (arg == lab[dx]);
            }
        }
    }
    if (labeled) atomicAdd(&local[C * C], labeled);
    if (correct) atomicAdd(&local[C * C + 1], correct);
    // local[j]: j < C * C -> hist[k * C * C + j], j = C * C -> counts[2k] (labeled), C * C + 1 -> counts[2k + 1] (correct)
    lds_flush(local, C * C, hist + (long long)k * (C * C), 2, counts + 2 * k);
}

// any other geometry: one lane = one output pixel of head blockIdx.y, the classes 4 at a time
template <typename T>
__global__ __launch_bounds__(256) void heads_confusion_kernel(HeadsArgs a, int N, int Hi, int Wi, int Ho, int Wo, int C, float rh,
                                                              float rw, const void* __restrict__ gt, int gt_bytes,
                                                              unsigned long long* __restrict__ hist, unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned int local[];
    const int k = blockIdx.y;
    lds_zero(local, C * C + 2);
    const T* x = static_cast<const T*>(head_ptr(a, k));
    const int cs = head_cs(a, k);
    const long long total = (long long)N * Ho * Wo;
    unsigned int labeled = 0, correct = 0;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int g = label_at(gt, gt_bytes, idx, C);
        if (g < 0) continue;
        long long t = idx;
        const int ow = (int)(t % Wo); t /= Wo;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        const Tap th = make_tap(rh, oh, Hi);
        const Tap tw = make_tap(rw, ow, Wi);
        const T* r0 = x + ((long long)n * Hi + th.i0) * Wi * cs;
        const T* r1 = x + ((long long)n * Hi + th.i1) * Wi * cs;
        float best = -INFINITY;
        int arg = 0;
        for (int c0 = 0; c0 < C; c0 += 4) {
            float p[4][4];
            quad_stage(r0, r1, cs, tw, c0, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = quad_value(p, th, tw, j);
                if (c0 + j < C && v > best) {
                    best = v;
                    arg = c0 + j;
                }
            }
        }
        atomicAdd(&local[g * C + arg], 1u);
        labeled += 1;
        correct += (arg == g);
    }
    if (labeled) atomicAdd(&local[C * C], labeled);
    if (correct) atomicAdd(&local[C * C + 1], correct);
    // local[j]: j < C * C -> hist[k * C * C + j], j = C * C -> counts[2k] (labeled), C * C + 1 -> counts[2k + 1] (correct)
    lds_flush(local, C * C, hist + (long long)k * (C * C), 2, counts + 2 * k);
}

template <typename T>
static void launch_strip(int cq, dim3 grid, size_t lds, hipStream_t st, const HeadsArgs& a, const fs_heads_desc* d, float rh, float rw,
                         const void* gt, int gt_bytes, unsigned long long* hist, unsigned long long* counts) {
#define FS_HEADS8(CQ)                                                                                                            \
    case CQ:                                                                                                                     \
        FS_LAUNCH((heads_confusion8_kernel<T, CQ>), grid, dim3(256), lds, st, a, d->N, d->h, d->w, d->H, d->W, d->C, rh, rw, \
                  gt, gt_bytes, hist, counts);                                                                                   \
        break;
    switch (cq) {
        FS_HEADS8(1) FS_HEADS8(2) FS_HEADS8(3) FS_HEADS8(4) FS_HEADS8(5)
        default: break;
    }
#undef FS_HEADS8
}

}  // namespace fs

using namespace fs;

extern "C" fs_status fs_heads_confusion(void* stream, const fs_heads_desc* d, const void* const* heads, const void* gt, int gt_bytes,
                                        unsigned long long* hist, unsigned long long* counts) {
    FS_REQUIRE(d && heads && gt && hist && counts, FS_ERR_INVALID, "fs_heads_confusion: null argument");
    FS_REQUIRE(d->K >= 1 && d->K <= FS_MAX_HEADS, FS_ERR_UNSUPPORTED, "fs_heads_confusion: K=%d heads not in 1..%d", d->K, FS_MAX_HEADS);
    FS_REQUIRE(d->C >= 1 && d->C <= 32, FS_ERR_UNSUPPORTED, "fs_heads_confusion: C=%d classes not in 1..32", d->C);
    FS_REQUIRE(d->N > 0 && d->h > 0 && d->w > 0 && d->H > 0 && d->W > 0, FS_ERR_INVALID, "fs_heads_confusion: bad dimension");
    FS_REQUIRE(d->dtype == FS_F32 || d->dtype == FS_BF16, FS_ERR_INVALID, "fs_heads_confusion: bad dtype");
    FS_REQUIRE(gt_bytes == 1 || gt_bytes == 4 || gt_bytes == 8, FS_ERR_INVALID, "fs_heads_confusion: labels must be uint8, int32 or int64");
    const long long pixels = (long long)d->N * d->H * d->W;
    FS_REQUIRE(pixels < (1LL << 40), FS_ERR_UNSUPPORTED, "fs_heads_confusion: %lld output pixels (limit 2^40)", pixels);
    const int align = d->dtype == FS_F32 ? 16 : 8;
    const int cmin = ((d->C + 3) / 4) * 4;
    HeadsArgs a = {};
    for (int k = 0; k < d->K; ++k) {
        FS_REQUIRE(heads[k], FS_ERR_INVALID, "fs_heads_confusion: head %d is null", k);
        FS_REQUIRE(d->cs[k] >= cmin && d->cs[k] % 4 == 0, FS_ERR_INVALID,
                   "fs_heads_confusion: head %d channel stride %d must be a multiple of 4 and >= %d", k, d->cs[k], cmin);
        FS_REQUIRE((reinterpret_cast<uintptr_t>(heads[k]) & (align - 1)) == 0, FS_ERR_INVALID, "fs_heads_confusion: head %d misaligned", k);
        a.p[k] = heads[k];
        a.cs[k] = d->cs[k];
    }
    FS_REQUIRE((reinterpret_cast<uintptr_t>(gt) & (gt_bytes - 1)) == 0 && (reinterpret_cast<uintptr_t>(hist) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(counts) & 7) == 0,
               FS_ERR_INVALID, "fs_heads_confusion: misaligned labels / accumulators");
    const float rh = d->H > 1 ? (float)(d->h - 1) / (float)(d->H - 1) : 0.f;
    const float rw = d->W > 1 ? (float)(d->w - 1) / (float)(d->W - 1) : 0.f;
    const size_t lds = (size_t)(d->C * d->C + 2) * sizeof(unsigned int);
    hipStream_t st = (hipStream_t)stream;
    double bytes = (double)pixels * gt_bytes;
    for (int k = 0; k < d->K; ++k) bytes += (double)d->N * d->h * d->w * d->cs[k] * (d->dtype == FS_F32 ? 4 : 2);
    // grid (x, K): at most kHeadsBlocks blocks per head, every block flushes up to C * C + 2 bins of its head with global atomics
    if (d->W == 8 * d->w && d->w >= 2 && cmin <= 20) {
        const long long lanes = (long long)d->N * d->H * (d->W / 8);
        const unsigned g = (unsigned)std::min<long long>((lanes + 255) / 256, kHeadsBlocks);
        FS_NOTE_BYTES(bytes);
        if (d->dtype == FS_F32) launch_strip<float>(cmin / 4, dim3(g, d->K), lds, st, a, d, rh, rw, gt, gt_bytes, hist, counts);
        else launch_strip<bf16_t>(cmin / 4, dim3(g, d->K), lds, st, a, d, rh, rw, gt, gt_bytes, hist, counts);
        return check_launch("fs_heads_confusion");
    }
    const unsigned g = (unsigned)std::min<long long>((pixels + 255) / 256, kHeadsBlocks);
    FS_NOTE_BYTES(bytes);
    if (d->dtype == FS_F32)
        FS_LAUNCH((heads_confusion_kernel<float>), dim3(g, d->K), dim3(256), lds, st, a, d->N, d->h, d->w, d->H, d->W, d->C, rh, rw, gt,
                  gt_bytes, hist, counts);
    else
        FS_LAUNCH((heads_confusion_kernel<bf16_t>), dim3(g, d->K), dim3(256), lds, st, a, d->N, d->h, d->w, d->H, d->W, d->C, rh, rw, gt,
                  gt_bytes, hist, counts);
    return check_launch("fs_heads_confusion");
}
