// Evaluation path on the device (gfx950): class map and confusion histogram without moving logits to the host.
//
// The reference evaluator runs the network, takes exp() of the (19, 1024, 2048) fp32 score map, copies all 159 MB to the host,
// and only there reduces it to a class index per pixel (tools/engine/evaluator.py:205-225 whole_eval, :297-318
// val_func_process; np.argmax at :223) before accumulating the confusion histogram (tools/seg_opr/metric.py:7-17 hist_info).
// exp is monotone, so the class map is the arg-max of the up-sampled logits:
//   fs_bilinear_argmax   1/8-resolution NHWC logits -> bilinear x8 (align_corners=True, model_seg.py:365) -> arg-max -> uint8
//                        (N, Ho, Wo): 2 MB written instead of 159 MB, nothing materialised in between;
//   fs_hist_info         n_cl x n_cl confusion counts + labeled + correct from (pred, gt) on the device, integer atomics
//                        (bit-exact with np.bincount).
// The up-sampled class values come from logits_up.h, which states the bit contract they share with confidence.hip and eval_heads.hip;
// the class map equals the arg-max of the logits tensor the engine would have written up to ties in the last bits.
#include "logits_up.h"

namespace fs {

// one lane: 4 consecutive output columns of one output row, all classes (4 at a time)
template <typename T>
__global__ __launch_bounds__(256) void bilinear_argmax_kernel(int N, int Hi, int Wi, int Ho, int Wo, int C, float rh, float rw,
                                                              const T* __restrict__ x, int x_cs, unsigned char* __restrict__ y) {
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
        int arg[4] = {0, 0, 0, 0};
        for (int c0 = 0; c0 < C; c0 += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float p[4][4];
                quad_stage(r0, r1, x_cs, tw[q], c0, p);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float v = quad_value(p, th, tw[q], k);
                    if (c0 + k < C && v > best[q]) {       // strict: the first maximum wins (np.argmax)
                        best[q] = v;
                        arg[q] = c0 + k;
                    }
                }
            }
        }
        const uint32_t packed = (uint32_t)arg[0] | ((uint32_t)arg[1] << 8) | ((uint32_t)arg[2] << 16) | ((uint32_t)arg[3] << 24);
        *reinterpret_cast<uint32_t*>(y + ((long long)n * Ho + oh) * Wo + ow0) = packed;
    }
}

// x8 case (the network's own logits up-sample, model_seg.py:365): one lane = one 1 x 8 output strip (logits_up.h)
template <typename T, int CQ>       // CQ = ceil(C / 4) <= 5
__global__ __launch_bounds__(256) void bilinear_argmax8_kernel(int N, int Hi, int Wi, int Ho, int Wo, int C, float rh, float rw,
                                                               const T* __restrict__ x, int x_cs, unsigned char* __restrict__ y) {
    const int w8 = Wo >> 3;
    const long long total = (long long)N * Ho * w8;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int ow0 = (int)(t % w8) * 8; t /= w8;
        const int oh = (int)(t % Ho);
        const int n = (int)(t / Ho);
        Tap th;
        int bx;
        float top[3][CQ * 4], bot[3][CQ * 4];
        strip_stage<T, CQ>(x, x_cs, n, oh, ow0, Hi, Wi, rh, rw, th, bx, top, bot);
        uint32_t lo = 0, hi = 0;
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
            if (dx < 4) lo |= (uint32_t)arg << (8 * dx);
            else hi |= (uint32_t)arg << (8 * (dx - 4));
        }
        *reinterpret_cast<uint2*>(y + ((long long)n * Ho + oh) * Wo + ow0) = make_uint2(lo, hi);
    }
}

// confusion histogram: hist[n_cl * gt + pred] over pixels with 0 <= gt < n_cl; out[0] = labeled, out[1] = correct
template <typename G>
__global__ __launch_bounds__(256) void hist_info_kernel(const unsigned char* __restrict__ pred, const G* __restrict__ gt, long long n,
                                                        int n_cl, unsigned long long* __restrict__ hist,
                                                        unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned int local[];            // n_cl * n_cl + 2
    const int bins = n_cl * n_cl;
    lds_zero(local, bins + 2);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)gt[i];
        if (g >= 0 && g < n_cl) {
            const int p = pred[i];
            atomicAdd(&local[bins], 1u);
            if (p == (int)g) atomicAdd(&local[bins + 1], 1u);
            if (p < n_cl) atomicAdd(&local[(int)g * n_cl + p], 1u);
        }
    }
    lds_flush(local, bins, hist);
    if (threadIdx.x == 0) {
        if (local[bins]) atomicAdd(&counts[0], (unsigned long long)local[bins]);
        if (local[bins + 1]) atomicAdd(&counts[1], (unsigned long long)local[bins + 1]);
    }
}

}  // namespace fs

using namespace fs;

extern "C" fs_status fs_bilinear_argmax(void* stream, const fs_resize_desc* d, const void* x, unsigned char* classes) {
    FS_REQUIRE(d && x && classes, FS_ERR_INVALID, "fs_bilinear_argmax: null argument");
    ClassMapLaunch l;                                      // x: 8 bytes for every dtype; no confidence map, no ignore label
    if (const fs_status e = class_map_launch("fs_bilinear_argmax", d, x, 8, classes, nullptr, 0, &l)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (l.strip)
        FS_DTYPE_SWITCH(d->dtype, T, FS_LAUNCH((bilinear_argmax8_kernel<T, 5>), dim3(l.grid), dim3(256), 0, st, d->N, d->Hi, d->Wi, d->Ho, d->Wo,
                                               d->C, l.rh, l.rw, (const T*)x, d->x_cs, classes));
    else
        FS_DTYPE_SWITCH(d->dtype, T, FS_LAUNCH((bilinear_argmax_kernel<T>), dim3(l.grid), dim3(256), 0, st, d->N, d->Hi, d->Wi, d->Ho, d->Wo,
                                               d->C, l.rh, l.rw, (const T*)x, d->x_cs, classes));
    return check_launch("fs_bilinear_argmax");
}

extern "C" fs_status fs_hist_info(void* stream, const unsigned char* pred, const void* gt, int gt_bytes, long long n, int n_cl,
                                  unsigned long long* hist, unsigned long long* counts) {
    FS_REQUIRE(n >= 0 && hist && counts, FS_ERR_INVALID, "fs_hist_info: bad argument");
    if (n == 0) return FS_OK;                              // an empty image contributes nothing (pointers may be null)
    FS_REQUIRE(pred && gt, FS_ERR_INVALID, "fs_hist_info: null pred / gt");
    FS_REQUIRE(n_cl > 0 && n_cl <= 64, FS_ERR_UNSUPPORTED, "fs_hist_info: n_cl=%d not in 1..64", n_cl);
    FS_REQUIRE(gt_bytes == 1 || gt_bytes == 4 || gt_bytes == 8, FS_ERR_INVALID, "fs_hist_info: labels must be uint8, int32 or int64");
    long long g = (n + 256 * 16 - 1) / (256 * 16);
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    const size_t lds = (size_t)(n_cl * n_cl + 2) * sizeof(unsigned int);
    hipStream_t st = (hipStream_t)stream;
    if (gt_bytes == 1)
        FS_LAUNCH((hist_info_kernel<unsigned char>), dim3((unsigned)g), dim3(256), lds, st, pred, (const unsigned char*)gt, n, n_cl, hist, counts);
    else if (gt_bytes == 4)
        FS_LAUNCH((hist_info_kernel<int>), dim3((unsigned)g), dim3(256), lds, st, pred, (const int*)gt, n, n_cl, hist, counts);
    else
        FS_LAUNCH((hist_info_kernel<long long>), dim3((unsigned)g), dim3(256), lds, st, pred, (const long long*)gt, n, n_cl, hist, counts);
    return check_launch("fs_hist_info");
}
