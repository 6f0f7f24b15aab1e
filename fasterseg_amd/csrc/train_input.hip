// Training batches on the device (gfx950): the reference's TrainPre (search|train/dataloader.py) after BaseDataset._open_image.
//
// The reference builds every crop on the host (tools/utils/img_utils.py): cv2.flip, cv2.resize of the uint8 image (INTER_LINEAR) and
// label (INTER_NEAREST) to int(H * s) x int(W * s), a float64 normalisation, the crop / pad_image_to_shape, the INTER_NEAREST label
// down-sample, then a pinned copy of the fp32 batch.  Here:
//   fs_train_batch   B uint8 sources -> the whole batch in one launch: (B, 3, crop_h, crop_w) fp32 images and
//                    (B, crop_h / g, crop_w / g) int64 labels.  Per output pixel only integer arithmetic runs on the device (the
//                    scaled coordinate, the pad test, the mirror); every floating-point index (cv2's linear taps and nearest indices)
//                    comes from host-built tables, and the normalisation is a 3 x 256 fp32 lookup table: bit-exact by construction;
//   fs_resize_u8     the one-time down-sampling at load (BaseDataset._open_image): uint8 HWC INTER_LINEAR or uint8 INTER_NEAREST.
// No atomics: every output element is written once by one lane, a pure function of the inputs.
#include <string.h>

#include "common.h"

namespace fs {

namespace {

__device__ __forceinline__ int grid_stride_i() { return (int)(gridDim.x * blockDim.x); }

// cv2's 8-bit INTER_LINEAR of one channel from its four taps (eval_ms.hip's resize_u8: OpenCV 4's HResizeLinear in int32, then
// VResizeLinear with INTER_RESIZE_COEF_BITS = 11)
__device__ __forceinline__ int lin_u8(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1) {
    const int d0 = s00 * a0 + s01 * a1;
    const int d1 = s10 * a0 + s11 * a1;
    const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct TrainArgs {
    int crop_h, crop_w, gy, gx, lh, lw, img_lanes, lanes;
};

}  // namespace

// blockIdx.y = sample.  Lanes [0, img_lanes): 4 consecutive output columns of one image row, 3 channels -> three 16-byte stores;
// lanes [img_lanes, lanes): 2 consecutive label columns -> one 16-byte store (lw even) or two 8-byte stores.
__global__ __launch_bounds__(256) void train_batch_kernel(TrainArgs a, const fs_train_sample* __restrict__ samples,
                                                          const unsigned char* const* __restrict__ images,
                                                          const unsigned char* const* __restrict__ labels, const int* __restrict__ tab,
                                                          const float* __restrict__ norm, float* __restrict__ out_img,
                                                          long long* __restrict__ out_lbl) {
    const int b = blockIdx.y;
    const fs_train_sample s = samples[b];
    const int wq = a.crop_w >> 2;
    const long long plane = (long long)a.crop_h * a.crop_w;
    const int2* ylin = reinterpret_cast<const int2*>(tab + s.ylin);
    const int2* xlin = reinterpret_cast<const int2*>(tab + s.xlin);
    for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < a.lanes; idx += grid_stride_i()) {
        if (idx < a.img_lanes) {
            const int y = idx / wq;
            const int x0 = (idx - y * wq) * 4;
            const int ry = y - s.top;                      // row of the crop; outside [0, rows): pad_image_to_shape's 0.0
            float v[3][4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][q] = 0.f;
            if (ry >= 0 && ry < s.rows) {
                const unsigned char* img = images[b];
                const int2 ty = ylin[s.pos_h + ry];        // taps of the scaled row
                const int sy0 = clampi(ty.x, s.H - 1);
                const int sy1 = min(sy0 + 1, s.H - 1);
                const int b0 = ty.y & 0xffff, b1 = (ty.y >> 16) & 0xffff;
                const unsigned char* r0 = img + (long long)sy0 * s.W * 3;
                const unsigned char* r1 = img + (long long)sy1 * s.W * 3;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int rx = x0 + q - s.left;
                    if (rx < 0 || rx >= s.cols) continue;
                    const int2 tx = xlin[s.pos_w + rx];
                    int sx0 = clampi(tx.x, s.W - 1);
                    int sx1 = min(sx0 + 1, s.W - 1);
                    if (s.mirror) {                        // resize(flip(A)): the same taps read the mirrored source columns
                        sx0 = s.W - 1 - sx0;
                        sx1 = s.W - 1 - sx1;
                    }
                    const int a0 = tx.y & 0xffff, a1 = (tx.y >> 16) & 0xffff;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int u = lin_u8(r0[sx0 * 3 + c], r0[sx1 * 3 + c], r1[sx0 * 3 + c], r1[sx1 * 3 + c], a0, a1, b0, b1);
                        v[c][q] = norm[c * 256 + u];
                    }
                }
            }
            float* o = out_img + (long long)b * 3 * plane + (long long)y * a.crop_w + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                f32x4 st;
                st[0] = v[c][0]; st[1] = v[c][1]; st[2] = v[c][2]; st[3] = v[c][3];
                *reinterpret_cast<f32x4*>(o + c * plane) = st;
            }
        } else {
            const int lq = (a.lw + 1) >> 1;
            const int li = idx - a.img_lanes;
            const int j = li / lq;
            const int i0 = (li - j * lq) * 2;
            const int ry = clampi(tab[a.gy + j], a.crop_h - 1) - s.top;   // the label down-sample's row of the padded crop
            const bool row_ok = ry >= 0 && ry < s.rows;
            const unsigned char* lrow = nullptr;
            if (row_ok) lrow = labels[b] + (long long)clampi(tab[s.ynn + s.pos_h + ry], s.H - 1) * s.W;
            long long v[2] = {255, 255};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = i0 + q;
                if (i >= a.lw || !row_ok) continue;
                const int rx = clampi(tab[a.gx + i], a.crop_w - 1) - s.left;
                if (rx < 0 || rx >= s.cols) continue;
                int sx = clampi(tab[s.xnn + s.pos_w + rx], s.W - 1);
                if (s.mirror) sx = s.W - 1 - sx;
                v[q] = lrow[sx];
            }
            long long* o = out_lbl + ((long long)b * a.lh + j) * a.lw + i0;
            if ((a.lw & 1) == 0) {
                *reinterpret_cast<longlong2*>(o) = make_longlong2(v[0], v[1]);
            } else {
                o[0] = v[0];
                if (i0 + 1 < a.lw) o[1] = v[1];
            }
        }
    }
}

// one lane: one output pixel, C channels.  mode 0: INTER_LINEAR taps (int32 pairs), mode 1: INTER_NEAREST indices
__global__ __launch_bounds__(256) void resize_u8_kernel(const unsigned char* __restrict__ src, int H, int W, int C,
                                                        unsigned char* __restrict__ dst, int h, int w, const int* __restrict__ ytab,
                                                        const int* __restrict__ xtab, int mode) {
    const long long n = (long long)h * w;
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % w);
        const int y = (int)(idx / w);
        unsigned char* o = dst + idx * C;
        if (mode == 1) {
            const unsigned char* p = src + ((long long)clampi(ytab[y], H - 1) * W + clampi(xtab[x], W - 1)) * C;
            for (int c = 0; c < C; ++c) o[c] = p[c];
            continue;
        }
        const int2 ty = reinterpret_cast<const int2*>(ytab)[y];
        const int2 tx = reinterpret_cast<const int2*>(xtab)[x];
        const int sy0 = clampi(ty.x, H - 1), sy1 = min(sy0 + 1, H - 1);
        const int sx0 = clampi(tx.x, W - 1), sx1 = min(sx0 + 1, W - 1);
        const unsigned char* r0 = src + (long long)sy0 * W * C;
        const unsigned char* r1 = src + (long long)sy1 * W * C;
        for (int c = 0; c < C; ++c)
            o[c] = (unsigned char)lin_u8(r0[sx0 * C + c], r0[sx1 * C + c], r1[sx0 * C + c], r1[sx1 * C + c], tx.y & 0xffff,
                                         (tx.y >> 16) & 0xffff, ty.y & 0xffff, (ty.y >> 16) & 0xffff);
    }
}

}  // namespace fs

using namespace fs;

static inline bool aligned_to(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }

static inline long long round16(long long v) { return (v + 15) & ~15LL; }

// layout of the device argument block: B descriptors, then B image pointers, then B label pointers (each part 16-byte aligned)
static inline long long ptr_offset(int B) { return round16((long long)B * (long long)sizeof(fs_train_sample)); }

extern "C" long long fs_train_batch_args_bytes(int B) {
    if (B < 1) return 0;
    return ptr_offset(B) + 2 * round16((long long)B * (long long)sizeof(void*));
}

static bool table_fits(long long off, long long n, long long total) { return off >= 0 && n >= 0 && off + n <= total; }

extern "C" fs_status fs_train_batch(void* stream, const fs_train_batch_desc* d, const fs_train_sample* samples,
                                    const unsigned char* const* images, const unsigned char* const* labels, const int* tables,
                                    const float* norm, void* staging, void* args, float* out_img, long long* out_lbl) {
    FS_REQUIRE(d && samples && images && labels && tables && norm && staging && args && out_img && out_lbl, FS_ERR_INVALID,
               "fs_train_batch: null argument");
    FS_REQUIRE(d->B >= 1 && d->B <= 65535, FS_ERR_INVALID, "fs_train_batch: batch size %d outside [1, 65535]", d->B);
    FS_REQUIRE(d->crop_h > 0 && d->crop_w > 0, FS_ERR_INVALID, "fs_train_batch: bad crop %dx%d", d->crop_h, d->crop_w);
    FS_REQUIRE(d->crop_w % 4 == 0, FS_ERR_UNSUPPORTED, "fs_train_batch: crop width %d must be a multiple of 4", d->crop_w);
    FS_REQUIRE(d->g >= 1 && d->crop_h % d->g == 0 && d->crop_w % d->g == 0, FS_ERR_INVALID,
               "fs_train_batch: gt_down_sampling %d must divide the crop %dx%d", d->g, d->crop_h, d->crop_w);
    const int lh = d->crop_h / d->g, lw = d->crop_w / d->g;
    const long long img_lanes = (long long)d->crop_h * (d->crop_w / 4);
    const long long lanes = img_lanes + (long long)lh * ((lw + 1) / 2);
    FS_REQUIRE(lanes < (1LL << 31), FS_ERR_UNSUPPORTED, "fs_train_batch: crop %dx%d too large", d->crop_h, d->crop_w);
    FS_REQUIRE(table_fits(d->gy, lh, d->n_tables) && table_fits(d->gx, lw, d->n_tables), FS_ERR_INVALID,
               "fs_train_batch: label down-sample tables (%d, %d) outside the %lld-entry table", d->gy, d->gx, d->n_tables);
    for (int b = 0; b < d->B; ++b) {
        const fs_train_sample& s = samples[b];
        FS_REQUIRE(images[b] && labels[b], FS_ERR_INVALID, "fs_train_batch: sample %d: null source", b);
        FS_REQUIRE(s.H > 0 && s.W > 0 && s.sh > 0 && s.sw > 0 && (s.mirror == 0 || s.mirror == 1), FS_ERR_INVALID,
                   "fs_train_batch: sample %d: bad source %dx%d, scaled %dx%d or mirror %d", b, s.H, s.W, s.sh, s.sw, s.mirror);
        FS_REQUIRE(s.rows >= 1 && s.cols >= 1 && s.pos_h >= 0 && s.pos_w >= 0 && s.pos_h + s.rows <= s.sh && s.pos_w + s.cols <= s.sw &&
                       s.top >= 0 && s.left >= 0 && s.top + s.rows <= d->crop_h && s.left + s.cols <= d->crop_w,
                   FS_ERR_INVALID, "fs_train_batch: sample %d: crop (%d, %d) + %dx%d at (%d, %d) does not fit the %dx%d scaled image and "
                   "the %dx%d crop", b, s.pos_h, s.pos_w, s.rows, s.cols, s.top, s.left, s.sh, s.sw, d->crop_h, d->crop_w);
        FS_REQUIRE(s.ylin % 2 == 0 && s.xlin % 2 == 0 && table_fits(s.ylin, 2LL * s.sh, d->n_tables) &&
                       table_fits(s.xlin, 2LL * s.sw, d->n_tables) && table_fits(s.ynn, s.sh, d->n_tables) &&
                       table_fits(s.xnn, s.sw, d->n_tables),
                   FS_ERR_INVALID, "fs_train_batch: sample %d: tap tables (%d, %d, %d, %d) outside the %lld-entry table or odd", b,
                   s.ylin, s.xlin, s.ynn, s.xnn, d->n_tables);
    }
    FS_REQUIRE(aligned_to(out_img, 16) && aligned_to(out_lbl, lw % 2 == 0 ? 16 : 8) && aligned_to(tables, 8) && aligned_to(args, 16) &&
                   aligned_to(norm, 4),
               FS_ERR_INVALID, "fs_train_batch: misaligned operand");
    const int B = d->B;
    const long long po = ptr_offset(B), pb = round16((long long)B * (long long)sizeof(void*));
    char* st = static_cast<char*>(staging);
    memcpy(st, samples, sizeof(fs_train_sample) * (size_t)B);
    memcpy(st + po, images, sizeof(void*) * (size_t)B);
    memcpy(st + po + pb, labels, sizeof(void*) * (size_t)B);
    hipStream_t strm = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(args, staging, (size_t)fs_train_batch_args_bytes(B), hipMemcpyHostToDevice, strm);
    FS_REQUIRE(e == hipSuccess, FS_ERR_LAUNCH, "fs_train_batch: argument upload failed: %s", hipGetErrorString(e));
    TrainArgs a;
    a.crop_h = d->crop_h; a.crop_w = d->crop_w; a.gy = d->gy; a.gx = d->gx; a.lh = lh; a.lw = lw;
    a.img_lanes = (int)img_lanes; a.lanes = (int)lanes;
    long long gx = (lanes + 255) / 256;
    if (gx > 1024) gx = 1024;
    double src_bytes = 0;
    for (int b = 0; b < B; ++b) src_bytes += (double)samples[b].rows * samples[b].cols * 4;   // 3 image bytes + 1 label byte per pixel
    FS_NOTE_BYTES((double)B * ((double)d->crop_h * d->crop_w * 12 + (double)lh * lw * 8) + src_bytes);
    char* ab = static_cast<char*>(args);
    FS_LAUNCH(train_batch_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, strm, a, reinterpret_cast<const fs_train_sample*>(ab),
              reinterpret_cast<const unsigned char* const*>(ab + po), reinterpret_cast<const unsigned char* const*>(ab + po + pb), tables,
              norm, out_img, out_lbl);
    return check_launch("fs_train_batch");
}

extern "C" fs_status fs_resize_u8(void* stream, const unsigned char* src, int H, int W, int C, unsigned char* dst, int h, int w,
                                  const int* ytab, const int* xtab, int mode) {
    FS_REQUIRE(src && dst && ytab && xtab, FS_ERR_INVALID, "fs_resize_u8: null argument");
    FS_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0 && C >= 1 && C <= 4, FS_ERR_INVALID, "fs_resize_u8: bad shape %dx%dx%d -> %dx%d", H, W,
               C, h, w);
    FS_REQUIRE(mode == 0 || mode == 1, FS_ERR_INVALID, "fs_resize_u8: mode must be 0 (linear) or 1 (nearest)");
    FS_REQUIRE(mode == 1 || (aligned_to(ytab, 8) && aligned_to(xtab, 8)), FS_ERR_INVALID, "fs_resize_u8: misaligned tap table");
    FS_REQUIRE(src != dst, FS_ERR_INVALID, "fs_resize_u8: in-place resize");
    const long long n = (long long)h * w;
    long long g = (n + 255) / 256;
    if (g > 16384) g = 16384;
    FS_NOTE_BYTES((double)n * C * 2);
    FS_LAUNCH(resize_u8_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, src, H, W, C, dst, h, w, ytab, xtab, mode);
    return check_launch("fs_resize_u8");
}
