// Prediction rendering on the device (gfx950): the tail of the reference's test / eval loop after the arg-max.
//
// The reference turns a class map into files on the host, per frame: a Python double loop over every pixel for the trainId -> labelId
// map (train/test.py:66-69), and per overlay panel 19 np.where passes plus cv2.addWeighted (tools/utils/visualize.py:6-41: set_img_color,
// show_prediction, show_img).  Here ONE launch writes a whole composite - the untouched image, up to four overlay panels, the black
// pivot columns between them - and, optionally, the label-ID map of the first class map.  Pure byte streaming, no atomics: every output
// byte is written once by one lane, a pure function of the inputs.
//
// Work item = (row, panel, chunk).  Per (row, panel) the lanes agree on a head of 0..15 pixels after which the panel's destination bytes
// are 16-byte aligned (3 is invertible mod 16, so such a head exists for every base, pitch and panel offset): item 0 writes the head
// pixels and the pivot columns behind the panel byte by byte, item k >= 1 the 16 pixels from head + 16 (k - 1) on: 48 image bytes and 16
// class bytes in, three aligned 16-byte stores out.  The last, partial chunk of a row goes byte by byte.  The loads of a vector chunk are
// as aligned as the sources happen to be (they are when the head is 0 and W % 16 == 0, the 1024 x 2048 frame); they are declared with
// alignment 1 and the compiler picks the access for the target.
#include "common.h"

namespace fs {

namespace {

struct RenderArgs {
    int H, W, P, panels, image_panel, gap, n_items, id_panel;
    long long dst_pitch;
    long long total;
    int show255[FS_RENDER_MAX_PANELS];
    float alpha[FS_RENDER_MAX_PANELS], beta[FS_RENDER_MAX_PANELS];
    const unsigned char* maps[FS_RENDER_MAX_PANELS];
    int n_colors, background;
};

struct __attribute__((packed, aligned(1))) U128Unaligned {
    u32x4 v;
};
__device__ __forceinline__ u32x4 ld16_any(const unsigned char* p) { return reinterpret_cast<const U128Unaligned*>(p)->v; }

// set_img_color for one channel byte: c = the colour the class paints (or the image byte), o = the image byte.  The FMA is spelled
// out: cv2.addWeighted's fp32 form with the contraction fixed, round-half-even, saturated.
__device__ __forceinline__ unsigned int blend(float c, float o, float alpha, float beta) {
    const int v = __float2int_rn(__fmaf_rn(c, alpha, __fmul_rn(o, beta)));
    return (unsigned int)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// entry of the LDS table: the colour's three bytes, bit 24 = "this class is painted"
__device__ __forceinline__ unsigned int overlay_byte(unsigned int e, int k, int ch, unsigned int o, int show255, float alpha, float beta) {
    unsigned int c = (e >> 24) ? ((e >> (8 * ch)) & 255u) : o;
    if (show255 && k == 255) c = 0;               // painted after the colours (visualize.py:11-12)
    return blend((float)c, (float)o, alpha, beta);
}

// kernel arguments live in SGPRs: a select chain instead of a dynamically indexed (scratch) copy of the array
template <typename T> __device__ __forceinline__ T pick(const T (&v)[FS_RENDER_MAX_PANELS], int i) {
    return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3]));
}

}  // namespace

__global__ __launch_bounds__(256) void render_prediction_kernel(RenderArgs a, const unsigned char* image, const unsigned char* __restrict__ palette,
                                                                const unsigned char* __restrict__ lut, unsigned char* composite,
                                                                unsigned char* __restrict__ ids) {
    __shared__ unsigned int s_pal[256];
    __shared__ unsigned int s_lut[256];
    {
        const int k = threadIdx.x;                 // blockDim.x == 256
        unsigned int e = 0;
        if (k < a.n_colors && k != a.background) e = (unsigned int)palette[3 * k] | ((unsigned int)palette[3 * k + 1] << 8) |
                                                     ((unsigned int)palette[3 * k + 2] << 16) | (1u << 24);
        s_pal[k] = e;
        s_lut[k] = ids ? (unsigned int)lut[k] : 0u;
    }
    __syncthreads();
    const int W = a.W;
    const int PW = a.P > 0 ? a.P : 1;              // ids only: one pass over the class map
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < a.total; idx += (long long)gridDim.x * blockDim.x) {
        long long t = idx;
        const int item = divmod32(t, a.n_items);
        const int p = divmod32(t, PW);
        const int y = (int)t;
        const int ov = p - a.image_panel;          // overlay index of this panel; -1: the image panel
        const bool is_overlay = a.P > 0 && ov >= 0;
        const bool do_ids = ids != nullptr && p == a.id_panel;
        const long long pix0 = (long long)y * W;
        const unsigned char* img_row = a.P > 0 ? image + pix0 * 3 : nullptr;
        const unsigned char* map_row = is_overlay ? pick(a.maps, ov) + pix0 : nullptr;
        const unsigned char* id_map = do_ids ? a.maps[0] + pix0 : nullptr;
        unsigned char* id_row = do_ids ? ids + pix0 : nullptr;
        unsigned char* dst = a.P > 0 ? composite + (long long)y * a.dst_pitch + 3LL * p * (W + a.gap) : nullptr;
        int head;
        if (a.P > 0) head = (int)(((16u - (unsigned int)(reinterpret_cast<uintptr_t>(dst) & 15u)) * 11u) & 15u);   // (dst + 3 head) % 16 == 0
        else head = (int)((16u - (unsigned int)(reinterpret_cast<uintptr_t>(id_row) & 15u)) & 15u);
        if (head > W) head = W;
        const int show255 = is_overlay ? pick(a.show255, ov) : 0;
        const float alpha = is_overlay ? pick(a.alpha, ov) : 0.f, beta = is_overlay ? pick(a.beta, ov) : 0.f;
        int x0, n;
        if (item == 0) {
            x0 = 0;
            n = head;
            if (a.P > 0 && p < a.P - 1) {            // the black pivot behind this panel
                unsigned char* g = dst + 3LL * W;
                for (int i = 0; i < 3 * a.gap; ++i) g[i] = 0;
            }
        } else {
            x0 = head + 16 * (item - 1);
            n = W - x0 < 16 ? W - x0 : 16;
        }
        if (n <= 0) continue;
        if (n < 16 || item == 0) {                   // head, or the partial last chunk: byte by byte
            for (int i = 0; i < n; ++i) {
                const int x = x0 + i;
                if (do_ids) id_row[x] = (unsigned char)s_lut[id_map[x]];
                if (a.P == 0) continue;
                if (is_overlay) {
                    const int k = map_row[x];
                    const unsigned int e = s_pal[k];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch)
                        dst[3 * x + ch] = (unsigned char)overlay_byte(e, k, ch, img_row[3 * x + ch], show255, alpha, beta);
                } else {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) dst[3 * x + ch] = img_row[3 * x + ch];
                }
            }
            continue;
        }
        // 16 whole pixels, destination 16-byte aligned
        if (do_ids) {
            const u32x4 m = ld16_any(id_map + x0);
            u32x4 o;
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                unsigned int r = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) r |= s_lut[(m[wd] >> (8 * b)) & 255u] << (8 * b);
                o[wd] = r;
            }
            unsigned char* q = id_row + x0;
            if ((reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
                stg16(q, o);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) q[i] = (unsigned char)(o[i >> 2] >> (8 * (i & 3)));
            }
        }
        if (a.P == 0) continue;
        u32x4 im[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) im[v] = ld16_any(img_row + 3 * x0 + 16 * v);
        if (is_overlay) {
            const u32x4 m = ld16_any(map_row + x0);
            unsigned int e[16];
            int k[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                k[i] = (int)((m[i >> 2] >> (8 * (i & 3))) & 255u);
                e[i] = s_pal[k[i]];
            }
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                u32x4 o;
#pragma unroll
                for (int wd = 0; wd < 4; ++wd) {
                    unsigned int r = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int j = 16 * v + 4 * wd + b;       // byte of the 48: pixel j / 3, channel j % 3
                        const unsigned int ob = (im[v][wd] >> (8 * b)) & 255u;
                        r |= overlay_byte(e[j / 3], k[j / 3], j % 3, ob, show255, alpha, beta) << (8 * b);
                    }
                    o[wd] = r;
                }
                im[v] = o;
            }
        }
#pragma unroll
        for (int v = 0; v < 3; ++v) stg16(dst + 3 * x0 + 16 * v, im[v]);
    }
}

}  // namespace fs

using namespace fs;

extern "C" fs_status fs_render_prediction(void* stream, const fs_render_desc* d, const unsigned char* image, const unsigned char* const maps[4],
                                          const unsigned char* palette, const unsigned char* lut, unsigned char* composite,
                                          unsigned char* ids) {
    FS_REQUIRE(d, FS_ERR_INVALID, "fs_render_prediction: null descriptor");
    FS_REQUIRE(d->H > 0 && d->W > 0, FS_ERR_INVALID, "fs_render_prediction: bad size %dx%d", d->H, d->W);
    FS_REQUIRE(d->panels >= 0 && d->panels <= FS_RENDER_MAX_PANELS, FS_ERR_INVALID, "fs_render_prediction: %d overlay panels outside [0, %d]",
               d->panels, FS_RENDER_MAX_PANELS);
    FS_REQUIRE((d->image_panel == 0 || d->image_panel == 1) && (d->write_ids == 0 || d->write_ids == 1) && d->gap >= 0 && d->gap <= 4096,
               FS_ERR_INVALID, "fs_render_prediction: image_panel %d / write_ids %d must be 0 or 1, gap %d in [0, 4096]", d->image_panel,
               d->write_ids, d->gap);
    FS_REQUIRE(d->n_colors >= 0 && d->n_colors <= 256, FS_ERR_INVALID, "fs_render_prediction: n_colors %d outside [0, 256]", d->n_colors);
    const int P = d->image_panel + d->panels;
    FS_REQUIRE(P > 0 || d->write_ids, FS_ERR_INVALID, "fs_render_prediction: no panel and no label-ID map asked for");
    if (P > 0) {
        FS_REQUIRE(image && composite, FS_ERR_INVALID, "fs_render_prediction: null image or composite");
        const long long need = 3LL * ((long long)d->W * P + (long long)d->gap * (P - 1));
        FS_REQUIRE(d->dst_pitch >= need, FS_ERR_INVALID, "fs_render_prediction: dst_pitch %d below the %lld bytes of a composite row",
                   d->dst_pitch, need);
    }
    if (d->panels > 0 || d->write_ids) {
        FS_REQUIRE(maps, FS_ERR_INVALID, "fs_render_prediction: null class-map list");
        const int n_maps = d->panels > 0 ? d->panels : 1;
        for (int i = 0; i < n_maps; ++i) FS_REQUIRE(maps[i], FS_ERR_INVALID, "fs_render_prediction: class map %d is null", i);
    }
    FS_REQUIRE(d->panels == 0 || d->n_colors == 0 || palette, FS_ERR_INVALID, "fs_render_prediction: null palette");
    FS_REQUIRE(!d->write_ids || (lut && ids), FS_ERR_INVALID, "fs_render_prediction: write_ids without a table or an output");
    for (int i = 0; i < d->panels; ++i)
        FS_REQUIRE(d->alpha[i] == d->alpha[i] && d->beta[i] == d->beta[i], FS_ERR_INVALID, "fs_render_prediction: panel %d: NaN weight", i);
    RenderArgs a;
    a.H = d->H; a.W = d->W; a.P = P; a.panels = d->panels; a.image_panel = d->image_panel; a.gap = d->gap;
    a.n_items = 1 + (d->W + 15) / 16;
    a.id_panel = d->panels > 0 ? d->image_panel : 0;        // the lanes of the first overlay panel (or of the only pass) write the ids
    a.dst_pitch = d->dst_pitch;
    a.total = (long long)d->H * (P > 0 ? P : 1) * a.n_items;
    FS_REQUIRE(a.total < (1LL << 31), FS_ERR_UNSUPPORTED, "fs_render_prediction: %dx%d with %d panels is too large", d->H, d->W, P);
    for (int i = 0; i < FS_RENDER_MAX_PANELS; ++i) {
        const bool on = i < d->panels;
        a.show255[i] = on ? (d->show255[i] != 0) : 0;
        a.alpha[i] = on ? d->alpha[i] : 0.f;
        a.beta[i] = on ? d->beta[i] : 0.f;
        a.maps[i] = (maps && (on || (i == 0 && d->write_ids))) ? maps[i] : nullptr;
    }
    a.n_colors = d->panels > 0 ? d->n_colors : 0;
    a.background = d->background;
    long long g = (a.total + 255) / 256;
    if (g > 8192) g = 8192;
    const double px = (double)d->H * d->W;
    // per panel 3 image bytes in and 3 out, a class byte per overlay, the pivots; the ids: a byte out (and in, when no overlay reads the map)
    FS_NOTE_BYTES(px * (6.0 * P + d->panels + (d->write_ids ? (d->panels > 0 ? 1.0 : 2.0) : 0.0)) + (P > 1 ? 3.0 * d->gap * (P - 1) * d->H : 0.0));
    FS_LAUNCH(render_prediction_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, a, image, a.n_colors > 0 ? palette : nullptr,
              d->write_ids ? lut : nullptr, P > 0 ? composite : nullptr, d->write_ids ? ids : nullptr);
    return check_launch("fs_render_prediction");
}
