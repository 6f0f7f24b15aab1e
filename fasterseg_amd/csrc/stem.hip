// Stem convolution: 3x3 stride-2 pad-1 on the input image (Cin = 3), NHWC output.
//
// Replaces ConvNorm(3, C, kernel_size=3, stride=2) at reference train/model_seg.py:193 / search/model_search.py:148
// (nn.Conv2d + BatchNorm2d + ReLU, operations.py:77-82).  Cin=3 is pure bandwidth (AI ~10 flop/B):
// a direct convolution on the vector ALUs that reads the planar image coalesced along W, keeps the 27 taps of one
// output pixel in registers, takes the filter through the scalar cache (wave-uniform addresses) and writes 16
// consecutive output channels per lane, so the image never needs an NCHW->NHWC repack.
//
// Two image sources feed the same three kernel bodies (template parameter Src):
//   StemF32  fs_conv_stem_fwd     planar fp32 NCHW, already normalised.
//   StemU8   fs_conv_stem_u8_fwd  uint8 N x H x W x 3 (interleaved RGB); byte u of channel c enters the convolution as
//                                 ((float)u / 255.f - mean[c]) / std[c] (fp32, IEEE division - the expression of
//                                 eval_ms.hip's window builder and of the reference's normalize, tools/utils/img_utils.py:179-185).
//                                 Taps outside the image are 0.0 AFTER normalisation, which is why the affine map is not folded
//                                 into the filter and shift: border pixels see fewer taps.
// Only the global read and the normalisation differ: window layout, tap gathers, operand split, MFMA order, epilogue and stores
// are shared, so for the same normalised values both entry points write the same bits (tests/test_stem_u8_gpu.py).
//
// Dispatch (both sources): the LDS-tiled forms need W % 4 == 0, N <= 65535 and an aligned image base - 16 bytes for fp32
// (a pixel quad of one channel is one 16-byte load), 4 bytes for uint8 (a pixel quad of all three channels is 12 contiguous bytes at
// a multiple of 12 from the base: one 12-byte load, 297 per tile instead of 891 16-byte ones).  Of the tiled forms, bf16 output with
// Cout <= 64, Cout % 8 == 0 takes the MFMA kernel, everything else the vector-ALU one.  Any other W or base alignment takes the direct
// kernel (scalar fp32 loads / byte loads).
#include "common.h"

namespace fs {

// LDS tile geometry of the tiled kernels below (the image sources stage whole windows of it)
constexpr int S_TH = 4, S_TW = 64;
constexpr int S_ROWS = 2 * S_TH + 1;          // input rows of a tile
constexpr int S_HALF = S_TW + 2;              // even (odd) columns of a tile: window cols [2*ow0-4, 2*ow0+128)
constexpr int S_PITCH = S_HALF + 2;
constexpr int S_VPR = S_HALF / 2;                          // pixel quads per staged row (33)
constexpr int S_VECS = 3 * S_ROWS * S_VPR;                 // float4 vectors of a tile's window (891)
constexpr int S_LD = (S_VECS + 255) / 256;                 // ... per thread (4)
constexpr int S_QUADS = S_ROWS * S_VPR;                    // three-channel pixel quads of a tile's window (297)
constexpr int S_QLD = (S_QUADS + 255) / 256;               // ... per thread (2)
constexpr int S_WIN = 2 * 3 * S_ROWS * S_PITCH;            // floats of a window: [parity][c][row][col]

// four consecutive pixels of channel c, window row r, quad q -> the window's even / odd column planes
__device__ __forceinline__ void stem_put_quad(float* win, int c, int r, int q, const f32x4& t) {
    float* ev = win + ((0 * 3 + c) * S_ROWS + r) * S_PITCH;
    float* od = win + ((1 * 3 + c) * S_ROWS + r) * S_PITCH;
    ev[2 * q] = t[0]; od[2 * q] = t[1];
    ev[2 * q + 1] = t[2]; od[2 * q + 1] = t[3];
}

struct StemNoNorm {};
struct StemNorm { float mean[3], std[3]; };

// Image source: planar fp32 NCHW.  A tile's window is 891 float4 vectors (channel, row, quad), four per thread.
struct StemF32 {
    typedef float Elem;
    typedef StemNoNorm Norm;
    static constexpr int ALIGN = 16;
    struct Regs { f32x4 v[S_LD]; };
    static __device__ __forceinline__ float tap(const float* __restrict__ x, const Norm&, int n, int c, int ih, int iw, int H, int W) {
        return x[(((long long)n * 3 + c) * H + ih) * W + iw];
    }
    static __device__ __forceinline__ void load(Regs& reg, const float* __restrict__ x, int H, int W, int n, int oh0, int ow0, int tid) {
#pragma unroll
        for (int j = 0; j < S_LD; ++j) {
            const int v = tid + 256 * j;
            const int c = v / (S_ROWS * S_VPR);
            const int rem = v - c * (S_ROWS * S_VPR);
            const int r = rem / S_VPR, q = rem - r * S_VPR;
            const int ih = 2 * oh0 - 1 + r, iw = 2 * ow0 - 4 + 4 * q;
            f32x4 t = {0.f, 0.f, 0.f, 0.f};
            if (v < S_VECS && (unsigned)ih < (unsigned)H && iw >= 0 && iw + 3 < W)
                t = *reinterpret_cast<const f32x4*>(x + (((long long)n * 3 + c) * H + ih) * W + iw);
            reg.v[j] = t;
        }
    }
    static __device__ __forceinline__ void write(const Regs& reg, const Norm&, float* win, int tid) {
#pragma unroll
        for (int j = 0; j < S_LD; ++j) {
            const int v = tid + 256 * j;
            if (v < S_VECS) {
                const int c = v / (S_ROWS * S_VPR);
                const int rem = v - c * (S_ROWS * S_VPR);
                const int r = rem / S_VPR, q = rem - r * S_VPR;
                stem_put_quad(win, c, r, q, reg.v[j]);
            }
        }
    }
};

// Image source: uint8 NHWC (interleaved RGB), normalised while staging.  A tile's window is 297 pixel quads (row, quad) of 12 bytes,
// at most two per thread; the bytes stay packed in three registers per quad until they are written to the window, where each becomes
// ((float)u / 255.f - mean[c]) / std[c] - or 0.0 where the quad lies outside the image.
struct StemU8 {
    typedef unsigned char Elem;
    typedef StemNorm Norm;
    static constexpr int ALIGN = 4;
    struct Quad { uint32_t w[3]; };
    struct Regs { Quad q[S_QLD]; uint32_t inside; };
    // ((float)u / 255.f - mean) / std.  The first quotient has 256 possible values and a constant divisor: u * RN(1/255) corrected once
    // with its exact remainder equals the IEEE quotient for every byte (tests/test_stem_u8_abi.py proves it in exact rational
    // arithmetic) at 3 instructions instead of a division's 10; the second division is the IEEE one.
    static __device__ __forceinline__ float norm(uint32_t u, float mean, float std) {
        constexpr float R255 = 1.f / 255.f;
        const float f = (float)u;
        float q = __fmul_rn(f, R255);
        q = __builtin_fmaf(__builtin_fmaf(-255.f, q, f), R255, q);
        return (q - mean) / std;
    }
    static __device__ __forceinline__ float tap(const unsigned char* __restrict__ img, const Norm& nm, int n, int c, int ih, int iw, int H, int W) {
        return norm(img[(((long long)n * H + ih) * W + iw) * 3 + c], nm.mean[c], nm.std[c]);
    }
    static __device__ __forceinline__ void load(Regs& reg, const unsigned char* __restrict__ img, int H, int W, int n, int oh0, int ow0, int tid) {
        reg.inside = 0;
#pragma unroll
        for (int j = 0; j < S_QLD; ++j) {
            const int v = tid + 256 * j;
            const int r = v / S_VPR, q = v - r * S_VPR;
            const int ih = 2 * oh0 - 1 + r, iw = 2 * ow0 - 4 + 4 * q;
            Quad t = {{0u, 0u, 0u}};
            if (v < S_QUADS && (unsigned)ih < (unsigned)H && iw >= 0 && iw + 3 < W) {
                t = *reinterpret_cast<const Quad*>(img + (((long long)n * H + ih) * W + iw) * 3);   // 4-byte aligned: W % 4 == 0, iw % 4 == 0
                reg.inside |= 1u << j;
            }
            reg.q[j] = t;
        }
    }
    static __device__ __forceinline__ void write(const Regs& reg, const Norm& nm, float* win, int tid) {
#pragma unroll
        for (int j = 0; j < S_QLD; ++j) {
            const int v = tid + 256 * j;
            if (v < S_QUADS) {
                const int r = v / S_VPR, q = v - r * S_VPR;
                const bool in = (reg.inside >> j) & 1u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    f32x4 t;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int b = 3 * p + c;                                  // byte of pixel p, channel c within the quad
                        const uint32_t u = (reg.q[j].w[b >> 2] >> (8 * (b & 3))) & 0xffu;
                        t[p] = in ? norm(u, nm.mean[c], nm.std[c]) : 0.f;
                    }
                    stem_put_quad(win, c, r, q, t);
                }
            }
        }
    }
};

template <typename Src, typename T>
__global__ __launch_bounds__(256) void stem_conv_kernel(int N, int H, int W, int Ho, int Wo, int Cout,
                                                        const typename Src::Elem* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        T* __restrict__ y, int y_cs, int relu, typename Src::Norm nm) {
    const int co0 = blockIdx.y * 16;
    const long long total = (long long)N * Ho * Wo;
    for (long long pix = blockIdx.x * (long long)blockDim.x + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * blockDim.x) {
        const int ow = (int)(pix % Wo);
        const int oh = (int)((pix / Wo) % Ho);
        const int n = (int)(pix / ((long long)Wo * Ho));
        float in[27];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int ih = oh * 2 - 1 + r, iw = ow * 2 - 1 + s;
                    const bool ok = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
                    // unconditional load from a clamped address + select: all 27 loads are in flight together
                    const int ihc = min(max(ih, 0), H - 1), iwc = min(max(iw, 0), W - 1);
                    const float v = Src::tap(x, nm, n, c, ihc, iwc, H, W);
                    in[(r * 3 + s) * 3 + c] = ok ? v : 0.f;
                }
        float out[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int co = co0 + k;
            float a = 0.f;
            if (co < Cout) {
                const float* wk = w + co * 27;   // [co][r][s][ci], wave-uniform -> scalar loads
#pragma unroll
                for (int j = 0; j < 27; ++j) a = fmaf(in[j], wk[j], a);
                a = a * (scale ? scale[co] : 1.f) + (shift ? shift[co] : 0.f);
                if (relu) a = fmaxf(a, 0.f);
            }
            out[k] = a;
        }
        T* dst = y + pix * y_cs + co0;
        constexpr int VEC = Elem<T>::VEC;
        if (co0 + 16 <= Cout) {
#pragma unroll
            for (int v = 0; v < 16 / VEC; ++v) stg16(dst + v * VEC, Elem<T>::pack(out + v * VEC));
        } else {
            for (int k = 0; k < 16 && co0 + k < Cout; ++k) Elem<T>::store(dst + k, out[k]);
        }
    }
}

// LDS-tiled variant (W % 4 == 0): a block computes a 4 x 64 output tile.  Its 3 x 9 x 132 input window is staged with
// coalesced 16-byte loads - every input pixel is read from global memory once (plus one halo row per four) instead of being
// gathered with stride-2 dword loads by 2 x 9 lanes - and split into even / odd columns so that the stride-2 tap reads of
// neighbouring lanes hit consecutive LDS words.  (A bf16-MFMA formulation - K = 27 taps padded to 32 - was measured slower,
// 43 vs 33 us at 1024x2048: its D fragments leave as 2-byte column stores, and the fp32 products here are exact.)
template <typename Src, typename T>
__global__ __launch_bounds__(256) void stem_lds_kernel(int H, int W, int Ho, int Wo, int Cout, const typename Src::Elem* __restrict__ x,
                                                       const float* __restrict__ w, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, T* __restrict__ y, int y_cs, int relu,
                                                       typename Src::Norm nm) {
    __shared__ __attribute__((aligned(16))) float win[S_WIN];
    const float (*even)[S_ROWS][S_PITCH] = reinterpret_cast<const float (*)[S_ROWS][S_PITCH]>(win);
    const float (*odd)[S_ROWS][S_PITCH] = even + 3;
    const int tid = threadIdx.x;
    const int ow0 = blockIdx.x * S_TW, oh0 = blockIdx.y * S_TH, n = blockIdx.z;
    typename Src::Regs reg;
    Src::load(reg, x, H, W, n, oh0, ow0, tid);
    Src::write(reg, nm, win, tid);
    __syncthreads();
    const int ty = tid / S_TW, tx = tid - ty * S_TW;
    const int oh = oh0 + ty, ow = ow0 + tx;
    if (oh >= Ho || ow >= Wo) return;
    // window column of tap s for output column tx: 2*tx + 3 + s  ->  odd[tx+1], even[tx+2], odd[tx+2]
    float in[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            in[(r * 3 + 0) * 3 + c] = odd[c][2 * ty + r][tx + 1];
            in[(r * 3 + 1) * 3 + c] = even[c][2 * ty + r][tx + 2];
            in[(r * 3 + 2) * 3 + c] = odd[c][2 * ty + r][tx + 2];
        }
    const long long pix = ((long long)n * Ho + oh) * Wo + ow;
    constexpr int VEC = Elem<T>::VEC;
    for (int co0 = 0; co0 < Cout; co0 += 16) {
        float out[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int co = co0 + k;
            float a = 0.f;
            if (co < Cout) {
                const float* wk = w + co * 27;   // [co][r][s][ci], wave-uniform -> scalar loads
#pragma unroll
                for (int j = 0; j < 27; ++j) a = fmaf(in[j], wk[j], a);
                a = a * (scale ? scale[co] : 1.f) + (shift ? shift[co] : 0.f);
                if (relu) a = fmaxf(a, 0.f);
            }
            out[k] = a;
        }
        T* dst = y + pix * y_cs + co0;
        if (co0 + 16 <= Cout) {
#pragma unroll
            for (int v = 0; v < 16 / VEC; ++v) stg16(dst + v * VEC, Elem<T>::pack(out + v * VEC));
        } else {
            for (int k = 0; k < 16 && co0 + k < Cout; ++k) Elem<T>::store(dst + k, out[k]);
        }
    }
}


// ---- MFMA form (bf16 output) ------------------------------------------------------------------------------------------
// The direct form above spends its time on 864 fp32 FMAs per output pixel (0.9 GFLOP at 1024x2048: 31 us, 28 TFLOP/s on
// the vector ALUs) although the layer moves only 59 MB.  Here the 27 taps of a pixel are the K dimension of a 32 x 32 x 32
// GEMM tile (K padded 27 -> 32): M = 32 consecutive output pixels of a row, N = 32 output channels.  Image and filter are
// split into bf16 high and low parts (x = x_hi + x_lo with x_lo = bf16(x - x_hi)) and three MFMAs accumulate
// x_hi*w_hi + x_lo*w_hi + x_hi*w_lo in fp32: the dropped x_lo*w_lo term is 2^-16 relative, so the result matches the
// fp32 direct form to ~1e-5 while the matrix core does all the arithmetic.  Staging (coalesced 16-byte image loads, even /
// odd columns de-interleaved) is the direct kernel's; A fragments are gathered from that window with constant offsets; the
// D fragments go through an LDS transpose so every lane stores 16 bytes (the earlier MFMA attempt mentioned above lost on
// its 2-byte column stores).


struct StemTapOff {
    int off[2][2][8];      // [kk][k-half of the lane][e]: word offset of tap k = kk*16 + half*8 + e relative to the lane's base; -1 = zero pad
};

__host__ __device__ constexpr int stem_tap_offset(int k) {
    // k = (r*3 + s)*3 + c  ->  window word offset (relative to [parity 0][c 0][row 2*ty][col tx]); window = win[2][3][S_ROWS][S_PITCH]
    // tap s of output column tx: s=0 odd[tx+1], s=1 even[tx+2], s=2 odd[tx+2]   (parity 0 = even, 1 = odd)
    return k >= 27 ? -1
                   : ((((k / 3) % 3 == 1) ? 0 : 1) * 3 + (k % 3)) * (S_ROWS * S_PITCH) + ((k / 3) / 3) * S_PITCH + (((k / 3) % 3 == 0) ? 1 : 2);
}

__device__ __forceinline__ void split_bf16(const float (&v)[8], u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = v[2 * i], b = v[2 * i + 1];
        const uint32_t h = pack2_bf16(a, b);
        const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
        hi[i] = h;
        lo[i] = pack2_bf16(ra, rb);
    }
}

// Multi-tile, software-pipelined form.  One 4 x 64 tile per block left a CU with four short serial chains (image loads -> LDS ->
// barrier -> gathers -> MFMA -> transpose -> stores) and every block re-gathered and re-split the same filter.  Now
//   * the grid is at most `4 blocks per compute unit`; block b walks tiles b, b + gridDim.x, ... of a linear order that runs down the
//     rows (ty fastest, then tx, then n) in a plain bounded loop: no tile counter in memory, nothing shared between blocks;
//   * the filter fragments (bh / bl) are loaded and split ONCE per block, before the loop;
//   * the window is double-buffered: the NEXT tile's image loads are issued into registers before the current tile's LDS gathers and
//     MFMAs and written into the other window buffer after them - one __syncthreads() per tile.
// The arithmetic per output is the single-tile kernel's (same operand split, the same three MFMAs per kk in the same order, scale /
// shift / ReLU, one bf16 rounding): outputs are bit-identical to it (tests/test_stem_pipelined_gpu.py, tests/golden/stem_parent.npz).
__device__ __forceinline__ void stem_tile_origin(int t, int tyn, int txn, int& n, int& oh0, int& ow0) {
    const int u = t / tyn;
    n = u / txn;
    oh0 = (t - u * tyn) * S_TH;
    ow0 = (u - n * txn) * S_TW;
}

template <typename Src, int NT, typename TO>                 // n-tiles of 32 output channels: 1 (Cout <= 32) or 2; TO: bf16_t or f16_t output
__global__ __launch_bounds__(256, NT == 1 ? 4 : 3) void stem_mfma_kernel(int N, int H, int W, int Ho, int Wo, int Cout,
                                                        const typename Src::Elem* __restrict__ x,
                                                        const float* __restrict__ w, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, TO* __restrict__ y, int y_cs, int relu,
                                                        typename Src::Norm nm) {
    static_assert(sizeof(TO) == 2, "16-bit output");
    constexpr int OUT_PITCH = 32 * 2 + 16;                   // bytes per pixel row of the transpose tile
    __shared__ __attribute__((aligned(16))) float win[2][S_WIN + 4];     // two window buffers, each + a zero word for the K padding
    __shared__ __attribute__((aligned(16))) unsigned char sout[4][32 * OUT_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
    const int txn = (Wo + S_TW - 1) / S_TW, tyn = (Ho + S_TH - 1) / S_TH;
    const int total = N * txn * tyn;
    int t = blockIdx.x;
    if (t >= total) return;
    int n, oh0, ow0;
    typename Src::Regs reg;
    stem_tile_origin(t, tyn, txn, n, oh0, ow0);
    Src::load(reg, x, H, W, n, oh0, ow0, tid);
    if (tid < 4) win[0][S_WIN + tid] = 0.f;
    else if (tid < 8) win[1][S_WIN + tid - 4] = 0.f;
    // filter fragments of this lane: B[k][n = l31], k = kk*16 + half*8 + e, split like the image - once per block
    u32x4 bh[NT][2], bl[NT][2];                               // [n-tile][kk]
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            float wv[8];
            const int co = nt * 32 + l31;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = kk * 16 + half * 8 + e;
                wv[e] = (co < Cout && k < 27) ? w[co * 27 + k] : 0.f;
            }
            split_bf16(wv, bh[nt][kk], bl[nt][kk]);
        }
    Src::write(reg, nm, win[0], tid);
    __syncthreads();
    // wave = output row `wave` of the tile; m-tile h = columns [32h, 32h + 32)
    const int ty = wave;
    unsigned char* so = sout[wave];
    for (int buf = 0;; buf ^= 1) {
        const int tn = t + (int)gridDim.x;
        const bool more = tn < total;                         // block-uniform
        int nn = 0, noh0 = 0, now0 = 0;
        if (more) {                                           // the next tile's image loads fly during this tile's gathers and MFMAs
            stem_tile_origin(tn, tyn, txn, nn, noh0, now0);
            Src::load(reg, x, H, W, nn, noh0, now0, tid);
        }
        const float* wb = win[buf];
        const int oh = oh0 + ty;
#pragma unroll 1                                              // not unrolled: both m-tiles' 64 gathered taps at once spill
        for (int h = 0; h < 2; ++h) {
            const int tx = 32 * h + l31;
            const float* base = wb + (2 * ty) * S_PITCH + tx;
            u32x4 ah[2], al[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                float av[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int o0 = stem_tap_offset(kk * 16 + e), o1 = stem_tap_offset(kk * 16 + 8 + e);
                    const float* p0 = o0 >= 0 ? base + o0 : wb + S_WIN;
                    const float* p1 = o1 >= 0 ? base + o1 : wb + S_WIN;
                    av[e] = *(half ? p1 : p0);
                }
                split_bf16(av, ah[kk], al[kk]);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al[kk]), __builtin_bit_cast(bf16x8, bh[nt][kk]), acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[kk]), __builtin_bit_cast(bf16x8, bl[nt][kk]), acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah[kk]), __builtin_bit_cast(bf16x8, bh[nt][kk]), acc, 0, 0, 0);
                }
                const int co = nt * 32 + l31;
                const bool cvalid = co < Cout;
                const float sc = (scale && cvalid) ? scale[co] : 1.f, sh = (shift && cvalid) ? shift[co] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int prow = (r & 3) + 8 * (r >> 2) + 4 * half;               // pixel (column) of the m-tile
                    float o = acc[r] * sc + sh;
                    if (relu) o = fmaxf(o, 0.f);
                    Elem<TO>::store(reinterpret_cast<TO*>(so + prow * OUT_PITCH + l31 * 2), o);
                }
                __builtin_amdgcn_wave_barrier();
                const int cbase = nt * 32;
                const int nvalid = Cout - cbase < 32 ? Cout - cbase : 32;                // multiple of 8 (y_cs and Cout are)
#pragma unroll
                for (int ps = 0; ps < 2; ++ps) {                                      // 32 pixels x 4 vectors of 8 channels
                    const int prow = ps * 16 + (lane >> 2), seg = lane & 3;
                    const int ow = ow0 + 32 * h + prow;
                    if (oh < Ho && ow < Wo && seg * 8 < nvalid)
                        stg16(y + (((long long)n * Ho + oh) * Wo + ow) * y_cs + cbase + seg * 8,
                              *reinterpret_cast<const u32x4*>(so + prow * OUT_PITCH + seg * 16));
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (!more) break;
        Src::write(reg, nm, win[buf ^ 1], tid);
        __syncthreads();                                      // the other buffer is complete; every wave is done reading this one
        t = tn; n = nn; oh0 = noh0; ow0 = now0;
    }
}

}  // namespace fs

using namespace fs;

static int g_stem_mfma = 1;
/* test hook: 0 = always the direct (vector-ALU) stem kernel */
extern "C" void fs_debug_stem_mfma(int on) { g_stem_mfma = on; }
static int g_stem_blocks = 0;
static int compute_units() {
    static int cus = 0;
    if (!cus) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
        else cus = 256;
    }
    return cus;
}
/* test hook: 0 = default grid, n > 0 = at most n blocks (every block walks many tiles) */
extern "C" void fs_debug_stem_blocks(int n) { g_stem_blocks = n; }

template <typename Src>
static fs_status stem_launch(const char* name, void* stream, int N, int H, int W, int Cout, const typename Src::Elem* x, const float* w,
                             const float* scale, const float* shift, void* y, int y_cs, int dtype, int relu, typename Src::Norm nm) {
    FS_REQUIRE(x && w && y, FS_ERR_INVALID, "%s: null pointer", name);
    FS_REQUIRE(N > 0 && H > 1 && W > 1 && Cout > 0, FS_ERR_INVALID, "%s: bad shape", name);
    FS_REQUIRE(dtype_ok(dtype), FS_ERR_INVALID, "%s: bad dtype", name);
    FS_REQUIRE(y_cs >= Cout && y_cs % vec_elems(dtype) == 0 && aligned16(y), FS_ERR_INVALID,
               "%s: output slice misaligned (y_cs=%d)", name, y_cs);
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    if (W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & (Src::ALIGN - 1)) == 0 && N <= 65535) {   // LDS-tiled kernels: coalesced quad loads
        dim3 tiles((unsigned)((Wo + S_TW - 1) / S_TW), (unsigned)((Ho + S_TH - 1) / S_TH), (unsigned)N);
        const long long ntile = (long long)tiles.x * tiles.y * tiles.z;
        if (elem_size(dtype) == 2 && Cout <= 64 && Cout % 8 == 0 && g_stem_mfma && ntile < (1ll << 31)) {      // matrix-core form (split-bf16 operands, bf16 or fp16 store)
            // resident blocks per compute unit: 4 x 39.6 KB of LDS at one n-tile; two n-tiles hold twice the filter fragments (3 by registers)
            long long blocks = g_stem_blocks > 0 ? g_stem_blocks : (long long)(Cout <= 32 ? 4 : 3) * compute_units();
            if (blocks > ntile) blocks = ntile;
            if (Cout <= 32)
                FS_DTYPE16_SWITCH(dtype, T, FS_LAUNCH((stem_mfma_kernel<Src, 1, T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, N, H, W,
                                                      Ho, Wo, Cout, x, w, scale, shift, (T*)y, y_cs, relu, nm));
            else
                FS_DTYPE16_SWITCH(dtype, T, FS_LAUNCH((stem_mfma_kernel<Src, 2, T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, N, H, W,
                                                      Ho, Wo, Cout, x, w, scale, shift, (T*)y, y_cs, relu, nm));
            return check_launch(name);
        }
        FS_DTYPE_SWITCH(dtype, T, FS_LAUNCH((stem_lds_kernel<Src, T>), tiles, dim3(256), 0, (hipStream_t)stream, H, W, Ho, Wo, Cout, x, w, scale,
                                            shift, (T*)y, y_cs, relu, nm));
        return check_launch(name);
    }
    const long long total = (long long)N * Ho * Wo;
    long long gx = (total + 255) / 256;
    if (gx > 32768) gx = 32768;
    dim3 grid((unsigned)gx, (Cout + 15) / 16);
    FS_DTYPE_SWITCH(dtype, T, FS_LAUNCH((stem_conv_kernel<Src, T>), grid, dim3(256), 0, (hipStream_t)stream, N, H, W, Ho, Wo, Cout, x, w, scale,
                                        shift, (T*)y, y_cs, relu, nm));
    return check_launch(name);
}

extern "C" fs_status fs_conv_stem_fwd(void* stream, int N, int H, int W, int Cout, const float* x, const float* w,
                                      const float* scale, const float* shift, void* y, int y_cs, int dtype, int relu) {
    return stem_launch<StemF32>("fs_conv_stem_fwd", stream, N, H, W, Cout, x, w, scale, shift, y, y_cs, dtype, relu, StemNoNorm{});
}

static fs_status stem_u8(const char* name, void* stream, int N, int H, int W, int Cout, const unsigned char* img, const float* w,
                         const float* scale, const float* shift, void* y, int y_cs, int dtype, int relu, float mean_r, float mean_g,
                         float mean_b, float std_r, float std_g, float std_b) {
    FS_REQUIRE(std_r != 0.f && std_g != 0.f && std_b != 0.f, FS_ERR_INVALID, "%s: std must be non-zero (%g, %g, %g)", name,
               (double)std_r, (double)std_g, (double)std_b);
    const StemNorm nm = {{mean_r, mean_g, mean_b}, {std_r, std_g, std_b}};
    return stem_launch<StemU8>(name, stream, N, H, W, Cout, img, w, scale, shift, y, y_cs, dtype, relu, nm);
}

// the entry point of ABI 221: fp32 / bf16, as its boundary contract says (any other code, FS_F16 included, is "bad dtype")
extern "C" fs_status fs_conv_stem_u8_fwd(void* stream, int N, int H, int W, int Cout, const unsigned char* img, const float* w,
                                         const float* scale, const float* shift, void* y, int y_cs, int dtype, int relu,
                                         float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b) {
    FS_REQUIRE(std_r != 0.f && std_g != 0.f && std_b != 0.f, FS_ERR_INVALID, "fs_conv_stem_u8_fwd: std must be non-zero (%g, %g, %g)",
               (double)std_r, (double)std_g, (double)std_b);
    // (null pointers and bad shapes keep their messages, which come first)
    FS_REQUIRE(!(img && w && y && N > 0 && H > 1 && W > 1 && Cout > 0) || dtype_train_ok(dtype), FS_ERR_INVALID, "fs_conv_stem_u8_fwd: bad dtype");
    return stem_u8("fs_conv_stem_u8_fwd", stream, N, H, W, Cout, img, w, scale, shift, y, y_cs, dtype, relu, mean_r, mean_g, mean_b, std_r,
                   std_g, std_b);
}

// the same launch for the three storage types: what an inference engine and the program executor issue
extern "C" fs_status fs_conv_stem_u8_infer_fwd(void* stream, int N, int H, int W, int Cout, const unsigned char* img, const float* w,
                                               const float* scale, const float* shift, void* y, int y_cs, int dtype, int relu,
                                               float mean_r, float mean_g, float mean_b, float std_r, float std_g, float std_b) {
    return stem_u8("fs_conv_stem_u8_infer_fwd", stream, N, H, W, Cout, img, w, scale, shift, y, y_cs, dtype, relu, mean_r, mean_g, mean_b,
                   std_r, std_g, std_b);
}
