// 3x3 / stride 1 / pad 1 convolution with an LDS-staged input halo tile (gfx950), NHWC.
//
// The generic implicit-GEMM kernel (conv_igemm.hip) re-gathers every input pixel nine times (once per filter tap)
// from L2.  Here a block owns a TH x 16 patch of output pixels; per chunk of input channels (64 bytes per pixel) it
// stages the (TH+2) x 18 halo patch ONCE into LDS (double buffered, issue-early / write-late) and runs all nine taps
// from it: tap (r,s) is just a constant LDS offset (r*18+s)*pitch on the A-fragment address, so the im2col matrix
// never exists anywhere.  The filter bank does not go through LDS at all: it is pre-packed in MFMA fragment order
// (fs_pack_weight_frag) so each B fragment is one fully coalesced 1 KiB global load straight into registers, kept
// three taps ahead of the MFMAs in a static register ring (the bank is tiny and L2-resident).
// One barrier per channel chunk; 18 * WM_T * WN_T MFMAs per wave between barriers.
// An MFMA m-tile (32 pixels) is 2 image rows x 16 columns.  Epilogue as in conv_igemm: BN-stat partials, scale/shift,
// ReLU, LDS transpose, 16-byte stores into a channel slice.
//
// Further forms (inference epilogue, stride 1):
//  * K-split (conv3x3_halo_ksplit_kernel): on maps of <= 32 x 64 pixels the plain form launches 16-96 blocks on 256 CUs and each
//    block walks every channel chunk in one wave-serial chain.  The K-split block owns ONE m-tile x ONE 32-channel n-tile and its four
//    waves share the channel chunks (wave w: chunks w, w + 4, ..): four times the blocks, a quarter of the chain, every wave fetches
//    only its own filter fragments and stages its own 4 x 18 halo patches (no block barrier in the chunk loop); the four partial
//    accumulators meet in LDS and are summed in wave order, so the result does not depend on timing.  conv3x3_halo_ksplit16_kernel is
//    the same with 16-channel n-tiles (16 x 16 MFMAs): twice the blocks again, for the layers still under half of the CUs.
//  * resample-at-staging (fs_conv_desc.vr_*): the staged pixel is interpolated from a source map of another size (VrTap below), which
//    folds the 1/2 down-sample in front of a zoomed convolution into the convolution.
//
// Replaces the stride-1 3x3 nn.Conv2d calls (+BatchNorm2d/ReLU) of reference search/operations.py:149-152,221-224,
// 298-306,380-388, seg_oprs.py:22 — the layers that carry the FLOPs at >= 128x256 resolution.
#include "common.h"
#include "pack_index.h"

namespace fs {

struct HaloArgs {
    const unsigned char* x;
    const unsigned char* w;     // fragment-packed filter
    unsigned char* y;
    const float* scale;
    const float* shift;
    float* stats;
    int N, H, W, Cin, Cout;
    int Ho, Wo;                 // output size (= H, W at stride 1)
    int x_cs, y_cs;
    int tiles_x, tiles_y, tiles_n, nchunks;
    int flags;
    int vr_H, vr_W, vr_relu;    // resample-at-staging: x is a (vr_H, vr_W) map, the convolution reads its bilinear resampling to (H, W)
    float vr_rh, vr_rw;
};

constexpr int HPITCH = 80;                 // 64 data bytes + 16 pad per halo pixel

// Resample-at-staging (fs_conv_desc.vr_*): a staged halo pixel is the align_corners=True bilinear sample of the (vr_H, vr_W) source,
// computed in fp32 with the arithmetic of fs_bilinear_fwd (resize.hip) and rounded once to the storage type, ReLU after the
// interpolation when vr_relu.  Every input pixel is staged once per channel chunk, so the four source reads are paid once per
// pixel and chunk (the implicit GEMM pays them per tap).  Offsets are bytes inside one image (the host checks that they fit an int).
struct VrTap {
    int o00, o01, o10, o11;
    float lh, lw;
};
template <typename T> __device__ __forceinline__ VrTap vr_make_tap(const HaloArgs& p, int iy, int ix, int c) {
    const Tap th = make_tap(p.vr_rh, iy, p.vr_H), tw = make_tap(p.vr_rw, ix, p.vr_W);
    VrTap t;
    t.o00 = ((th.i0 * p.vr_W + tw.i0) * p.x_cs + c) * (int)sizeof(T);
    t.o01 = ((th.i0 * p.vr_W + tw.i1) * p.x_cs + c) * (int)sizeof(T);
    t.o10 = ((th.i1 * p.vr_W + tw.i0) * p.x_cs + c) * (int)sizeof(T);
    t.o11 = ((th.i1 * p.vr_W + tw.i1) * p.x_cs + c) * (int)sizeof(T);
    t.lh = th.l1;
    t.lw = tw.l1;
    return t;
}
template <typename T> __device__ __forceinline__ u32x4 vr_sample(const unsigned char* img, const VrTap& t, bool relu) {
    constexpr int VEC = Elem<T>::VEC;
    float p00[VEC], p01[VEC], p10[VEC], p11[VEC];
    Elem<T>::unpack(ldg16(img + t.o00), p00);
    Elem<T>::unpack(ldg16(img + t.o01), p01);
    Elem<T>::unpack(ldg16(img + t.o10), p10);
    Elem<T>::unpack(ldg16(img + t.o11), p11);
    const float h1 = t.lh, h0 = 1.f - h1, w1 = t.lw, w0 = 1.f - w1;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const float o = h0 * (w0 * p00[e] + w1 * p01[e]) + h1 * (w0 * p10[e] + w1 * p11[e]);
        p00[e] = relu ? fmaxf(o, 0.f) : o;
    }
    return Elem<T>::pack(p00);
}

// STRIDE 2: the block's 8 x 16 OUTPUT pixels read a 17 x 33 input patch.  It is staged with its even and odd columns
// de-interleaved (LDS column = (hx & 1) * 17 + hx / 2), so that tap s of 16 consecutive output columns is again 16
// consecutive LDS pixels (s = 0: even columns ox, s = 1: odd columns ox, s = 2: even columns ox + 1) and the A-fragment
// reads stay conflict-free; the patch is 45 KB per channel chunk, so it is single-buffered (the chunk loop of these layers
// is 1-2 iterations long: Cin = 32 / 64).
template <typename T, int WAVES_M, int WAVES_N, int WM_T, int WN_T, int STRIDE = 1, bool VRES = false>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(HaloArgs p) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr int CK = 4 * VEC;                           // input channels per chunk (64 bytes)
    constexpr int TH = 2 * WAVES_M * WM_T;                // output rows per block
    constexpr int HALO_W = 15 * STRIDE + 3;               // input columns of the patch: 18 / 33
    constexpr int HALO_H = (TH - 1) * STRIDE + 3;
    constexpr int NBUF = STRIDE == 1 ? 2 : 1;
    constexpr int EVEN_COLS = 17;                         // stride 2: columns 0, 2, .., 32 come first, then 1, 3, .., 31
    constexpr int HALO_PIX = HALO_H * HALO_W;
    constexpr int HALO_VECS = HALO_PIX * 4;
    constexpr int A_ITEMS = (HALO_VECS + 255) / 256;
    constexpr int HALO_BYTES = HALO_PIX * HPITCH;
    constexpr int OUT_PITCH = 32 * (int)sizeof(T) + 16;
    constexpr int OUT_BYTES = 4 * 32 * OUT_PITCH;
    constexpr int SMEM = cmax(NBUF * HALO_BYTES, OUT_BYTES);
    static_assert(WAVES_M * WAVES_N == 4, "4 waves per block");
    static_assert(!VRES || STRIDE == 1, "resample-at-staging: stride 1 only");
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    int b = blockIdx.x;
    const int tn = b % p.tiles_n; b /= p.tiles_n;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y;
    const int img = b / p.tiles_y;
    const int y0 = ty * TH, x0 = tx * 16;
    const int n0 = tn * (WAVES_N * WN_T * 32);

    // ---- halo staging map: vector v -> (halo pixel, 16-byte slot) -------------------------------------
    long long a_off[A_ITEMS];
    VrTap a_tap[VRES ? A_ITEMS : 1];
    uint32_t a_keep[A_ITEMS];
    int a_lds[A_ITEMS];
    const unsigned char* ximg = p.x + (long long)img * p.vr_H * p.vr_W * p.x_cs * (long long)sizeof(T);   // VRES: this image of the source map
    const bool vr_relu = VRES && p.vr_relu != 0;
#pragma unroll
    for (int i = 0; i < A_ITEMS; ++i) {
        const int v = tid + i * 256;
        const int pix = v >> 2, slot = v & 3;
        const int hy = pix / HALO_W, hx = pix - hy * HALO_W;
        const int iy = STRIDE * y0 - 1 + hy, ix = STRIDE * x0 - 1 + hx;
        // VRES: (iy, ix) address the RESAMPLED map, whose border the zero padding applies to
        const bool ok = (v < HALO_VECS) && ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
        a_keep[i] = ok ? 0xffffffffu : 0u;
        if constexpr (VRES) {
            a_tap[i] = vr_make_tap<T>(p, ok ? iy : 0, ok ? ix : 0, slot * VEC);
            a_off[i] = 0ll;
        } else {
            a_off[i] = ok ? ((((long long)img * p.H + iy) * p.W + ix) * p.x_cs + slot * VEC) * (long long)sizeof(T) : 0ll;
        }
        const int lcol = STRIDE == 1 ? hx : (hx & 1) * EVEN_COLS + (hx >> 1);
        a_lds[i] = (v < HALO_VECS) ? (hy * HALO_W + lcol) * HPITCH + slot * 16 : -1;
    }
    u32x4 a_reg[A_ITEMS];
    uint32_t a_cmask[A_ITEMS];
    auto load_halo = [&](int chunk) {
        const int c0 = chunk * CK;
#pragma unroll
        for (int i = 0; i < A_ITEMS; ++i) {
            const int slot = (tid + i * 256) & 3;
            const bool cok = (c0 + slot * VEC) < p.Cin;        // channel tail of the last chunk reads zeros
            a_cmask[i] = cok ? a_keep[i] : 0u;
            if constexpr (VRES) a_reg[i] = vr_sample<T>(ximg + (cok ? c0 * (int)sizeof(T) : 0), a_tap[i], vr_relu);
            else a_reg[i] = ldg16(p.x + (cok ? a_off[i] + (long long)c0 * sizeof(T) : 0ll));
        }
    };
    auto store_halo = [&](int buf) {
#pragma unroll
        for (int i = 0; i < A_ITEMS; ++i) {
            if (a_lds[i] >= 0) {
                u32x4 v = a_reg[i];
                const uint32_t k = a_cmask[i];
                v[0] &= k; v[1] &= k; v[2] &= k; v[3] &= k;
                *reinterpret_cast<u32x4*>(smem + buf * HALO_BYTES + a_lds[i]) = v;
            }
        }
    };

    // ---- filter fragments: [n_tile][chunk][tap][kk][lane] x 16 bytes ------------------------------------
    const unsigned char* wbase[WN_T];
#pragma unroll
    for (int j = 0; j < WN_T; ++j) {
        const int nt = (n0 >> 5) + wn * WN_T + j;
        wbase[j] = p.w + ((long long)nt * p.nchunks * 18) * 1024 + lane * 16;
    }
    u32x4 bring[3][2][WN_T];                               // ring of three taps
    auto load_b = [&](int slot, int chunk, int tap) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < WN_T; ++j)
                bring[slot][kk][j] = ldg16(wbase[j] + ((long long)(chunk * 9 + tap) * 2 + kk) * 1024);
    };

    f32x16 acc[WM_T][WN_T];
#pragma unroll
    for (int i = 0; i < WM_T; ++i)
#pragma unroll
        for (int j = 0; j < WN_T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    float ep_sc[WN_T], ep_sh[WN_T];
#pragma unroll
    for (int j = 0; j < WN_T; ++j) {
        const int co = n0 + (wn * WN_T + j) * 32 + (lane & 31);
        const bool cvalid = co < p.Cout;
        ep_sc[j] = (p.scale && cvalid) ? p.scale[co] : 1.f;
        ep_sh[j] = (p.shift && cvalid) ? p.shift[co] : 0.f;
    }

    // A fragment base: m-tile i of this wave covers halo rows (wm*WM_T + i)*2 + {0,1}, columns 0..15
    const int l31 = lane & 31;
    const int frag_base = (STRIDE * ((wm * WM_T) * 2 + (l31 >> 4)) * HALO_W + (l31 & 15)) * HPITCH + (lane >> 5) * 16;

    load_halo(0);
    load_b(0, 0, 0);
    load_b(1, 0, 1);
    load_b(2, 0, 2);
    store_halo(0);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        const int buf = NBUF == 2 ? (c & 1) : 0;
        const bool more = (c + 1) < p.nchunks;
        if (more) load_halo(c + 1);
        const unsigned char* hal = smem + buf * HALO_BYTES + frag_base;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const int slot = tap % 3;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                u32x4 af[WM_T];
#pragma unroll
                for (int i = 0; i < WM_T; ++i)
                    af[i] = *reinterpret_cast<const u32x4*>(hal + ((STRIDE * i * 2 + r) * HALO_W + (STRIDE == 1 ? s : (s & 1) * EVEN_COLS + (s >> 1))) * HPITCH + kk * 32);
#pragma unroll
                for (int i = 0; i < WM_T; ++i)
#pragma unroll
                    for (int j = 0; j < WN_T; ++j) Mma<T>::run(af[i], bring[slot][kk][j], acc[i][j]);
            }
            // refill this ring slot with the tap three steps ahead (wraps into the next chunk)
            if (tap < 6) load_b(slot, c, tap + 3);
            else if (more) load_b(slot, c + 1, tap - 6);
        }
        if (NBUF == 1 && more) __syncthreads();          // single buffer: every wave is done reading before it is refilled
        if (more) store_halo(NBUF == 2 ? (buf ^ 1) : 0);
        __syncthreads();
    }

    // ---- epilogue -----------------------------------------------------------------------------------------
    const bool relu = (p.flags & FS_CONV_RELU) != 0;
    const bool scalar_store = (p.flags & CONV_SCALAR_STORE) != 0;
    T* y = reinterpret_cast<T*>(p.y);
    unsigned char* sOut = smem + wave * 32 * OUT_PITCH;
    constexpr int LPR = 32 * (int)sizeof(T) / 16;
    constexpr int RPP = 64 / LPR;
#pragma unroll
    for (int j = 0; j < WN_T; ++j) {
        const int cbase = n0 + (wn * WN_T + j) * 32;
        const int co = cbase + l31;
        const bool cvalid = co < p.Cout;
        const float sc = ep_sc[j], sh = ep_sh[j];
        const bool full_n = (cbase + 32 <= p.Cout) && !scalar_store;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < WM_T; ++i) {
            const int row0 = y0 + (wm * WM_T + i) * 2;
            if (full_n) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int prow = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);     // pixel index in the m-tile
                    const int oy = row0 + (prow >> 4), ox = x0 + (prow & 15);
                    const bool pv = oy < p.Ho && ox < p.Wo;
                    const float v = pv ? acc[i][j][r] : 0.f;
                    s1 += v;
                    s2 += v * v;
                    float o = v * sc + sh;
                    if (relu) o = fmaxf(o, 0.f);
                    Elem<T>::store(reinterpret_cast<T*>(sOut + prow * OUT_PITCH) + l31, o);
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int ps = 0; ps < 32 / RPP; ++ps) {
                    const int prow = ps * RPP + lane / LPR;
                    const int seg = lane % LPR;
                    const int oy = row0 + (prow >> 4), ox = x0 + (prow & 15);
                    if (oy < p.Ho && ox < p.Wo)
                        stg16(y + (((long long)img * p.Ho + oy) * p.Wo + ox) * p.y_cs + cbase + seg * (16 / (int)sizeof(T)),
                              *reinterpret_cast<const u32x4*>(sOut + prow * OUT_PITCH + seg * 16));
                }
                __builtin_amdgcn_wave_barrier();
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int prow = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    const int oy = row0 + (prow >> 4), ox = x0 + (prow & 15);
                    const bool pv = oy < p.Ho && ox < p.Wo;
                    const float v = pv ? acc[i][j][r] : 0.f;
                    s1 += v;
                    s2 += v * v;
                    if (pv && cvalid) {
                        float o = v * sc + sh;
                        if (relu) o = fmaxf(o, 0.f);
                        Elem<T>::store(y + (((long long)img * p.Ho + oy) * p.Wo + ox) * p.y_cs + co, o);
                    }
                }
            }
        }
        if (p.stats) {
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (lane < 32 && cvalid) {
                atomicAdd(p.stats + co, s1);
                atomicAdd(p.stats + p.Cout + co, s2);
            }
        }
    }
}

// K-split form, stride 1, inference epilogue (no BN statistics).  One block = one m-tile (2 rows x 16 columns) x one 32-channel
// n-tile; wave w contracts the channel chunks w, w + 4, w + 8, .. (a wave without a chunk contributes zeros, the channel tail of the
// last chunk is staged as zeros).  Each wave stages the 4 x 18 halo patch of ITS chunk into its own double-buffered LDS region and
// reads only its own filter fragments, so the chunk loop needs no block barrier: LDS operations of one wave complete in order.
// Then the four accumulators go to LDS as [wave][register][lane] and wave w finishes accumulator registers 4w .. 4w+3 (pixels
// 8w .. 8w+7 of the tile): partials added in wave order 0, 1, 2, 3 - a fixed order, two runs give the same bits.
constexpr int KS_HALO_W = 18, KS_HALO_H = 4;
constexpr int KS_VECS = KS_HALO_H * KS_HALO_W * 4;        // 288 16-byte vectors per chunk patch
constexpr int KS_ITEMS = (KS_VECS + 63) / 64;             // per lane
constexpr int KS_BYTES = KS_HALO_H * KS_HALO_W * HPITCH;  // 5760
constexpr int KS_PART_BYTES = 4 * 16 * 64 * 4;            // the four partial accumulators

template <typename T, bool VRES>
__global__ __launch_bounds__(256) void conv3x3_halo_ksplit_kernel(HaloArgs p) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr int CK = 4 * VEC;
    constexpr int OUT_PITCH = 32 * (int)sizeof(T) + 16;
    constexpr int SMEM = cmax(4 * 2 * KS_BYTES, KS_PART_BYTES + 32 * OUT_PITCH);
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int tn = b % p.tiles_n; b /= p.tiles_n;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y;
    const int img = b / p.tiles_y;
    const int y0 = ty * 2, x0 = tx * 16;
    const int cbase = tn * 32;

    // ---- this wave's staging map: vector v -> (halo pixel, 16-byte slot) ------------------------------------------------
    long long a_off[KS_ITEMS];
    VrTap a_tap[VRES ? KS_ITEMS : 1];
    uint32_t a_keep[KS_ITEMS];
    int a_lds[KS_ITEMS];
    const unsigned char* ximg = p.x + (long long)img * p.vr_H * p.vr_W * p.x_cs * (long long)sizeof(T);   // VRES: this image of the source map
    const bool vr_relu = VRES && p.vr_relu != 0;
#pragma unroll
    for (int i = 0; i < KS_ITEMS; ++i) {
        const int v = lane + i * 64;
        const int pix = v >> 2, slot = v & 3;
        const int hy = pix / KS_HALO_W, hx = pix - hy * KS_HALO_W;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = (v < KS_VECS) && ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
        a_keep[i] = ok ? 0xffffffffu : 0u;
        if constexpr (VRES) {
            a_tap[i] = vr_make_tap<T>(p, ok ? iy : 0, ok ? ix : 0, slot * VEC);
            a_off[i] = 0ll;
        } else {
            a_off[i] = ok ? ((((long long)img * p.H + iy) * p.W + ix) * p.x_cs + slot * VEC) * (long long)sizeof(T) : 0ll;
        }
        a_lds[i] = (v < KS_VECS) ? pix * HPITCH + slot * 16 : -1;
    }
    u32x4 a_reg[KS_ITEMS];
    uint32_t a_cmask[KS_ITEMS];
    auto load_halo = [&](int chunk) {
        const int c0 = chunk * CK;
#pragma unroll
        for (int i = 0; i < KS_ITEMS; ++i) {
            const int slot = (lane + i * 64) & 3;
            const bool cok = (c0 + slot * VEC) < p.Cin;        // channel tail of the last chunk reads zeros
            a_cmask[i] = cok ? a_keep[i] : 0u;
            if constexpr (VRES) a_reg[i] = vr_sample<T>(ximg + (cok ? c0 * (int)sizeof(T) : 0), a_tap[i], vr_relu);
            else a_reg[i] = ldg16(p.x + (cok ? a_off[i] + (long long)c0 * sizeof(T) : 0ll));
        }
    };
    unsigned char* wsm = smem + wave * 2 * KS_BYTES;           // this wave's two patch buffers
    auto store_halo = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KS_ITEMS; ++i) {
            if (a_lds[i] >= 0) {
                u32x4 v = a_reg[i];
                const uint32_t k = a_cmask[i];
                v[0] &= k; v[1] &= k; v[2] &= k; v[3] &= k;
                *reinterpret_cast<u32x4*>(wsm + buf * KS_BYTES + a_lds[i]) = v;
            }
        }
    };
    // the wave's own LDS writes become visible to its own later reads: in-order LDS, the fence only stops the compiler
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    // ---- filter fragments of this n-tile: [n_tile][chunk][tap][kk][lane] x 16 bytes ---------------------------------------
    const unsigned char* wbase = p.w + ((long long)tn * p.nchunks * 18) * 1024 + lane * 16;
    u32x4 bring[3][2];
    auto load_b = [&](int slot, int chunk, int tap) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) bring[slot][kk] = ldg16(wbase + ((long long)(chunk * 9 + tap) * 2 + kk) * 1024);
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const int l31 = lane & 31;
    const int co = cbase + l31;
    const bool cvalid = co < p.Cout;
    const float sc = (p.scale && cvalid) ? p.scale[co] : 1.f;
    const float sh = (p.shift && cvalid) ? p.shift[co] : 0.f;
    const int frag_base = ((l31 >> 4) * KS_HALO_W + (l31 & 15)) * HPITCH + (lane >> 5) * 16;

    int c = wave;
    if (c < p.nchunks) {
        load_halo(c);
        load_b(0, c, 0);
        load_b(1, c, 1);
        load_b(2, c, 2);
        store_halo(0);
        wave_sync();
    }
    int buf = 0;
    for (; c < p.nchunks; c += 4) {
        const bool more = (c + 4) < p.nchunks;
        if (more) load_halo(c + 4);
        const unsigned char* hal = wsm + buf * KS_BYTES + frag_base;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const int slot = tap % 3;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const u32x4 af = *reinterpret_cast<const u32x4*>(hal + (r * KS_HALO_W + s) * HPITCH + kk * 32);
                Mma<T>::run(af, bring[slot][kk], acc);
            }
            if (tap < 6) load_b(slot, c, tap + 3);
            else if (more) load_b(slot, c + 4, tap - 6);
        }
        if (more) store_halo(buf ^ 1);                   // last read by this wave one iteration ago
        wave_sync();
        buf ^= 1;
    }

    // ---- the four partial accumulators meet in LDS ----------------------------------------------------------------------------
    __syncthreads();                                     // every wave is done with its patch buffers
    float* part = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(wave * 16 + r) * 64 + lane] = acc[r];
    __syncthreads();
    float fin[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = wave * 4 + q;
        fin[q] = ((part[(0 * 16 + r) * 64 + lane] + part[(1 * 16 + r) * 64 + lane]) + part[(2 * 16 + r) * 64 + lane]) + part[(3 * 16 + r) * 64 + lane];
    }

    // ---- epilogue: wave w owns pixels 8w .. 8w+7 of the tile (accumulator registers 4w .. 4w+3) -------------------------------
    const bool relu = (p.flags & FS_CONV_RELU) != 0;
    const bool scalar_store = (p.flags & CONV_SCALAR_STORE) != 0;
    T* y = reinterpret_cast<T*>(p.y);
    unsigned char* sOut = smem + KS_PART_BYTES;            // rows of different waves are disjoint
    constexpr int LPR = 32 * (int)sizeof(T) / 16;        // lanes per pixel row of 32 channels
    const bool full_n = (cbase + 32 <= p.Cout) && !scalar_store;
    if (full_n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int prow = q + 8 * wave + 4 * (lane >> 5);
            float o = fin[q] * sc + sh;
            if (relu) o = fmaxf(o, 0.f);
            Elem<T>::store(reinterpret_cast<T*>(sOut + prow * OUT_PITCH) + l31, o);
        }
        wave_sync();
        const int pr = lane / LPR, seg = lane % LPR;
        if (pr < 8) {
            const int prow = 8 * wave + pr;
            const int oy = y0 + (prow >> 4), ox = x0 + (prow & 15);
            if (oy < p.Ho && ox < p.Wo)
                stg16(y + (((long long)img * p.Ho + oy) * p.Wo + ox) * p.y_cs + cbase + seg * (16 / (int)sizeof(T)),
                      *reinterpret_cast<const u32x4*>(sOut + prow * OUT_PITCH + seg * 16));
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int prow = q + 8 * wave + 4 * (lane >> 5);
            const int oy = y0 + (prow >> 4), ox = x0 + (prow & 15);
            if (oy < p.Ho && ox < p.Wo && cvalid) {
                float o = fin[q] * sc + sh;
                if (relu) o = fmaxf(o, 0.f);
                Elem<T>::store(y + (((long long)img * p.Ho + oy) * p.Wo + ox) * p.y_cs + co, o);
            }
        }
    }
}

// K-split form with a 16-channel n-tile: the same block and wave roles, but the tile is 2 rows x 16 columns x SIXTEEN output channels,
// contracted with the 16 x 16 MFMAs (two m-subtiles of one image row each).  Twice the blocks of the 32-channel K-split form for the
// layers that one still leaves under half of the CUs (128->128 on a 16 x 32 map: 64 -> 128 blocks).  The filter bank is the same
// fragment pack: lane l needs output channel c = cbase + (l & 15) and the l >> 4 = g-th 16-byte group of the chunk's input channels,
// which the pack holds at [c >> 5][chunk][tap][kk = g >> 1][lane (g & 1) * 32 + (c & 31)] - one 16-byte load per tap.
template <typename T> struct Mma16;
template <> struct Mma16<float> {
    static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[j]), __uint_as_float(b[j]), c, 0, 0, 0);
    }
};
template <> struct Mma16<bf16_t> {
    static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mma16<f16_t> {
    static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

template <typename T, bool VRES>
__global__ __launch_bounds__(256) void conv3x3_halo_ksplit16_kernel(HaloArgs p) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr int CK = 4 * VEC;
    constexpr int OUT_PITCH = 16 * (int)sizeof(T) + 16;
    constexpr int PART_BYTES = 4 * 8 * 64 * 4;               // four waves x 8 accumulator registers
    constexpr int SMEM = cmax(4 * 2 * KS_BYTES, PART_BYTES + 32 * OUT_PITCH);
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int b = blockIdx.x;
    const int tn = b % p.tiles_n; b /= p.tiles_n;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y;
    const int img = b / p.tiles_y;
    const int y0 = ty * 2, x0 = tx * 16;
    const int cbase = tn * 16;

    // ---- this wave's staging map (as in conv3x3_halo_ksplit_kernel) ---------------------------------------------------------
    long long a_off[KS_ITEMS];
    VrTap a_tap[VRES ? KS_ITEMS : 1];
    uint32_t a_keep[KS_ITEMS];
    int a_lds[KS_ITEMS];
    const unsigned char* ximg = p.x + (long long)img * p.vr_H * p.vr_W * p.x_cs * (long long)sizeof(T);
    const bool vr_relu = VRES && p.vr_relu != 0;
#pragma unroll
    for (int i = 0; i < KS_ITEMS; ++i) {
        const int v = lane + i * 64;
        const int pix = v >> 2, slot = v & 3;
        const int hy = pix / KS_HALO_W, hx = pix - hy * KS_HALO_W;
        const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
        const bool ok = (v < KS_VECS) && ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
        a_keep[i] = ok ? 0xffffffffu : 0u;
        if constexpr (VRES) {
            a_tap[i] = vr_make_tap<T>(p, ok ? iy : 0, ok ? ix : 0, slot * VEC);
            a_off[i] = 0ll;
        } else {
            a_off[i] = ok ? ((((long long)img * p.H + iy) * p.W + ix) * p.x_cs + slot * VEC) * (long long)sizeof(T) : 0ll;
        }
        a_lds[i] = (v < KS_VECS) ? pix * HPITCH + slot * 16 : -1;
    }
    u32x4 a_reg[KS_ITEMS];
    uint32_t a_cmask[KS_ITEMS];
    auto load_halo = [&](int chunk) {
        const int c0 = chunk * CK;
#pragma unroll
        for (int i = 0; i < KS_ITEMS; ++i) {
            const int slot = (lane + i * 64) & 3;
            const bool cok = (c0 + slot * VEC) < p.Cin;
            a_cmask[i] = cok ? a_keep[i] : 0u;
            if constexpr (VRES) a_reg[i] = vr_sample<T>(ximg + (cok ? c0 * (int)sizeof(T) : 0), a_tap[i], vr_relu);
            else a_reg[i] = ldg16(p.x + (cok ? a_off[i] + (long long)c0 * sizeof(T) : 0ll));
        }
    };
    unsigned char* wsm = smem + wave * 2 * KS_BYTES;
    auto store_halo = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KS_ITEMS; ++i) {
            if (a_lds[i] >= 0) {
                u32x4 v = a_reg[i];
                const uint32_t k = a_cmask[i];
                v[0] &= k; v[1] &= k; v[2] &= k; v[3] &= k;
                *reinterpret_cast<u32x4*>(wsm + buf * KS_BYTES + a_lds[i]) = v;
            }
        }
    };
    auto wave_sync = [&]() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    const int l15 = lane & 15, g = lane >> 4;
    const int co = cbase + l15;
    const bool cvalid = co < p.Cout;
    const unsigned char* wbase = p.w + ((long long)(co >> 5) * p.nchunks * 18) * 1024 + (g >> 1) * 1024 + ((g & 1) * 32 + (co & 31)) * 16;
    u32x4 bring[3];
    auto load_b = [&](int slot, int chunk, int tap) { bring[slot] = ldg16(wbase + (long long)(chunk * 9 + tap) * 2048); };

    f32x4 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;

    const float sc = (p.scale && cvalid) ? p.scale[co] : 1.f;
    const float sh = (p.shift && cvalid) ? p.shift[co] : 0.f;
    const int frag_base = l15 * HPITCH + g * 16;             // m-subtile i: halo row i + r, column l15 + s, 16-byte group g

    int c = wave;
    if (c < p.nchunks) {
        load_halo(c);
        load_b(0, c, 0);
        load_b(1, c, 1);
        load_b(2, c, 2);
        store_halo(0);
        wave_sync();
    }
    int buf = 0;
    for (; c < p.nchunks; c += 4) {
        const bool more = (c + 4) < p.nchunks;
        if (more) load_halo(c + 4);
        const unsigned char* hal = wsm + buf * KS_BYTES + frag_base;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const int slot = tap % 3;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const u32x4 af = *reinterpret_cast<const u32x4*>(hal + ((i + r) * KS_HALO_W + s) * HPITCH);
                Mma16<T>::run(af, bring[slot], acc[i]);
            }
            if (tap < 6) load_b(slot, c, tap + 3);
            else if (more) load_b(slot, c + 4, tap - 6);
        }
        if (more) store_halo(buf ^ 1);
        wave_sync();
        buf ^= 1;
    }

    // ---- partial accumulators: [wave][register 0..7][lane]; wave w finishes registers 2w, 2w+1 (fixed order 0, 1, 2, 3) ------
    __syncthreads();
    float* part = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(wave * 8 + i * 4 + r) * 64 + lane] = acc[i][r];
    __syncthreads();
    float fin[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = wave * 2 + q;
        fin[q] = ((part[(0 * 8 + k) * 64 + lane] + part[(1 * 8 + k) * 64 + lane]) + part[(2 * 8 + k) * 64 + lane]) + part[(3 * 8 + k) * 64 + lane];
    }

    // ---- epilogue: register k = i * 4 + r of lane (l15, g) is pixel (row i, column g * 4 + r), channel cbase + l15; wave w owns
    //      row w >> 1, columns g * 4 + 2 * (w & 1) + {0, 1}: 8 pixels x 16 channels -------------------------------------------------
    const bool relu = (p.flags & FS_CONV_RELU) != 0;
    const bool scalar_store = (p.flags & CONV_SCALAR_STORE) != 0;
    T* y = reinterpret_cast<T*>(p.y);
    unsigned char* sOut = smem + PART_BYTES;
    const int oy = y0 + (wave >> 1);
    const bool full_n = (cbase + 16 <= p.Cout) && !scalar_store;
    if (full_n) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int prow = wave * 8 + g * 2 + q;           // this wave's 8 pixels: g * 2 + q <-> column g * 4 + 2 * (wave & 1) + q
            float o = fin[q] * sc + sh;
            if (relu) o = fmaxf(o, 0.f);
            Elem<T>::store(reinterpret_cast<T*>(sOut + prow * OUT_PITCH) + l15, o);
        }
        wave_sync();
        constexpr int LPR = 16 * (int)sizeof(T) / 16;      // 16-byte segments per pixel: 2 (bf16) / 4 (fp32)
        const int pr = lane / LPR, seg = lane % LPR;
        if (pr < 8) {
            const int ox = x0 + (pr >> 1) * 4 + 2 * (wave & 1) + (pr & 1);
            if (oy < p.Ho && ox < p.Wo)
                stg16(y + (((long long)img * p.Ho + oy) * p.Wo + ox) * p.y_cs + cbase + seg * (16 / (int)sizeof(T)),
                      *reinterpret_cast<const u32x4*>(sOut + (wave * 8 + pr) * OUT_PITCH + seg * 16));
        }
    } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ox = x0 + g * 4 + 2 * (wave & 1) + q;
            if (oy < p.Ho && ox < p.Wo && cvalid) {
                float o = fin[q] * sc + sh;
                if (relu) o = fmaxf(o, 0.f);
                Elem<T>::store(y + (((long long)img * p.Ho + oy) * p.Wo + ox) * p.y_cs + co, o);
            }
        }
    }
}

// fragment-order filter pack: out[n_tile][chunk][tap][kk][lane][VEC] with
//   cout = n_tile*32 + (lane&31), cin = chunk*CK + kk*(CK/2) + (lane>>5)*VEC + e   (zero outside the bank)
template <typename T>
__global__ void pack_weight_frag_kernel(const float* __restrict__ w, long long o_stride, long long i_stride, int Cout, int Cin,
                                        int nchunks, long long total, T* __restrict__ out) {
    for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long src = pack_frag_src_offset<Elem<T>::VEC>(idx, o_stride, i_stride, Cout, Cin, nchunks);
        const float v = src >= 0 ? w[src] : 0.f;
        Elem<T>::store(out + idx, v);
    }
}

template <typename T, int WAVES_M, int WAVES_N, int WM_T, int WN_T, int STRIDE = 1, bool VRES = false>
static void launch_halo(hipStream_t st, HaloArgs& a) {
    constexpr int TH = 2 * WAVES_M * WM_T;
    constexpr int BN = WAVES_N * WN_T * 32;
    a.tiles_x = (a.Wo + 15) / 16;
    a.tiles_y = (a.Ho + TH - 1) / TH;
    a.tiles_n = (a.Cout + BN - 1) / BN;
    const long long blocks = (long long)a.N * a.tiles_y * a.tiles_x * a.tiles_n;
    FS_LAUNCH((conv3x3_halo_kernel<T, WAVES_M, WAVES_N, WM_T, WN_T, STRIDE, VRES>), dim3((unsigned)blocks), dim3(256), 0, st, a);
}

template <typename T, bool VRES> static void launch_halo_ksplit(hipStream_t st, HaloArgs& a, int ntile) {
    a.tiles_x = (a.Wo + 15) / 16;
    a.tiles_y = (a.Ho + 1) / 2;
    a.tiles_n = (a.Cout + ntile - 1) / ntile;
    const long long blocks = (long long)a.N * a.tiles_y * a.tiles_x * a.tiles_n;
    if (ntile == 16) FS_LAUNCH((conv3x3_halo_ksplit16_kernel<T, VRES>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    else FS_LAUNCH((conv3x3_halo_ksplit_kernel<T, VRES>), dim3((unsigned)blocks), dim3(256), 0, st, a);
}

// The launch form of a layer (host only; fs_conv3x3_halo_plan exports it).
//  Output-channel tile of the plain form: 32, 64 or 128 per block (always 8 x 16 pixels).  `force_tile` (FS_CONV_TILE_* in
//  fs_conv_desc.flags) picks one; otherwise the widest tile that wastes no half-empty channel block AND still gives every CU a block:
//  a 192->128 layer on a 64 x 128 map is 64 blocks of 128 channels (a quarter of the chip, 21.8 us) but 256 blocks of 32.
//  K-split form (2 x 16 pixels x 32 channels per block, the four waves share the channel chunks): chosen when even the 32-channel
//  plain tile would launch fewer than half of the 256 CUs and there are at least two chunks to share; stride 1 and no BN statistics
//  only (a training call never selects it).  Where that still leaves fewer than 128 blocks, its 16-channel form (tile = 16).
//  `force_ks`: 0 decide here, 1 K-split with 32-channel tiles, 2 with 16-channel tiles, -1 plain.
struct HaloPlan {
    int tile, ksplit;
    long long workgroups;
};
static HaloPlan plan_halo(int N, int Ho, int Wo, int Cout, int nchunks, int stride, int force_tile, int force_ks, bool has_stats) {
    const long long pix_tiles = (long long)N * ((Ho + 7) / 8) * ((Wo + 15) / 16);
    HaloPlan pl;
    int tile = force_tile;
    if (tile == 0) {
        if (Cout <= 32) tile = 32;
        else if (Cout <= 64 || (Cout % 128 != 0 && Cout % 128 <= 64)) tile = 64;
        else tile = 128;
        while (tile > 32 && pix_tiles * ((Cout + tile - 1) / tile) < 256) tile >>= 1;
    }
    pl.tile = tile;
    pl.workgroups = pix_tiles * ((Cout + tile - 1) / tile);
    const bool can = stride == 1 && !has_stats;
    pl.ksplit = 0;
    if (force_ks > 0) pl.ksplit = can ? 1 : -1;          // -1: the forced form does not exist for this call
    else if (force_ks == 0 && force_tile == 0 && can && nchunks >= 2 && pix_tiles * ((Cout + 31) / 32) < 128) pl.ksplit = 1;
    if (pl.ksplit == 1) {
        const long long m_tiles = (long long)N * ((Ho + 1) / 2) * ((Wo + 15) / 16);
        pl.tile = force_ks == 2 || (force_ks == 0 && m_tiles * ((Cout + 31) / 32) < 128) ? 16 : 32;
        pl.workgroups = m_tiles * ((Cout + pl.tile - 1) / pl.tile);
    }
    return pl;
}

template <typename T> static void dispatch_halo(hipStream_t st, HaloArgs& a, const HaloPlan& pl, int stride) {
    const int tile = pl.tile;
    const bool vres = a.vr_H > 0;
    if (pl.ksplit == 1) {
        if (vres) launch_halo_ksplit<T, true>(st, a, tile);
        else launch_halo_ksplit<T, false>(st, a, tile);
        return;
    }
    if (stride == 2) {
        if (tile == 32) launch_halo<T, 4, 1, 1, 1, 2>(st, a);
        else if (tile == 64) launch_halo<T, 2, 2, 2, 1, 2>(st, a);
        else launch_halo<T, 2, 2, 2, 2, 2>(st, a);
        return;
    }
    if (vres) {
        if (tile == 32) launch_halo<T, 4, 1, 1, 1, 1, true>(st, a);
        else if (tile == 64) launch_halo<T, 2, 2, 2, 1, 1, true>(st, a);
        else launch_halo<T, 2, 2, 2, 2, 1, true>(st, a);
        return;
    }
    if (tile == 32) launch_halo<T, 4, 1, 1, 1>(st, a);             // 8x16 px x 32 ch
    else if (tile == 64) launch_halo<T, 2, 2, 2, 1>(st, a);        // 8x16 x 64
    else launch_halo<T, 2, 2, 2, 2>(st, a);                        // 8x16 x 128
}

static int force_tile_of(int flags) {
    return (flags & FS_CONV_TILE_MASK) == FS_CONV_TILE_32 ? 32 : (flags & FS_CONV_TILE_MASK) == FS_CONV_TILE_64 ? 64
           : (flags & FS_CONV_TILE_MASK) == FS_CONV_TILE_128 ? 128 : 0;
}
static int force_ks_of(int flags) {
    return (flags & FS_CONV_KSPLIT16) == FS_CONV_KSPLIT16 ? 2 : (flags & FS_CONV_KSPLIT) ? 1 : (flags & FS_CONV_NO_KSPLIT) ? -1 : 0;
}

}  // namespace fs

using namespace fs;

extern "C" long long fs_packed_weight_frag_elems(int Cout, int Cin, int dtype) {
    return pack_frag_elems(Cout, Cin, vec_elems(dtype));
}

extern "C" fs_status fs_pack_weight_frag(void* stream, const float* w, long long o_stride, long long i_stride, int Cout, int Cin,
                                         int dtype, void* out) {
    FS_REQUIRE(w && out && Cout > 0 && Cin > 0, FS_ERR_INVALID, "fs_pack_weight_frag: bad argument");
    FS_REQUIRE(dtype_ok(dtype), FS_ERR_INVALID, "fs_pack_weight_frag: bad dtype");
    const int vec = vec_elems(dtype), ck = 4 * vec;
    const int nchunks = (Cin + ck - 1) / ck;
    const long long total = fs_packed_weight_frag_elems(Cout, Cin, dtype);
    long long g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    FS_DTYPE_SWITCH(dtype, T, FS_LAUNCH((pack_weight_frag_kernel<T>), dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, w, o_stride,
                                        i_stride, Cout, Cin, nchunks, total, (T*)out));
    return check_launch("fs_pack_weight_frag");
}

extern "C" fs_status fs_conv3x3_halo_plan(const fs_conv_desc* d, int has_stats, int* tile, int* ksplit, long long* workgroups) {
    FS_REQUIRE(d && dtype_ok(d->dtype) && d->N > 0 && d->Ho > 0 && d->Wo > 0 && d->Cin > 0 && d->Cout > 0 &&
                   (d->stride == 1 || d->stride == 2),
               FS_ERR_INVALID, "fs_conv3x3_halo_plan: bad descriptor");
    FS_REQUIRE((d->flags & (FS_CONV_KSPLIT | FS_CONV_NO_KSPLIT)) != (FS_CONV_KSPLIT | FS_CONV_NO_KSPLIT), FS_ERR_INVALID,
               "fs_conv3x3_halo_plan: FS_CONV_KSPLIT and FS_CONV_NO_KSPLIT exclude each other");
    const int ck = 4 * vec_elems(d->dtype);
    const HaloPlan pl = plan_halo(d->N, d->Ho, d->Wo, d->Cout, (d->Cin + ck - 1) / ck, d->stride, force_tile_of(d->flags), force_ks_of(d->flags),
                                  has_stats != 0);
    FS_REQUIRE(pl.ksplit >= 0, FS_ERR_UNSUPPORTED, "fs_conv3x3_halo_plan: the K-split form is stride 1 without BN statistics only");
    if (tile) *tile = pl.tile;
    if (ksplit) *ksplit = pl.ksplit;
    if (workgroups) *workgroups = pl.workgroups;
    return FS_OK;
}

extern "C" fs_status fs_conv3x3_s1_fwd(void* stream, const fs_conv_desc* d, const void* x, const void* w_frag, const float* scale,
                                       const float* shift, void* y, float* stats) {
    FS_REQUIRE(d && x && w_frag && y, FS_ERR_INVALID, "fs_conv3x3_s1_fwd: null argument");
    FS_REQUIRE(dtype_ok(d->dtype), FS_ERR_INVALID, "fs_conv3x3_s1_fwd: bad dtype");
    FS_REQUIRE(d->dtype != FS_F16 || !stats, FS_ERR_UNSUPPORTED, "fs_conv3x3_s1_fwd: FS_F16 is inference only (no BN statistics)");
    FS_REQUIRE(d->R == 3 && d->S == 3 && (d->stride == 1 || d->stride == 2) && d->pad == 1 && d->Ho == (d->H - 1) / d->stride + 1 &&
                   d->Wo == (d->W - 1) / d->stride + 1 && !(d->flags & ~(FS_CONV_RELU | FS_CONV_TILE_MASK | FS_CONV_KSPLIT16 | FS_CONV_NO_KSPLIT)),
               FS_ERR_UNSUPPORTED, "fs_conv3x3_s1_fwd: only 3x3 / stride 1 or 2 / pad 1 (got %dx%d s%d p%d)", d->R, d->S, d->stride, d->pad);
    FS_REQUIRE((d->flags & (FS_CONV_KSPLIT | FS_CONV_NO_KSPLIT)) != (FS_CONV_KSPLIT | FS_CONV_NO_KSPLIT), FS_ERR_INVALID,
               "fs_conv3x3_s1_fwd: FS_CONV_KSPLIT and FS_CONV_NO_KSPLIT exclude each other");
    const int vec = vec_elems(d->dtype);
    FS_REQUIRE(d->Cin % vec == 0 && d->x_cs % vec == 0 && d->x_cs >= d->Cin && d->y_cs >= d->Cout, FS_ERR_INVALID,
               "fs_conv3x3_s1_fwd: bad channel counts/strides");
    FS_REQUIRE(aligned16(x) && aligned16(w_frag), FS_ERR_INVALID, "fs_conv3x3_s1_fwd: operands must be 16-byte aligned");
    HaloArgs a;
    a.x = (const unsigned char*)x; a.w = (const unsigned char*)w_frag; a.y = (unsigned char*)y;
    a.scale = scale; a.shift = shift; a.stats = stats;
    a.N = d->N; a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout;
    a.Ho = d->Ho; a.Wo = d->Wo;
    a.x_cs = d->x_cs; a.y_cs = d->y_cs;
    a.nchunks = (d->Cin + 4 * vec - 1) / (4 * vec);
    a.flags = d->flags & FS_CONV_RELU;
    a.vr_H = a.vr_W = a.vr_relu = 0;
    a.vr_rh = a.vr_rw = 0.f;
    if (d->vr_H > 0 || d->vr_W > 0) {          // resample-at-staging: down- and up-sampling alike, the taps are ATen's for any size pair
        FS_REQUIRE(d->vr_H > 0 && d->vr_W > 0, FS_ERR_INVALID, "fs_conv3x3_s1_fwd: bad virtual-resize source size %dx%d", d->vr_H, d->vr_W);
        FS_REQUIRE(d->stride == 1, FS_ERR_UNSUPPORTED, "fs_conv3x3_s1_fwd: a resampled input needs stride 1");
        FS_REQUIRE((long long)d->vr_H * d->vr_W * d->x_cs * elem_size(d->dtype) < (1ll << 31), FS_ERR_UNSUPPORTED,
                   "fs_conv3x3_s1_fwd: resampled source image too large");
        a.vr_H = d->vr_H; a.vr_W = d->vr_W; a.vr_relu = d->vr_relu ? 1 : 0;
        a.vr_rh = d->H > 1 ? (float)(d->vr_H - 1) / (float)(d->H - 1) : 0.f;      // ATen: scale = (in-1)/(out-1), 0 when out == 1
        a.vr_rw = d->W > 1 ? (float)(d->vr_W - 1) / (float)(d->W - 1) : 0.f;
    }
    const HaloPlan pl = plan_halo(d->N, d->Ho, d->Wo, d->Cout, a.nchunks, d->stride, force_tile_of(d->flags), force_ks_of(d->flags), stats != nullptr);
    FS_REQUIRE(pl.ksplit >= 0, FS_ERR_UNSUPPORTED, "fs_conv3x3_s1_fwd: the K-split form is stride 1 without BN statistics only");
    if (!(aligned16(y) && (d->y_cs % vec == 0))) a.flags |= CONV_SCALAR_STORE;
    FS_CENSUS(FS_CENSUS_CONV_HALO | (stats ? FS_CENSUS_STATS : 0), d);
    FS_DTYPE_SWITCH(d->dtype, T, dispatch_halo<T>((hipStream_t)stream, a, pl, d->stride));
    return check_launch("fs_conv3x3_s1_fwd");
}
