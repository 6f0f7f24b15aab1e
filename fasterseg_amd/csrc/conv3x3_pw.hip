// 3x3 / stride 1 / pad 1 LDS-halo convolution with the pointwise (1x1) convolution behind it in the same launch, inference epilogues,
// NHWC, 16-bit storage types (bf16, fp16; gfx950).
//
// The tail of every derived network ends in heads.conv_3x3 -> heads.conv_1x1 (model_seg.py:345, seg_oprs.py Head), and an arm of
// `_arm_up_refine` (model_seg.py:322-334) is a 3x3 whose only eval-mode reader is a 1x1.  As separate launches the 3x3's map is written
// once and read once by the next launch; here it never leaves the CU:
//
//   3x3   as conv3x3_halo_kernel with a 128-channel tile (the block owns every output channel of its TH x 16 pixels): the halo patch
//         staged per channel chunk, double-buffered, nine taps as constant LDS offsets, the fragment-packed filter
//         (fs_pack_weight_frag) in a three-tap register ring - the summation order of the stand-alone launch.
//   1x1   scale / shift / ReLU, rounded to the storage type exactly where the stand-alone launch stores it, to LDS as the A operand of
//         the pointwise GEMM (dense [Cout][C3] pack of fs_pack_weight, N padded to whole 32-channel tiles, rows >= Cout read as zero
//         and never stored), then scale / shift (or bias) and the store.  Pad channels of a wider pixel stride (the 19-class logits in
//         a 32-channel stride) are not written, as fs_conv2d_fwd does not write them.
//
// TH = 8 (WM_T = 2) or 4 (WM_T = 1) rows per block: 8 x 16 is the stand-alone kernel's tile, 4 x 16 doubles the blocks on maps where
// 8 x 16 leaves CUs without a second block (or without any).
//
// A form with a 1x1 in FRONT of the 3x3 as well (the halo patch of the 1x1's output computed into LDS) was built and measured: it cost
// ~10 us where the stand-alone 1x1 costs 9.7, and is not kept.
#include "common.h"

namespace fs {

struct PwArgs {
    const unsigned char* x;
    const unsigned char* w3;    // fragment-packed 3x3 filter Cmid -> C3
    const float* sc3;
    const float* sh3;
    const unsigned char* w2;    // 1x1: dense [Cpost][C3]
    const float* sc2;
    const float* sh2;
    unsigned char* y;
    int N, H, W;
    int Cmid, C3, Cpost;
    int x_cs, y_cs;
    int tiles_x, tiles_y, nchunks;   // nchunks: 32-channel chunks of Cmid
    int relu3, relu2, scalar_store;
};

constexpr int PW_PITCH = 80;           // 64 data bytes + 16 pad per pixel and channel chunk (HPITCH of conv3x3_halo.hip)
constexpr int PW_HALO_W = 18;

template <typename T, int WM_T>
__global__ __launch_bounds__(256) void conv3x3_pw_kernel(PwArgs p) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr int CK = 4 * VEC;                           // channels per chunk (64 bytes)
    constexpr int WN_T = 2;                               // 2 x 2 waves, each 2 n-tiles: 128 output channels per block
    constexpr int TH = 4 * WM_T;                          // output rows per block
    constexpr int HALO_H = TH + 2;
    constexpr int HALO_PIX = HALO_H * PW_HALO_W;
    constexpr int HALO_VECS = HALO_PIX * 4;
    constexpr int A_ITEMS = (HALO_VECS + 255) / 256;
    constexpr int HALO_BYTES = HALO_PIX * PW_PITCH;
    constexpr int MAXCH = 4;                              // chunks of the 1x1's contraction: C3 <= 128
    constexpr int TPIX = TH * 16;
    constexpr int T_BYTES = MAXCH * TPIX * PW_PITCH;
    constexpr int IN_BYTES = 2 * HALO_BYTES;
    constexpr int MAIN_BYTES = cmax(IN_BYTES, T_BYTES);
    constexpr int OUT_PITCH = 32 * (int)sizeof(T) + 16;
    constexpr int OUT_BYTES = 4 * 32 * OUT_PITCH;
    __shared__ __attribute__((aligned(16))) unsigned char smem[MAIN_BYTES + OUT_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int l31 = lane & 31, hi = lane >> 5;
    int b = blockIdx.x;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y;
    const int img = b / p.tiles_y;
    const int y0 = ty * TH, x0 = tx * 16;

    // ---- filter fragments of the 3x3: [n_tile][chunk][tap][kk][lane] x 16 bytes (whole 128-channel block tiles, zero outside the bank)
    const unsigned char* wbase[WN_T];
#pragma unroll
    for (int j = 0; j < WN_T; ++j) wbase[j] = p.w3 + ((long long)(wn * WN_T + j) * p.nchunks * 18) * 1024 + lane * 16;
    u32x4 bring[3][2][WN_T];
    auto load_b = [&](int slot, int chunk, int tap) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < WN_T; ++j)
                bring[slot][kk][j] = ldg16(wbase[j] + ((long long)(chunk * 9 + tap) * 2 + kk) * 1024);
    };

    // ---- staging: the halo patch of x, one chunk at a time (as conv3x3_halo_kernel) ------------------------------------------------------
    long long a_off[A_ITEMS];
    uint32_t a_keep[A_ITEMS];
    int a_lds[A_ITEMS];
    u32x4 a_reg[A_ITEMS];
    uint32_t a_cmask[A_ITEMS];
    {
#pragma unroll
        for (int i = 0; i < A_ITEMS; ++i) {
            const int v = tid + i * 256;
            const int pix = v >> 2, slot = v & 3;
            const int hy = pix / PW_HALO_W, hx = pix - hy * PW_HALO_W;
            const int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
            const bool ok = (v < HALO_VECS) && ((unsigned)iy < (unsigned)p.H) && ((unsigned)ix < (unsigned)p.W);
            a_keep[i] = ok ? 0xffffffffu : 0u;
            a_off[i] = ok ? ((((long long)img * p.H + iy) * p.W + ix) * p.x_cs + slot * VEC) * (long long)sizeof(T) : 0ll;
            a_lds[i] = (v < HALO_VECS) ? pix * PW_PITCH + slot * 16 : -1;
        }
    }
    auto load_halo = [&](int chunk) {
        const int c0 = chunk * CK;
#pragma unroll
        for (int i = 0; i < A_ITEMS; ++i) {
            const int slot = (tid + i * 256) & 3;
            const bool cok = (c0 + slot * VEC) < p.Cmid;       // channel tail of the last chunk reads zeros
            a_cmask[i] = cok ? a_keep[i] : 0u;
            a_reg[i] = ldg16(p.x + (cok ? a_off[i] + (long long)c0 * sizeof(T) : 0ll));
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

    // Everything the phases behind the chunk loop read from global memory is requested here, so that its (cold, in the frame) latency
    // passes under the 3x3: the 3x3's scale / shift, and the 1x1's filter fragments and scale / shift of this wave's first unit.
    float ep_sc[WN_T], ep_sh[WN_T];
#pragma unroll
    for (int j = 0; j < WN_T; ++j) {
        const int co = (wn * WN_T + j) * 32 + l31;
        const bool cvalid = co < p.C3;
        ep_sc[j] = (p.sc3 && cvalid) ? p.sc3[co] : 1.f;
        ep_sh[j] = (p.sh3 && cvalid) ? p.sh3[co] : 0.f;
    }
    constexpr int MT2 = TH / 2;                           // units of the 1x1: (32 pixels) x (32 output channels), wave w takes w, w + 4, ..
    const int units = MT2 * ((p.Cpost + 31) >> 5);
    u32x4 fb[MAXCH][2];
    float sc2 = 1.f, sh2 = 0.f;
    auto load_unit = [&](int u) {
        const int co = (u / MT2) * 32 + l31;
        const bool cvalid = co < p.Cpost;
        const unsigned char* bp = p.w2 + (cvalid ? (long long)co * p.C3 * (long long)sizeof(T) : 0ll);
#pragma unroll
        for (int c = 0; c < MAXCH; ++c)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int ci = c * CK + kk * (CK / 2) + hi * VEC;
                const uint32_t kb = (cvalid && ci < p.C3) ? 0xffffffffu : 0u;
                u32x4 w = ldg16(bp + (kb ? ci * (int)sizeof(T) : 0));
                w[0] &= kb; w[1] &= kb; w[2] &= kb; w[3] &= kb;
                fb[c][kk] = w;
            }
        sc2 = (p.sc2 && cvalid) ? p.sc2[co] : 1.f;
        sh2 = (p.sh2 && cvalid) ? p.sh2[co] : 0.f;
    };
    load_unit(wave < units ? wave : 0);

    load_halo(0);
    load_b(0, 0, 0);
    load_b(1, 0, 1);
    load_b(2, 0, 2);
    store_halo(0);
    __syncthreads();

    // ---- 3x3 ------------------------------------------------------------------------------------------------------------------------
    f32x16 acc[WM_T][WN_T];
#pragma unroll
    for (int i = 0; i < WM_T; ++i)
#pragma unroll
        for (int j = 0; j < WN_T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // A fragment base: m-tile i of this wave covers halo rows (wm*WM_T + i)*2 + {0,1}, columns 0..15
    const int frag_base = (((wm * WM_T) * 2 + (l31 >> 4)) * PW_HALO_W + (l31 & 15)) * PW_PITCH + hi * 16;
    for (int c = 0; c < p.nchunks; ++c) {
        const bool more = (c + 1) < p.nchunks;
        if (more) load_halo(c + 1);
        const unsigned char* hal = smem + (c & 1) * HALO_BYTES + frag_base;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int r = tap / 3, s = tap - r * 3;
            const int slot = tap % 3;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                u32x4 af[WM_T];
#pragma unroll
                for (int i = 0; i < WM_T; ++i)
                    af[i] = *reinterpret_cast<const u32x4*>(hal + ((i * 2 + r) * PW_HALO_W + s) * PW_PITCH + kk * 32);
#pragma unroll
                for (int i = 0; i < WM_T; ++i)
#pragma unroll
                    for (int j = 0; j < WN_T; ++j) Mma<T>::run(af[i], bring[slot][kk][j], acc[i][j]);
            }
            if (tap < 6) load_b(slot, c, tap + 3);
            else if (more) load_b(slot, c + 1, tap - 6);
        }
        if (more) store_halo((c & 1) ^ 1);
        __syncthreads();
    }

    T* y = reinterpret_cast<T*>(p.y);
    unsigned char* sOut = smem + MAIN_BYTES + wave * 32 * OUT_PITCH;
    constexpr int LPR = 32 * (int)sizeof(T) / 16;
    constexpr int RPP = 64 / LPR;

    {
        // ---- 1x1: t[chunk][pixel] = round_T(relu?(scale3 * acc + shift3)), then y = relu?(scale2 * (W2 . t) + shift2) ----------------------
        // (the chunk loop ended in a barrier: every wave is done with the halo patch the t image overwrites)
#pragma unroll
        for (int j = 0; j < WN_T; ++j) {
            const int nt = wn * WN_T + j;
            const int co = nt * 32 + l31;
            const bool cvalid = co < p.C3;
            const float sc = ep_sc[j], sh = ep_sh[j];
#pragma unroll
            for (int i = 0; i < WM_T; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pt = (wm * WM_T + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    float o = acc[i][j][r] * sc + sh;
                    if (p.relu3) o = fmaxf(o, 0.f);
                    if (!cvalid) o = 0.f;
                    Elem<T>::store(reinterpret_cast<T*>(smem + (nt * TPIX + pt) * PW_PITCH) + l31, o);
                }
        }
        __syncthreads();
        const int nch3 = (p.C3 + CK - 1) / CK;
        for (int u = wave; u < units; u += 4) {
            const int mt = u % MT2, nt = u / MT2;
            const int cbase = nt * 32;
            const int co = cbase + l31;
            const bool cvalid = co < p.Cpost;
            if (u != wave) load_unit(u);
            f32x16 acc2;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
            const unsigned char* ta = smem + (mt * 32 + l31) * PW_PITCH + hi * 16;
#pragma unroll
            for (int c = 0; c < MAXCH; ++c) {
                if (c < nch3) {
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const u32x4 a = *reinterpret_cast<const u32x4*>(ta + c * TPIX * PW_PITCH + kk * 32);
                        Mma<T>::run(a, fb[c][kk], acc2);
                    }
                }
            }
            const float sc = sc2, sh = sh2;
            const bool full_n = (cbase + 32 <= p.Cpost) && !p.scalar_store;
            const int row0 = y0 + mt * 2;
            if (full_n) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int prow = (r & 3) + 8 * (r >> 2) + 4 * hi;
                    float o = acc2[r] * sc + sh;
                    if (p.relu2) o = fmaxf(o, 0.f);
                    Elem<T>::store(reinterpret_cast<T*>(sOut + prow * OUT_PITCH) + l31, o);
                }
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int ps = 0; ps < 32 / RPP; ++ps) {
                    const int prow = ps * RPP + lane / LPR;
                    const int seg = lane % LPR;
                    const int oy = row0 + (prow >> 4), ox = x0 + (prow & 15);
                    if (oy < p.H && ox < p.W)
                        stg16(y + (((long long)img * p.H + oy) * p.W + ox) * p.y_cs + cbase + seg * (16 / (int)sizeof(T)),
                              *reinterpret_cast<const u32x4*>(sOut + prow * OUT_PITCH + seg * 16));
                }
                __builtin_amdgcn_wave_barrier();
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int prow = (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const int oy = row0 + (prow >> 4), ox = x0 + (prow & 15);
                    if (oy < p.H && ox < p.W && cvalid) {
                        float o = acc2[r] * sc + sh;
                        if (p.relu2) o = fmaxf(o, 0.f);
                        Elem<T>::store(y + (((long long)img * p.H + oy) * p.W + ox) * p.y_cs + co, o);
                    }
                }
            }
        }
    }
}

template <typename T, int WM_T> static void launch_pw(hipStream_t st, PwArgs& a) {
    constexpr int TH = 4 * WM_T;
    a.tiles_x = (a.W + 15) / 16;
    a.tiles_y = (a.H + TH - 1) / TH;
    const dim3 grid((unsigned)((long long)a.N * a.tiles_y * a.tiles_x));
    FS_LAUNCH((conv3x3_pw_kernel<T, WM_T>), grid, dim3(256), 0, st, a);
}

// Rows per block (host only; fs_conv3x3_pw_plan exports it): FS_PW_ROWS4 / FS_PW_ROWS8 in the flags pin it, otherwise 8 rows where
// that still gives every one of the 256 CUs a block, else 4.
static int plan_pw_rows(const fs_conv_pw_desc* d) {
    if ((d->flags & FS_PW_ROWS_MASK) == FS_PW_ROWS4) return 4;
    if ((d->flags & FS_PW_ROWS_MASK) == FS_PW_ROWS8) return 8;
    const long long blocks8 = (long long)d->N * ((d->H + 7) / 8) * ((d->W + 15) / 16);
    return blocks8 >= 256 ? 8 : 4;
}

static fs_status check_pw(const fs_conv_pw_desc* d, const char* who) {
    FS_REQUIRE(d, FS_ERR_INVALID, "%s: null descriptor", who);
    FS_REQUIRE(dtype_ok(d->dtype), FS_ERR_INVALID, "%s: bad dtype %d", who, d->dtype);
    FS_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Cin > 0 && d->C3 > 0 && d->Cout > 0, FS_ERR_INVALID,
               "%s: bad geometry N%d %dx%d channels %d -> %d -> %d", who, d->N, d->H, d->W, d->Cin, d->C3, d->Cout);
    FS_REQUIRE(!(d->flags & ~(FS_PW_RELU_3X3 | FS_PW_RELU_POST | FS_PW_ROWS_MASK)), FS_ERR_INVALID, "%s: unknown flags 0x%x", who, d->flags);
    FS_REQUIRE((d->flags & FS_PW_ROWS_MASK) != FS_PW_ROWS_MASK, FS_ERR_INVALID, "%s: FS_PW_ROWS4 and FS_PW_ROWS8 exclude each other", who);
    FS_REQUIRE(elem_size(d->dtype) == 2, FS_ERR_UNSUPPORTED, "%s: 16-bit storage types only (FS_BF16 / FS_F16; before FS_F16: bf16 only) - fp32 keeps the separate launches", who);
    const int vec = vec_elems(d->dtype);
    FS_REQUIRE(d->Cin % vec == 0 && d->x_cs % vec == 0 && d->x_cs >= d->Cin && d->y_cs >= d->Cout, FS_ERR_INVALID,
               "%s: bad channel counts/strides (Cin %d, x_cs %d, y_cs %d)", who, d->Cin, d->x_cs, d->y_cs);
    FS_REQUIRE(d->C3 <= 128 && d->C3 % vec == 0, FS_ERR_UNSUPPORTED,
               "%s: the block owns every 3x3 output channel: C3 <= 128 and a multiple of %d (got %d)", who, vec, d->C3);
    FS_REQUIRE(d->Cout <= 128, FS_ERR_UNSUPPORTED, "%s: Cout %d > 128", who, d->Cout);
    FS_REQUIRE((long long)d->N * ((d->H + 3) / 4) * ((d->W + 15) / 16) < (1ll << 31), FS_ERR_UNSUPPORTED, "%s: too many tiles", who);
    return FS_OK;
}

}  // namespace fs

using namespace fs;

extern "C" fs_status fs_conv3x3_pw_plan(const fs_conv_pw_desc* d, int* rows, long long* workgroups, int* lds_bytes) {
    const fs_status st = check_pw(d, "fs_conv3x3_pw_plan");
    if (st != FS_OK) return st;
    const int th = plan_pw_rows(d);
    if (rows) *rows = th;
    if (workgroups) *workgroups = (long long)d->N * ((d->H + th - 1) / th) * ((d->W + 15) / 16);
    if (lds_bytes) *lds_bytes = cmax(2 * (th + 2) * PW_HALO_W * PW_PITCH, 4 * th * 16 * PW_PITCH) + 4 * 32 * 80;
    return FS_OK;
}

extern "C" fs_status fs_conv3x3_pw_fwd(void* stream, const fs_conv_pw_desc* d, const void* x, const void* w_frag, const float* scale,
                                       const float* shift, const void* w_post, const float* scale_post, const float* shift_post, void* y) {
    const fs_status st = check_pw(d, "fs_conv3x3_pw_fwd");
    if (st != FS_OK) return st;
    FS_REQUIRE(x && w_frag && w_post && y, FS_ERR_INVALID, "fs_conv3x3_pw_fwd: null argument");
    FS_REQUIRE(aligned16(x) && aligned16(w_frag) && aligned16(w_post), FS_ERR_INVALID, "fs_conv3x3_pw_fwd: operands must be 16-byte aligned");
    const int vec = vec_elems(d->dtype);
    PwArgs a;
    a.x = (const unsigned char*)x;
    a.w3 = (const unsigned char*)w_frag; a.sc3 = scale; a.sh3 = shift;
    a.w2 = (const unsigned char*)w_post; a.sc2 = scale_post; a.sh2 = shift_post;
    a.y = (unsigned char*)y;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.Cmid = d->Cin; a.C3 = d->C3; a.Cpost = d->Cout;
    a.x_cs = d->x_cs; a.y_cs = d->y_cs;
    a.nchunks = (d->Cin + 4 * vec - 1) / (4 * vec);
    a.relu3 = (d->flags & FS_PW_RELU_3X3) != 0;
    a.relu2 = (d->flags & FS_PW_RELU_POST) != 0;
    a.scalar_store = !(aligned16(y) && (d->y_cs % vec == 0));
    if (plan_pw_rows(d) == 8) FS_DTYPE16_SWITCH(d->dtype, T, launch_pw<T, 2>((hipStream_t)stream, a));
    else FS_DTYPE16_SWITCH(d->dtype, T, launch_pw<T, 1>((hipStream_t)stream, a));
    return check_launch("fs_conv3x3_pw_fwd");
}
