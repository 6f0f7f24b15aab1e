// OHEM hard-example selection and the class-weighted loss reduction on the device (fs_ohem_select, ABI 217).
//
// Between the per-pixel forward (fs_ohem_ce_fwd / fs_ohem_ce_up_fwd: true_prob, nll) and the backward, ProbOhemCrossEntropy2d
// (reference tools/seg_opr/loss_opr.py:66-93) needs the k-th smallest true-class probability of the batch, the kept mask and the mean
// of the kept pixels' nll - with class weights (loss_opr.py:51-58) the mean weighted by w[target].  The unweighted criterion does this
// with a device sort of the B*H*W probabilities and about a dozen ATen launches.  Here:
//
//   clear     one block     zeroes the three histograms and the valid counter (a kernel, not a memset node: DESIGN.md capture note)
//   hist<0>   bits 31..21   histogram of the top 11 bits of every true_prob (2048 bins), counts the valid pixels
//   hist<1>   bits 20..10   prologue: every block scans histogram 0 for the bin that holds rank k (block 0 records it); histogram of the
//                           next 11 bits over the elements of that bin
//   hist<2>   bits  9..0    prologue: scan of histogram 1 narrows the prefix to 22 bits; histogram of the last 10 bits
//   emit                    prologue: scan of histogram 2 -> the exact k-th pattern; threshold = max(thresh, kth), apply; writes
//                           coef[p] = kept ? w[target] : 0 and per-block fp64 partials of sum coef, sum coef * nll and the two counts
//   final     one block     sums the partials in a fixed order -> result, counts
//
// A most-significant-digit-first radix select: non-negative floats order as their unsigned bit patterns, so after three passes the
// prefix IS the k-th smallest value, bit for bit what torch.sort(true_prob).values[k - 1] gives.  Any other pattern (NaN, negative)
// orders by its bits; every bin index is a masked bit field, so nothing indexes out of range whatever the input.  Histograms are
// block-private in LDS (32-bit integer atomics, with one round of wave aggregation because most probabilities share a few exponent
// bins) and flushed with 64-bit integer atomics; the float sums use no atomics at all, so two runs give identical bits.  Six launches
// (two when min_kept == 0: emit + final), nothing read back.  true_prob, nll and coef go 16 bytes per lane over the 16-byte aligned
// body of the vectors with a scalar head and tail; where the three pointers are not equally aligned the emit pass reads by element.
#include "common.h"

namespace fs {

constexpr int SEL_BINS = 2048;                  // 11-bit digits (the last pass uses 1024 of them)
constexpr int SEL_MAX_BLOCKS = 2048;            // 8 blocks per CU; the rest of P is a grid-stride loop
constexpr int SEL_MAXC = 20;

struct SelPartial {                             // one per emit block
    double den, num;
    long long valid, kept;
};
struct SelWs {                                  // layout of the caller's workspace
    unsigned long long hist[3][SEL_BINS];
    unsigned long long n_valid;
    unsigned long long pad;
    unsigned long long state[2][2];             // after pass 0 / 1: {prefix bits found so far, rank that remains inside that prefix}
    SelPartial part[1];                         // [blocks]
};

static inline unsigned sel_blocks(long long P) {
    long long b = (P + 1023) / 1024;            // four elements per lane
    return (unsigned)(b > SEL_MAX_BLOCKS ? SEL_MAX_BLOCKS : (b < 1 ? 1 : b));
}

__global__ __launch_bounds__(256) void ohem_select_clear_kernel(SelWs* __restrict__ ws) {
    unsigned long long* h = &ws->hist[0][0];
    for (int i = threadIdx.x; i < 3 * SEL_BINS; i += 256) h[i] = 0ull;
    if (threadIdx.x == 0) ws->n_valid = 0ull;
}

// sums over the block in a fixed order (lanes by xor butterfly, then waves 0..3); valid in every thread
template <typename V>
__device__ __forceinline__ V sel_block_sum(V v, V* sh4) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                            // sh4 of an earlier call has been read
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// Every thread of the block learns the bin of `hist` (2048 counts) that holds 0-based rank `r`, and r minus the counts below that bin.
// sc: 2 x 256 scratch, out: 2 words.  A rank beyond the total (cannot happen: the bin the previous pass chose holds it) picks bin 0.
__device__ __forceinline__ void sel_find_bin(const unsigned long long* __restrict__ hist, unsigned long long r, unsigned long long (*sc)[256],
                                             unsigned long long* out, unsigned& bin, unsigned long long& rem) {
    const int t = threadIdx.x;
    unsigned long long c[8], s = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        c[i] = hist[t * 8 + i];
        s += c[i];
    }
    if (t == 0) {
        out[0] = 0ull;
        out[1] = 0ull;
    }
    sc[0][t] = s;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int off = 1; off < 256; off <<= 1) {   // inclusive Hillis-Steele scan of the 256 group sums
        const unsigned long long v = sc[cur][t] + (t >= off ? sc[cur][t - off] : 0ull);
        sc[cur ^ 1][t] = v;
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long incl = sc[cur][t], excl = incl - s;
    if (r >= excl && r < incl) {                // exactly one thread
        unsigned long long below = excl;
        unsigned b = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {           // walk the group's bins while the rank lies above them (r < incl: it ends inside bin 7 at most)
            if (b == (unsigned)i && r >= below + c[i]) {
                below += c[i];
                b = i + 1;
            }
        }
        out[0] = (unsigned long long)(t * 8 + b);
        out[1] = r - below;
    }
    __syncthreads();
    bin = (unsigned)out[0] & (SEL_BINS - 1);
    rem = out[1];
    __syncthreads();                            // sc / out may be reused
}

// count `bin` in the block's LDS histogram; the lanes that share the first live lane's bin add once (pass 0: a few exponent bins
// hold almost every probability, and same-address LDS atomics serialise)
__device__ __forceinline__ void sel_hist_add(unsigned* h, unsigned bin, bool on) {
    const unsigned long long live = __ballot(on);
    if (live == 0ull) return;
    const int leader = __ffsll((long long)live) - 1;
    const unsigned first = (unsigned)__shfl((int)bin, leader, 64);
    const unsigned long long same = __ballot(on && bin == first);
    if (!on) return;
    if (bin == first) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[first], (unsigned)__popcll(same));
    } else {
        atomicAdd(&h[bin], 1u);
    }
}

__device__ __forceinline__ bool sel_valid(long long t, int ignore, int C) { return t != (long long)ignore && t >= 0 && t < (long long)C; }

// PASS 0 / 1 / 2: digit = bits 31..21 / 20..10 / 9..0 of the elements whose higher bits equal the prefix found so far.
// head: elements before the first 16-byte boundary of true_prob (all of P when it is read by element).
template <int PASS>
__global__ __launch_bounds__(256) void ohem_select_hist_kernel(const float* __restrict__ tp, const long long* __restrict__ target, long long P,
                                                               long long head, int C, int ignore, unsigned long long k,
                                                               SelWs* __restrict__ ws) {
    __shared__ unsigned h[SEL_BINS];
    __shared__ unsigned long long sc[2][256];
    __shared__ unsigned long long out[2];
    __shared__ unsigned long long sh4[4];
    for (int i = threadIdx.x; i < SEL_BINS; i += 256) h[i] = 0u;
    unsigned prefix = 0;
    if (PASS > 0) {
        const unsigned long long prev_prefix = PASS == 1 ? 0ull : ws->state[0][0];
        const unsigned long long r = PASS == 1 ? k - 1ull : ws->state[0][1];
        unsigned bin;
        unsigned long long rem;
        sel_find_bin(ws->hist[PASS - 1], r, sc, out, bin, rem);
        prefix = ((unsigned)prev_prefix << 11) | bin;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ws->state[PASS - 1][0] = prefix;
            ws->state[PASS - 1][1] = rem;
        }
    }
    __syncthreads();
    constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    constexpr unsigned MASK = PASS == 2 ? 1023u : 2047u;
    constexpr int PSHIFT = PASS == 1 ? 21 : 10;          // the prefix is the pattern above this bit (PASS > 0)
    const long long tid = blockIdx.x * 256ll + threadIdx.x, nthr = gridDim.x * 256ll;
    const long long nvec = (P - head) >> 2, tail0 = head + (nvec << 2), nscalar = head + (P - tail0);
    unsigned long long nv = 0;
    const bool t16 = ((reinterpret_cast<uintptr_t>(target + head)) & 15) == 0;
    for (long long v = tid; v < nvec; v += nthr) {
        const long long i = head + (v << 2);
        const u32x4 b = ldg16(tp + i);
        if (PASS == 0) {
            long long t[4];
            if (t16) {
                const longlong2 a = *reinterpret_cast<const longlong2*>(target + i), c = *reinterpret_cast<const longlong2*>(target + i + 2);
                t[0] = a.x; t[1] = a.y; t[2] = c.x; t[3] = c.y;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = target[i + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) nv += sel_valid(t[j], ignore, C) ? 1ull : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool on = PASS == 0 || (b[j] >> PSHIFT) == prefix;
            sel_hist_add(h, (b[j] >> SHIFT) & MASK, on);
        }
    }
    for (long long s = tid; s < nscalar; s += nthr) {
        const long long i = s < head ? s : tail0 + (s - head);
        const unsigned b = __float_as_uint(tp[i]);
        if (PASS == 0) nv += sel_valid(target[i], ignore, C) ? 1ull : 0ull;
        const bool on = PASS == 0 || (b >> PSHIFT) == prefix;
        sel_hist_add(h, (b >> SHIFT) & MASK, on);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SEL_BINS; i += 256) {
        const unsigned c = h[i];
        if (c) atomicAdd(&ws->hist[PASS][i], (unsigned long long)c);
    }
    if (PASS == 0) {
        nv = sel_block_sum<unsigned long long>(nv, sh4);
        if (threadIdx.x == 0 && nv) atomicAdd(&ws->n_valid, nv);
    }
}

// SELECT: min_kept > 0.  head as above, for the common alignment of true_prob, nll and coef (P: by element).
template <bool SELECT>
__global__ __launch_bounds__(256) void ohem_select_emit_kernel(const float* __restrict__ tp, const float* __restrict__ nll,
                                                               const long long* __restrict__ target, long long P, long long head, int C,
                                                               int ignore, const float* __restrict__ class_weight, float thresh,
                                                               unsigned long long min_kept, float* __restrict__ coef,
                                                               float* __restrict__ result, SelWs* __restrict__ ws) {
    __shared__ unsigned long long sc[2][256];
    __shared__ unsigned long long out[2];
    __shared__ double shd[4];
    __shared__ long long shl[4];
    __shared__ float w[SEL_MAXC];
    if (threadIdx.x < SEL_MAXC) w[threadIdx.x] = (class_weight && (int)threadIdx.x < C) ? class_weight[threadIdx.x] : 1.f;
    float threshold = thresh;
    bool apply = false;
    if (SELECT) {
        unsigned bin;
        unsigned long long rem;
        sel_find_bin(ws->hist[2], ws->state[1][1], sc, out, bin, rem);
        const unsigned bits = ((unsigned)ws->state[1][0] << 10) | (bin & 1023u);
        const float kth = __uint_as_float(bits);
        threshold = (kth != kth) ? kth : (kth > thresh ? kth : thresh);          // torch.maximum: a NaN propagates
        const unsigned long long n_valid = ws->n_valid;
        apply = n_valid >= min_kept && n_valid > 0ull;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[2] = threshold;
        result[3] = apply ? 1.f : 0.f;
    }
    __syncthreads();                            // w
    const bool all = !SELECT || !apply;
    const long long tid = blockIdx.x * 256ll + threadIdx.x, nthr = gridDim.x * 256ll;
    const long long nvec = (P - head) >> 2, tail0 = head + (nvec << 2), nscalar = head + (P - tail0);
    double den = 0.0, num = 0.0;
    long long n_v = 0, n_k = 0;
    const bool t16 = ((reinterpret_cast<uintptr_t>(target + head)) & 15) == 0;
    for (long long v = tid; v < nvec; v += nthr) {
        const long long i = head + (v << 2);
        const f32x4 p = *reinterpret_cast<const f32x4*>(tp + i), l = *reinterpret_cast<const f32x4*>(nll + i);
        long long t[4];
        if (t16) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(target + i), c = *reinterpret_cast<const longlong2*>(target + i + 2);
            t[0] = a.x; t[1] = a.y; t[2] = c.x; t[3] = c.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = target[i + j];
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool valid = sel_valid(t[j], ignore, C);
            const bool kept = valid && (all || p[j] <= threshold);
            const float cf = kept ? w[valid ? (int)t[j] : 0] : 0.f;
            o[j] = cf;
            den += (double)cf;
            num += (double)cf * (double)l[j];
            n_v += valid ? 1 : 0;
            n_k += kept ? 1 : 0;
        }
        *reinterpret_cast<f32x4*>(coef + i) = o;
    }
    for (long long s = tid; s < nscalar; s += nthr) {
        const long long i = s < head ? s : tail0 + (s - head);
        const long long t = target[i];
        const bool valid = sel_valid(t, ignore, C);
        const bool kept = valid && (all || tp[i] <= threshold);
        const float cf = kept ? w[valid ? (int)t : 0] : 0.f;
        coef[i] = cf;
        den += (double)cf;
        num += (double)cf * (double)nll[i];
        n_v += valid ? 1 : 0;
        n_k += kept ? 1 : 0;
    }
    den = sel_block_sum<double>(den, shd);
    num = sel_block_sum<double>(num, shd);
    n_v = sel_block_sum<long long>(n_v, shl);
    n_k = sel_block_sum<long long>(n_k, shl);
    if (threadIdx.x == 0) {
        SelPartial q;
        q.den = den; q.num = num; q.valid = n_v; q.kept = n_k;
        ws->part[blockIdx.x] = q;
    }
}

__global__ __launch_bounds__(256) void ohem_select_final_kernel(const SelWs* __restrict__ ws, int blocks, float* __restrict__ result,
                                                                long long* __restrict__ counts) {
    __shared__ double shd[4];
    __shared__ long long shl[4];
    double den = 0.0, num = 0.0;
    long long n_v = 0, n_k = 0;
    for (int i = threadIdx.x; i < blocks; i += 256) {       // fixed order: the grid depends on P alone
        const SelPartial q = ws->part[i];
        den += q.den; num += q.num; n_v += q.valid; n_k += q.kept;
    }
    den = sel_block_sum<double>(den, shd);
    num = sel_block_sum<double>(num, shd);
    n_v = sel_block_sum<long long>(n_v, shl);
    n_k = sel_block_sum<long long>(n_k, shl);
    if (threadIdx.x == 0) {
        result[0] = (float)(num / den);                     // 0 / 0 = NaN: nothing kept
        result[1] = (float)den;
        counts[0] = n_v;
        counts[1] = n_k;
    }
}

// elements of `p` before its first 16-byte boundary
static inline long long sel_head(const void* p, long long P) {
    const long long h = (long long)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / 4);
    return h < P ? h : P;
}

}  // namespace fs

using namespace fs;

extern "C" long long fs_ohem_select_workspace_bytes(long long P) {
    if (P <= 0) return 0;
    return (long long)(sizeof(SelWs) - sizeof(SelPartial)) + (long long)sel_blocks(P) * (long long)sizeof(SelPartial);
}

extern "C" fs_status fs_ohem_select(void* stream, const float* true_prob, const float* nll, const long long* target, long long P, int C,
                                    int ignore, const float* class_weight, float thresh, long long min_kept, float* coef, float* result,
                                    long long* counts, void* workspace, long long workspace_bytes) {
    FS_REQUIRE(P > 0, FS_ERR_INVALID, "fs_ohem_select: P = %lld must be positive", P);
    FS_REQUIRE(C >= 1 && C <= SEL_MAXC, FS_ERR_INVALID, "fs_ohem_select: C = %d classes, 1..%d supported", C, SEL_MAXC);
    FS_REQUIRE(true_prob && nll && target && coef && result && counts, FS_ERR_INVALID, "fs_ohem_select: null argument");
    FS_REQUIRE(min_kept >= 0, FS_ERR_INVALID, "fs_ohem_select: min_kept = %lld is negative", min_kept);
    auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    FS_REQUIRE(!mis(true_prob, 4) && !mis(nll, 4) && !mis(coef, 4) && !mis(result, 4) && !mis(target, 8) && !mis(counts, 8) &&
                   !(class_weight && mis(class_weight, 4)),
               FS_ERR_INVALID, "fs_ohem_select: float vectors must be 4-byte aligned, target and counts 8-byte aligned");
    const long long need = fs_ohem_select_workspace_bytes(P);
    FS_REQUIRE(workspace && workspace_bytes >= need && !mis(workspace, 8), FS_ERR_INVALID,
               "fs_ohem_select: 8-byte aligned workspace of %lld bytes needed (fs_ohem_select_workspace_bytes), got %lld", need,
               workspace ? workspace_bytes : 0ll);
    hipStream_t st = (hipStream_t)stream;
    SelWs* ws = (SelWs*)workspace;
    const unsigned blocks = sel_blocks(P);
    const long long head_tp = sel_head(true_prob, P);
    // the emit pass moves three float vectors in step: 16-byte accesses only where they share their alignment
    const bool same = ((reinterpret_cast<uintptr_t>(true_prob) ^ reinterpret_cast<uintptr_t>(nll)) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(true_prob) ^ reinterpret_cast<uintptr_t>(coef)) & 15) == 0;
    const long long head_emit = same ? head_tp : P;
    // bytes by the kernels' own count: true_prob once per pass, target in pass 0 and in emit, nll and coef once
    if (min_kept > 0) {
        const unsigned long long k = (unsigned long long)(min_kept < P ? min_kept : P);
        FS_LAUNCH(ohem_select_clear_kernel, dim3(1), dim3(256), 0, st, ws);
        FS_NOTE_BYTES(P * 12.0);
        FS_LAUNCH((ohem_select_hist_kernel<0>), dim3(blocks), dim3(256), 0, st, true_prob, target, P, head_tp, C, ignore, k, ws);
        FS_NOTE_BYTES(P * 4.0);
        FS_LAUNCH((ohem_select_hist_kernel<1>), dim3(blocks), dim3(256), 0, st, true_prob, target, P, head_tp, C, ignore, k, ws);
        FS_NOTE_BYTES(P * 4.0);
        FS_LAUNCH((ohem_select_hist_kernel<2>), dim3(blocks), dim3(256), 0, st, true_prob, target, P, head_tp, C, ignore, k, ws);
        FS_NOTE_BYTES(P * 20.0);
        FS_LAUNCH((ohem_select_emit_kernel<true>), dim3(blocks), dim3(256), 0, st, true_prob, nll, target, P, head_emit, C, ignore,
                  class_weight, thresh, (unsigned long long)min_kept, coef, result, ws);
    } else {
        FS_NOTE_BYTES(P * 20.0);
        FS_LAUNCH((ohem_select_emit_kernel<false>), dim3(blocks), dim3(256), 0, st, true_prob, nll, target, P, head_emit, C, ignore,
                  class_weight, thresh, 0ull, coef, result, ws);
    }
    FS_LAUNCH(ohem_select_final_kernel, dim3(1), dim3(256), 0, st, (const SelWs*)ws, (int)blocks, result, counts);
    return check_launch("fs_ohem_select");
}
