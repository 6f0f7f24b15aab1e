// PNG IDAT streams on the device (gfx950): the deflate behind SegTester's and PseudoLabeler's single-channel files.
//
// A label map is the easiest input deflate ever sees: after PNG's Up filter it is almost all zeros.  The encoder therefore knows one
// kind of match, (length, distance 1) - a run of equal bytes - and the fixed Huffman code, and the format is fixed so that the bytes
// can be checked against a reference encoder (include/fasterseg_hip.h states it in full): rows are cut into bands, every band is one
// fixed-Huffman block closed by an empty stored block (pigz's way of joining independently compressed pieces), so a band starts and
// ends on a byte boundary and is the work of ONE workgroup.
//
// Launch 1, png_band_kernel, one workgroup of 1024 threads per band:
//   1. the band's filtered bytes (filter byte 2, then row - row above, mod 256) are staged in LDS: 16-byte global loads of the row and
//      of the row above (alignment 1: any base, any pitch), a SWAR byte subtraction, byte stores into LDS;
//   2. every thread owns a contiguous piece of the band.  Two 1024-entry scans give it what the rules need at each position, the start
//      of the run it is in (max-scan of the last run start of each piece) and the end of that run (min-scan, from the right, of the
//      first run start of each piece); with o = position - start and L = end - start the position alone decides what it emits;
//   3. the pieces are walked twice: once to count bits - an exclusive sum-scan of the counts is each piece's bit offset - and once to
//      emit.  A thread gathers its codes in a 64-bit register and ORs whole 32-bit words into the zeroed LDS bit buffer with LDS
//      atomics (only the first and the last word of a piece are shared with a neighbour);
//   4. the buffer goes to the band's slot of the workspace with 16-byte stores, beside the band's byte length and its Adler-32 partials
//      (byte sum, position-weighted sum, count; 64-bit integers: 16384^2 * 255 < 2^37).
// Launch 2, png_pack_kernel: a block sums the lengths of the bands before its first one, then copies its bands behind `78 01`; block
// 0 also combines the Adler partials (a band's weighted sum shifts by (bytes after it) x (its byte sum)) and appends the final block,
// the checksum and the total.  No global atomic, no float: every output byte is a pure function of the input.
//
// LDS cap.  A band holds at most FS_PNG_BAND_MAX_BYTES = 16384 filtered bytes: 16 KiB of them, a bit buffer of 9/8 of that (18448
// bytes) and 16 KiB of scan scratch are 50.0 KiB a workgroup.  Two such workgroups are a CU's 32 waves, so LDS (three would fit the
// 160 KiB) does not limit occupancy, and the static allocation stays under the 64 KiB a kernel may declare without opting in.  The
// default band of a 1024 x 2048 map (4 rows, 8196 bytes) uses half of the cap.
// Block size.  The kernel is bound by the latency of each thread's serial walk over its piece (LDS byte loads, one after the other),
// not by bytes: with one band per CU (256 bands on 256 CUs) 256 threads left every SIMD with ONE wave and 33-byte pieces, 47 us for a
// 1024 x 2048 map; 1024 threads - four waves per SIMD, 9-byte pieces, two more steps in each scan - take 23 us.
#include "common.h"

namespace fs {

namespace {

constexpr int PNG_THREADS = 1024;         // of a band's workgroup: 16 waves, so a piece is short (9 bytes of the default band)
constexpr int PACK_THREADS = 256;
constexpr int PNG_CAP = FS_PNG_BAND_MAX_BYTES;
constexpr unsigned int ADLER_MOD = 65521u;

__host__ __device__ constexpr long long band_bound(long long n) { return (3 + 9 * n + 7 + 3 + 7) / 8 + 4; }
__host__ __device__ constexpr long long round16(long long v) { return (v + 15) / 16 * 16; }
constexpr int PNG_BUF_BYTES = (int)round16(band_bound(PNG_CAP));

struct BandMeta {                       // workspace, one per band, ahead of the slots
    unsigned long long bytes;           // the band's compressed bytes, its closing stored block included
    unsigned long long sum;             // sum of its filtered bytes
    unsigned long long weighted;        // sum of (count - i) * byte i
    unsigned long long count;           // its filtered bytes
};

struct PngArgs {
    int rows, row_bytes, rows_per_band, n_bands;
    long long pitch;
    long long slot;                     // bytes between two bands' slots (a multiple of 16)
};

struct __attribute__((packed, aligned(1))) U128Any {
    u32x4 v;
};
__device__ __forceinline__ u32x4 ld16_any(const unsigned char* p) { return reinterpret_cast<const U128Any*>(p)->v; }

// four bytes a - b mod 256 each: the low seven bits with the borrow kept inside the byte, then the top bits
__device__ __forceinline__ unsigned int sub_bytes(unsigned int a, unsigned int b) {
    return ((a | 0x80808080u) - (b & 0x7f7f7f7fu)) ^ ((a ^ ~b) & 0x80808080u);
}

// ---- the fixed Huffman code (RFC 1951 3.2.6), packed as the bit stream wants it: Huffman codes MSB first, extra bits LSB first --------
struct Code {
    unsigned int bits;
    int n;
};
__device__ __forceinline__ Code huff(unsigned int code, int n) { return Code{__brev(code) >> (32 - n), n}; }
__device__ __forceinline__ Code literal_code(unsigned int v) { return v < 144u ? huff(0x30u + v, 8) : huff(0x190u + v - 144u, 9); }
// a match of `len` in 3..258 at distance 1: the length symbol, its extra bits, the 5-bit distance code 0
__device__ __forceinline__ Code match_code(int len) {
    int k, e = 0;
    unsigned int extra = 0;
    const int m = len - 3;
    if (len == 258) k = 28;
    else if (m < 8) k = m;
    else {
        e = 29 - __clz(m);                               // floor(log2 m) - 2: 1..5 extra bits
        k = 4 * e + (m >> e);                            // four symbols per count of extra bits, from symbol 265 (m = 8, e = 1) on
        extra = (unsigned int)m & ((1u << e) - 1u);
    }
    const int sym = 257 + k;
    Code c = sym < 280 ? huff((unsigned int)(sym - 256), 7) : huff(0xC0u + (unsigned int)(sym - 280), 8);
    c.bits |= extra << c.n;
    c.n += e + 5;
    return c;
}

// ---- scans over the workgroup's PNG_THREADS entries, in LDS -------------------------------------------------------------------------------------------------------------
// inclusive scan over the entries in index order `i` (a thread passes threadIdx.x, or PNG_THREADS - 1 - threadIdx.x to scan from the right)
template <typename T, typename Op> __device__ __forceinline__ T block_scan(T v, T* s, int i, Op op) {
    s[i] = v;
    __syncthreads();
    for (int off = 1; off < PNG_THREADS; off <<= 1) {
        T o = v;
        const bool on = i >= off;
        if (on) o = s[i - off];
        __syncthreads();
        if (on) {
            v = op(o, v);
            s[i] = v;
        }
        __syncthreads();
    }
    return v;
}
// the entry before `i` of a finished scan, `first` for entry 0
template <typename T> __device__ __forceinline__ T scan_before(const T* s, int i, T first) { return i > 0 ? s[i - 1] : first; }

__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* s) {
    const int t = threadIdx.x;
    __syncthreads();                                     // s may still be read from an earlier use
    s[t] = v;
    __syncthreads();
    for (int off = (int)blockDim.x / 2; off > 0; off >>= 1) {
        if (t < off) s[t] += s[t + off];
        __syncthreads();
    }
    return s[0];
}

// The piece [c0, c1) of a band of n filtered bytes f.  start_in: the start of the run that reaches into the piece from the left;
// end_out: the first run start at or behind c1 (n: none).  Returns the bits of the piece's codes; with EMIT they are also ORed into buf
// from bit `at` on (acc / acc_n: what the caller has already placed below `at` in the word `at` lies in - the block header of piece 0).
template <bool EMIT>
__device__ __forceinline__ unsigned int walk(const unsigned char* f, int c0, int c1, int start_in, int end_out, unsigned int* buf,
                                             unsigned int at, unsigned long long acc) {
    unsigned int total = 0;
    unsigned int word = at >> 5;
    int acc_n = (int)(at & 31u);
    int s = start_in;
    int p = c0;
    while (p < c1) {
        const unsigned int v = f[p];
        if (p == 0 || f[p - 1] != v) s = p;
        int e = p + 1;
        while (e < c1 && f[e] == v) ++e;
        const int stop = e;                              // the part of the run inside the piece ends here
        if (e == c1) e = end_out;
        const int rest = e - s - 1;                      // L - 1: what follows the run's literal
        const int full = rest / 258, r = rest - full * 258;
        for (int q = p; q < stop; ++q) {
            const int o = q - s;
            Code c{0u, 0};
            if (o == 0) {
                c = literal_code(v);
            } else {
                const int k = (o - 1) / 258, at_k = (o - 1) - k * 258;
                if (k < full) {
                    if (at_k == 0) c = match_code(258);
                } else if (r >= 3) {
                    if (at_k == 0) c = match_code(r);
                } else {
                    c = literal_code(v);
                }
            }
            total += (unsigned int)c.n;
            if (EMIT && c.n) {
                acc |= (unsigned long long)c.bits << acc_n;
                acc_n += c.n;                            // < 32 + 18
                if (acc_n >= 32) {
                    atomicOr(&buf[word], (unsigned int)acc);
                    acc >>= 32;
                    acc_n -= 32;
                    ++word;
                }
            }
        }
        p = stop;
    }
    if (EMIT && acc != 0) atomicOr(&buf[word], (unsigned int)acc);
    return total;
}

}  // namespace

__global__ __launch_bounds__(PNG_THREADS) void png_band_kernel(PngArgs a, const unsigned char* __restrict__ src, BandMeta* __restrict__ meta,
                                                               unsigned char* __restrict__ slots) {
    __shared__ __attribute__((aligned(16))) unsigned char s_f[PNG_CAP];
    __shared__ __attribute__((aligned(16))) unsigned int s_buf[PNG_BUF_BYTES / 4];
    __shared__ int s_a[PNG_THREADS];
    __shared__ int s_b[PNG_THREADS];
    __shared__ unsigned long long s_w[PNG_THREADS];
    const int t = threadIdx.x;
    const int band = blockIdx.x;
    const int y0 = band * a.rows_per_band;
    const int rows = a.rows - y0 < a.rows_per_band ? a.rows - y0 : a.rows_per_band;
    const int stride = a.row_bytes + 1;
    const int n = rows * stride;                          // <= PNG_CAP (checked by the host)
    const int buf_words = (int)(round16(band_bound(n)) / 4);
    for (int i = t; i < buf_words; i += PNG_THREADS) s_buf[i] = 0u;

    // 1. the filtered band
    const int chunks = (a.row_bytes + 15) / 16;
    for (int item = t; item < rows * chunks; item += PNG_THREADS) {
        const int r = item / chunks, c = item - r * chunks;
        const int x0 = 16 * c;
        const int nb = a.row_bytes - x0 < 16 ? a.row_bytes - x0 : 16;
        const int y = y0 + r;
        const unsigned char* cur = src + (long long)y * a.pitch + x0;
        const unsigned char* up = cur - a.pitch;          // read only when y > 0
        unsigned char* dst = s_f + r * stride + 1 + x0;
        if (c == 0) dst[-1] = 2;
        if (nb == 16) {
            const u32x4 v = ld16_any(cur);
            u32x4 u = {0u, 0u, 0u, 0u};
            if (y > 0) u = ld16_any(up);
#pragma unroll
            for (int wd = 0; wd < 4; ++wd) {
                const unsigned int d = sub_bytes(v[wd], u[wd]);
#pragma unroll
                for (int b = 0; b < 4; ++b) dst[4 * wd + b] = (unsigned char)(d >> (8 * b));
            }
        } else {
            for (int i = 0; i < nb; ++i) dst[i] = (unsigned char)(cur[i] - (y > 0 ? up[i] : 0));
        }
    }
    __syncthreads();

    // 2. every thread's piece, the run that reaches into it and the run start behind it
    const int per = (n + PNG_THREADS - 1) / PNG_THREADS;
    const int c0 = t * per < n ? t * per : n;
    const int c1 = c0 + per < n ? c0 + per : n;
    int last = -1, first = n;
    unsigned long long sum = 0, weighted = 0;             // Adler partials of the piece: weighted = sum of (c1 - i) * f[i]
    for (int i = c0; i < c1; ++i) {
        const unsigned int v = s_f[i];
        if (i == 0 || s_f[i - 1] != v) {
            last = i;
            if (first == n) first = i;
        }
        sum += v;
        weighted += (unsigned long long)(c1 - i) * v;
    }
    block_scan(last, s_a, t, [](int l, int r) { return l > r ? l : r; });
    block_scan(first, s_b, PNG_THREADS - 1 - t, [](int l, int r) { return l < r ? l : r; });
    const int start_in = scan_before(s_a, t, 0);
    const int end_out = scan_before(s_b, PNG_THREADS - 1 - t, n);

    // 3. count, scan, emit.  Bits 0..2 are the block header: BFINAL = 0, BTYPE = 01 (LSB first: the value 2)
    const unsigned int mine = walk<false>(s_f, c0, c1, start_in, end_out, nullptr, 0u, 0ull);
    __syncthreads();                                      // s_a is read above and written below
    unsigned int* s_bits = reinterpret_cast<unsigned int*>(s_a);
    const unsigned int upto = block_scan(mine, s_bits, t, [](unsigned int l, unsigned int r) { return l + r; });
    const unsigned int code_bits = s_bits[PNG_THREADS - 1];
    walk<true>(s_f, c0, c1, start_in, end_out, s_buf, 3u + upto - mine, t == 0 ? 2ull : 0ull);
    // end of block (symbol 256: seven zero bits), the empty stored block (three zero bits, pad to the byte, 00 00 FF FF)
    const unsigned int bytes = (3u + code_bits + 7u + 3u + 7u) / 8u + 4u;
    __syncthreads();
    if (t == 0) {
        unsigned char* b = reinterpret_cast<unsigned char*>(s_buf);
        b[bytes - 2] = 0xFF;
        b[bytes - 1] = 0xFF;
    }
    const unsigned long long band_sum = block_sum(sum, s_w);
    const unsigned long long band_weighted = block_sum(weighted + (unsigned long long)(n - c1) * sum, s_w);   // (also orders b[] above)

    // 4. out: the slot and the band's record
    unsigned char* slot = slots + (long long)band * a.slot;
    for (int i = t; i < (int)((bytes + 15u) / 16u); i += PNG_THREADS) stg16(slot + 16 * i, *reinterpret_cast<const u32x4*>(&s_buf[4 * i]));
    if (t == 0) {
        BandMeta m;
        m.bytes = bytes;
        m.sum = band_sum;
        m.weighted = band_weighted;
        m.count = (unsigned long long)n;
        meta[band] = m;
    }
}

__global__ __launch_bounds__(PACK_THREADS) void png_pack_kernel(PngArgs a, const BandMeta* __restrict__ meta, const unsigned char* __restrict__ slots,
                                                               unsigned char* __restrict__ out, long long* __restrict__ out_bytes) {
    __shared__ unsigned long long s_w[PACK_THREADS];
    const int t = threadIdx.x;
    const int per = (a.n_bands + (int)gridDim.x - 1) / (int)gridDim.x;
    const int b0 = (int)blockIdx.x * per < a.n_bands ? (int)blockIdx.x * per : a.n_bands;
    const int b1 = b0 + per < a.n_bands ? b0 + per : a.n_bands;
    unsigned long long before = 0;
    for (int i = t; i < b0; i += PACK_THREADS) before += meta[i].bytes;
    unsigned long long off = 2ull + block_sum(before, s_w);
    for (int b = b0; b < b1; ++b) {
        const unsigned int bytes = (unsigned int)meta[b].bytes;
        const unsigned char* s = slots + (long long)b * a.slot;
        unsigned char* d = out + off;
        // bytes up to the first 16-byte boundary of the destination, then aligned 16-byte stores of unaligned loads, then the tail
        unsigned int head = (unsigned int)((16u - (unsigned int)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);
        if (head > bytes) head = bytes;
        const unsigned int vecs = (bytes - head) / 16u;
        const unsigned int tail = head + 16u * vecs;
        for (unsigned int i = t; i < head; i += PACK_THREADS) d[i] = s[i];
        for (unsigned int i = t; i < vecs; i += PACK_THREADS) stg16(d + head + 16u * i, ld16_any(s + head + 16u * i));
        for (unsigned int i = tail + t; i < bytes; i += PACK_THREADS) d[i] = s[i];
        off += bytes;
    }
    if (blockIdx.x != 0) return;
    // block 0: the stream's head, and behind the last band the final block and the Adler-32 of all filtered bytes
    const unsigned long long N = (unsigned long long)a.rows * (unsigned long long)(a.row_bytes + 1);
    const unsigned long long full = (unsigned long long)a.rows_per_band * (unsigned long long)(a.row_bytes + 1);
    unsigned long long len = 0, sa = 0, sb = 0;
    for (int i = t; i < a.n_bands; i += PACK_THREADS) {
        const BandMeta m = meta[i];
        const unsigned long long after = N - (full * (unsigned long long)i + m.count);
        len += m.bytes;
        sa += m.sum % ADLER_MOD;
        sb += (m.weighted % ADLER_MOD + (after % ADLER_MOD) * (m.sum % ADLER_MOD)) % ADLER_MOD;
    }
    len = block_sum(len, s_w);
    sa = block_sum(sa, s_w);
    sb = block_sum(sb, s_w);
    if (t == 0) {
        const unsigned int A = (unsigned int)((1ull + sa) % ADLER_MOD);
        const unsigned int B = (unsigned int)((N + sb) % ADLER_MOD);
        out[0] = 0x78;
        out[1] = 0x01;
        unsigned char* e = out + 2ull + len;
        e[0] = 0x01; e[1] = 0x00; e[2] = 0x00; e[3] = 0xFF; e[4] = 0xFF;
        e[5] = (unsigned char)(B >> 8); e[6] = (unsigned char)B; e[7] = (unsigned char)(A >> 8); e[8] = (unsigned char)A;
        *out_bytes = (long long)(2ull + len + 9ull);
    }
}

namespace {

// bands and bytes of a geometry; false: not a geometry
bool png_geometry(int rows, int row_bytes, int rows_per_band, long long* n_bands, long long* bound, long long* slot) {
    if (rows < 0 || row_bytes <= 0 || rows_per_band <= 0) return false;
    const long long stride = (long long)row_bytes + 1;
    const long long nb = ((long long)rows + rows_per_band - 1) / rows_per_band;
    long long total = 2 + 5 + 4;
    if (nb > 0) {
        const long long last_rows = (long long)rows - (nb - 1) * rows_per_band;
        total += (nb - 1) * band_bound((long long)rows_per_band * stride) + band_bound(last_rows * stride);
    }
    *n_bands = nb;
    *bound = total;
    *slot = round16(band_bound((long long)(rows < rows_per_band ? rows : rows_per_band) * stride));
    return true;
}

}  // namespace

}  // namespace fs

using namespace fs;

extern "C" size_t fs_png_deflate_bound(int rows, int row_bytes, int rows_per_band) {
    long long nb, bound, slot;
    return png_geometry(rows, row_bytes, rows_per_band, &nb, &bound, &slot) ? (size_t)bound : 0;
}

extern "C" size_t fs_png_deflate_workspace_bytes(int rows, int row_bytes, int rows_per_band) {
    long long nb, bound, slot;
    if (!png_geometry(rows, row_bytes, rows_per_band, &nb, &bound, &slot)) return 0;
    return (size_t)(nb * ((long long)sizeof(BandMeta) + slot));
}

extern "C" fs_status fs_png_deflate(void* stream, const unsigned char* src, int rows, int row_bytes, long long pitch, int rows_per_band,
                                    unsigned char* out, size_t out_capacity, long long* out_bytes, void* workspace, size_t ws_bytes) {
    long long nb, bound, slot;
    FS_REQUIRE(png_geometry(rows, row_bytes, rows_per_band, &nb, &bound, &slot), FS_ERR_INVALID,
               "fs_png_deflate: bad dimension: rows %d, row_bytes %d, rows_per_band %d", rows, row_bytes, rows_per_band);
    if (rows == 0) return FS_OK;
    FS_REQUIRE(pitch >= row_bytes, FS_ERR_INVALID, "fs_png_deflate: pitch %lld below the %d bytes of a row", pitch, row_bytes);
    const long long band_bytes = (long long)(rows < rows_per_band ? rows : rows_per_band) * ((long long)row_bytes + 1);
    FS_REQUIRE(band_bytes <= PNG_CAP, FS_ERR_UNSUPPORTED, "fs_png_deflate: a band of %lld filtered bytes is above the LDS cap of %d", band_bytes,
               PNG_CAP);
    const long long ws_need = nb * ((long long)sizeof(BandMeta) + slot);
    FS_REQUIRE((long long)rows * ((long long)row_bytes + 1) < (1LL << 31) && bound < (1LL << 31) && ws_need < (1LL << 31), FS_ERR_UNSUPPORTED,
               "fs_png_deflate: %d rows of %d bytes reach 2^31 bytes of filtered input, stream or workspace", rows, row_bytes);
    FS_REQUIRE(src && out && out_bytes && workspace, FS_ERR_INVALID, "fs_png_deflate: null src, out, out_bytes or workspace");
    FS_REQUIRE((reinterpret_cast<uintptr_t>(out_bytes) & 7) == 0 && aligned16(workspace), FS_ERR_INVALID,
               "fs_png_deflate: misaligned out_bytes (8 bytes) or workspace (16 bytes)");
    FS_REQUIRE(out_capacity >= (size_t)bound, FS_ERR_INVALID, "fs_png_deflate: out_capacity %zu below the bound of %lld bytes", out_capacity, bound);
    FS_REQUIRE(ws_bytes >= (size_t)ws_need, FS_ERR_INVALID, "fs_png_deflate: ws_bytes %zu below the %lld bytes of the workspace", ws_bytes, ws_need);
    PngArgs a;
    a.rows = rows; a.row_bytes = row_bytes; a.rows_per_band = rows_per_band; a.n_bands = (int)nb;
    a.pitch = pitch;
    a.slot = slot;
    BandMeta* meta = static_cast<BandMeta*>(workspace);
    unsigned char* slots = static_cast<unsigned char*>(workspace) + nb * (long long)sizeof(BandMeta);
    FS_NOTE_BYTES(2.0 * rows * (double)row_bytes + (double)bound);          // the map and its row above in, the band slots out
    FS_LAUNCH(png_band_kernel, dim3((unsigned)nb), dim3(PNG_THREADS), 0, (hipStream_t)stream, a, src, meta, slots);
    FS_NOTE_BYTES(2.0 * (double)bound);
    FS_LAUNCH(png_pack_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(PACK_THREADS), 0, (hipStream_t)stream, a,
              static_cast<const BandMeta*>(meta), static_cast<const unsigned char*>(slots), out, out_bytes);
    return check_launch("fs_png_deflate");
}
