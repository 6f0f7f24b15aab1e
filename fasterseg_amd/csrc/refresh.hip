// Reload of a built inference engine's weight-derived buffers: every filter pack, every folded BatchNorm scale / shift and the
// classifier bias rewritten in place by ONE table-driven launch (the shape of optim.hip's multi-tensor SGD).
//
// The engine (fasterseg_amd/engine.py) copies what it needs from the network once, at construction, and bakes the addresses into its
// launch records and its hipGraph.  The reference's drivers change the weights under a live evaluator: train/train.py:196-208 validates
// the model it is training after the first and every tenth epoch, search/train_search.py:141-183 after every epoch, and
// train/train.py:124-135 loads a trained teacher (weights0.pt) into a model that already exists.  Re-deriving a few MB of packs is a
// memory-bound gather; doing it as several hundred fs_pack_weight / torch launches would cost more in launches than in bytes.
//
// One block = one chunk of REFRESH_CHUNK destination elements of one entry; consecutive lanes write consecutive destination elements
// (coalesced 2- / 4-byte vector-memory stores), the sources are read through the index functions the stand-alone pack kernels use
// (pack_index.h), so the bytes are theirs.  No LDS, no atomics, nothing read back.
#include "common.h"
#include "pack_index.h"

namespace fs {

constexpr int REFRESH_CHUNK = 4096;       // destination elements per block

// destination elements of an entry (host: validated entries only)
__host__ __device__ inline long long refresh_elems(const fs_refresh_entry& e) {
    if (e.kind == FS_REFRESH_PACK) return (long long)e.Cout * e.R * e.S * e.Cin;
    if (e.kind == FS_REFRESH_PACK_FRAG) return pack_frag_elems(e.Cout, e.Cin, e.dtype == FS_F32 ? 4 : 8);      // elements per 16 bytes
    return e.Cout;
}

template <typename T>
__device__ __forceinline__ void refresh_pack(const fs_refresh_entry& e, long long begin, long long end) {
    T* const out = (T*)e.dst;
    for (long long idx = begin + threadIdx.x; idx < end; idx += 256)
        Elem<T>::store(out + idx, e.src[pack_src_offset(idx, e.o_stride, e.i_stride, e.Cin, e.R, e.S)]);
}

template <typename T>
__device__ __forceinline__ void refresh_pack_frag(const fs_refresh_entry& e, long long begin, long long end) {
    constexpr int VEC = Elem<T>::VEC;
    T* const out = (T*)e.dst;
    const int nchunks = (e.Cin + 4 * VEC - 1) / (4 * VEC);
    for (long long idx = begin + threadIdx.x; idx < end; idx += 256) {
        const long long src = pack_frag_src_offset<VEC>(idx, e.o_stride, e.i_stride, e.Cout, e.Cin, nchunks);
        const float v = src >= 0 ? e.src[src] : 0.f;
        Elem<T>::store(out + idx, v);
    }
}

__global__ __launch_bounds__(256) void refresh_weights_kernel(const fs_refresh_entry* __restrict__ entries, int n_entries,
                                                              const int* __restrict__ chunks) {
    const int t = chunks[2 * blockIdx.x];
    const int c = chunks[2 * blockIdx.x + 1];
    if (t < 0 || t >= n_entries || c < 0) return;
    const fs_refresh_entry e = entries[t];
    const long long total = refresh_elems(e);
    const long long begin = (long long)c * REFRESH_CHUNK;
    const long long end = begin + REFRESH_CHUNK < total ? begin + REFRESH_CHUNK : total;
    switch (e.kind) {
        case FS_REFRESH_PACK:
            if (e.dtype == FS_BF16) refresh_pack<bf16_t>(e, begin, end);
            else if (e.dtype == FS_F16) refresh_pack<f16_t>(e, begin, end);
            else refresh_pack<float>(e, begin, end);
            break;
        case FS_REFRESH_PACK_FRAG:
            if (e.dtype == FS_BF16) refresh_pack_frag<bf16_t>(e, begin, end);
            else if (e.dtype == FS_F16) refresh_pack_frag<f16_t>(e, begin, end);
            else refresh_pack_frag<float>(e, begin, end);
            break;
        case FS_REFRESH_FOLD: {
            float* const scale = (float*)e.dst;
            for (long long ch = begin + threadIdx.x; ch < end; ch += 256) {
                const float s = e.src[e.lo + ch] * rsqrtf(e.var[e.lo + ch] + e.eps);
                scale[ch] = s;
                e.shift[ch] = e.beta[e.lo + ch] - e.mean[e.lo + ch] * s;
            }
            break;
        }
        case FS_REFRESH_BIAS:
            for (long long ch = begin + threadIdx.x; ch < end; ch += 256) e.shift[ch] = e.src[ch];
            break;
        default:
            break;
    }
}

}  // namespace fs

using namespace fs;

extern "C" int fs_refresh_chunk_elems(void) { return REFRESH_CHUNK; }

static long long entry_chunks(const fs_refresh_entry* e, bool f16_too) {
    FS_REQUIRE(e, -1, "fs_refresh_entry_chunks: null entry");
    FS_REQUIRE(e->kind >= FS_REFRESH_PACK && e->kind <= FS_REFRESH_BIAS, -1, "fs_refresh_entry_chunks: unknown kind %d", e->kind);
    FS_REQUIRE(e->Cout >= 1, -1, "fs_refresh_entry_chunks: Cout %d < 1", e->Cout);
    FS_REQUIRE(e->src, -1, "fs_refresh_entry_chunks: null source");
    if (e->kind == FS_REFRESH_PACK || e->kind == FS_REFRESH_PACK_FRAG) {
        FS_REQUIRE(e->Cin >= 1, -1, "fs_refresh_entry_chunks: Cin %d < 1", e->Cin);
        FS_REQUIRE(f16_too ? dtype_ok(e->dtype) : dtype_train_ok(e->dtype), -1, "fs_refresh_entry_chunks: bad dtype %d", e->dtype);
        FS_REQUIRE(e->R >= 1 && e->S >= 1, -1, "fs_refresh_entry_chunks: bad taps %dx%d", e->R, e->S);
        FS_REQUIRE(e->kind != FS_REFRESH_PACK_FRAG || (e->R == 3 && e->S == 3), -1,
                   "fs_refresh_entry_chunks: the fragment pack is 3x3 only (got %dx%d)", e->R, e->S);
        FS_REQUIRE(e->o_stride >= 0 && e->i_stride >= 0, -1, "fs_refresh_entry_chunks: negative filter stride");
        FS_REQUIRE(e->dst, -1, "fs_refresh_entry_chunks: null destination");
    } else if (e->kind == FS_REFRESH_FOLD) {
        FS_REQUIRE(e->lo >= 0, -1, "fs_refresh_entry_chunks: negative channel offset %d", e->lo);
        FS_REQUIRE(e->beta && e->mean && e->var, -1, "fs_refresh_entry_chunks: null BatchNorm source");
        FS_REQUIRE(e->dst && e->shift, -1, "fs_refresh_entry_chunks: null destination");
    } else {
        FS_REQUIRE(e->shift, -1, "fs_refresh_entry_chunks: null destination");
    }
    return (refresh_elems(*e) + REFRESH_CHUNK - 1) / REFRESH_CHUNK;
}

// the validator of ABI 218: packs into fp32 / bf16, as its boundary contract says (any other code, FS_F16 included, is a bad dtype)
extern "C" long long fs_refresh_entry_chunks(const fs_refresh_entry* e) { return entry_chunks(e, false); }
// the same validator for an inference engine's table: packs into the three storage types
extern "C" long long fs_refresh_entry_chunks_infer(const fs_refresh_entry* e) { return entry_chunks(e, true); }

extern "C" fs_status fs_refresh_weights(void* stream, const fs_refresh_entry* entries, int n_entries, const int* chunks, int n_chunks) {
    FS_REQUIRE(entries && chunks, FS_ERR_INVALID, "fs_refresh_weights: null table");
    FS_REQUIRE(n_entries > 0 && n_chunks >= 0, FS_ERR_INVALID, "fs_refresh_weights: bad table size (%d entries, %d chunks)", n_entries,
               n_chunks);
    if (n_chunks == 0) return FS_OK;
    FS_LAUNCH(refresh_weights_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, entries, n_entries, chunks);
    return check_launch("fs_refresh_weights");
}
