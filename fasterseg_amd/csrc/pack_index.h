// Index arithmetic of the two filter-pack layouts, shared by the kernels that write them: fs_pack_weight (elementwise.hip),
// fs_pack_weight_frag (conv3x3_halo.hip) and the grouped fs_refresh_weights (refresh.hip).  One definition, so a pack written
// by any of them is the same bytes.
#pragma once
#include "common.h"

namespace fs {

// Implicit-GEMM pack out[co][r][s][ci]: element offset in the strided OIHW source (contiguous taps) of packed element `idx`.
__device__ __forceinline__ long long pack_src_offset(long long idx, long long o_stride, long long i_stride, int Cin, int R, int S) {
    long long t = idx;
    const int ci = divmod32(t, Cin);
    const int s = divmod32(t, S);
    const int r = divmod32(t, R);
    const int co = (int)t;
    return co * o_stride + ci * i_stride + r * S + s;
}

// Fragment-order pack out[n_tile][chunk][tap][kk][lane][VEC] (conv3x3_halo.hip, zoom_cell.hip) with
//   cout = n_tile*32 + (lane&31), cin = chunk*CK + kk*(CK/2) + (lane>>5)*VEC + e,   CK = 4 * VEC:
// source offset of packed element `idx`, or -1 outside the bank (the element is zero).
template <int VEC>
__device__ __forceinline__ long long pack_frag_src_offset(long long idx, long long o_stride, long long i_stride, int Cout, int Cin,
                                                          int nchunks) {
    constexpr int CK = 4 * VEC;
    long long t = idx;
    const int e = (int)(t % VEC); t /= VEC;
    const int lane = (int)(t % 64); t /= 64;
    const int kk = (int)(t % 2); t /= 2;
    const int tap = (int)(t % 9); t /= 9;
    const int chunk = (int)(t % nchunks);
    const int nt = (int)(t / nchunks);
    const int co = nt * 32 + (lane & 31);
    const int ci = chunk * CK + kk * (CK / 2) + (lane >> 5) * VEC + e;
    if (co < Cout && ci < Cin) return co * o_stride + ci * i_stride + tap;
    return -1;
}

// elements of a fragment-order bank: whole 128-channel block tiles x whole CK-channel chunks
__host__ __device__ inline long long pack_frag_elems(int Cout, int Cin, int vec) {
    const int ck = 4 * vec;
    const long long ntiles = ((Cout + 127) / 128) * 4, nchunks = (Cin + ck - 1) / ck;
    return ntiles * nchunks * 9 * 2 * 64 * vec;
}

}  // namespace fs
