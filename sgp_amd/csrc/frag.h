// The packed weight layout of every kernel that multiplies with v_mfma_f32_16x16x4_f32 and the weight as the A operand
// (rows = output features): the dense family (dense_tile.h), the recurrent window kernels (rnn_window.hip,
// rnn_impute.hip) and the GRIN stages (grin.hip).  This is the one place that describes and writes it.
//
// A matrix A[rows, cols] is cut into T = ceil(rows / 16) tiles of 16 rows and KB = ceil(cols / 16) k-blocks of 16
// columns and stored in FRAGMENT ORDER, zero outside the matrix:
//
//   packed[t][kb][l][s] = A[16 t + (l & 15)][16 kb + 4 (l >> 4) + s]      t < T, kb < KB, lane l < 64, s < 4
//
// frag_floats(rows, cols) = 256 T KB floats.  One coalesced 1 KB read per wave (16 bytes per lane) is the A operand of
// 4 consecutive MFMAs; their B operand is the lane's 16-byte piece, columns 16 kb + 4 (l >> 4) + 0 .. 3, of row
// (l & 15) of the other factor, so 16 rows of state or activations meet a tile of 16 output features with no shuffle,
// and lane (n = l & 15, q = l >> 4) ends up with features 16 t + 4 q + 0 .. 3 of row n.
// A is the source matrix itself (plain) or its transpose (the backward kernels' W^T); the source may have any row stride.
// The grouped first decoder layer (decoder.hip) is this map once per group.  The reservoir kernels' packs carry biases
// and bf16 pieces in other layouts and are not this one.
#pragma once
#include "common.h"
#include "device_math.h"

namespace sgp {

constexpr int kPad = 4;    // floats of padding per LDS row of the kernels that read B pieces from LDS (rows stay 16-byte aligned)

__host__ __device__ inline long long frag_floats(int rows, int cols) {
    return (long long)((rows + 15) / 16) * ((cols + 15) / 16) * 256;
}

// src: R x C with leading dimension ld;  A = src (T tiles along R, KB blocks along C) or, with trans, src^T (T along C, KB along R)
static __global__ void frag_pack(const float* __restrict__ src, long long ld, int R, int C, int T, int KB, int trans,
                                 float* __restrict__ out) {
    const long long total = (long long)T * KB * 256;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int s = (int)(i & 3), l = (int)((i >> 2) & 63);
        const long long tk = i >> 8;
        const int kb = (int)(tk % KB), t = (int)(tk / KB);
        const int a = 16 * t + (l & 15), k = 16 * kb + 4 * (l >> 4) + s;
        const int r = trans ? k : a, c = trans ? a : k;
        out[i] = (r < R && c < C) ? src[(long long)r * ld + c] : 0.f;
    }
}

// packs src [R, C] (or its transpose) at `out` and moves `out` past it: the parts of a packed buffer follow each other
static inline void frag_pack_to(float*& out, const float* src, long long ld, int R, int C, int trans, hipStream_t s) {
    const int T = ((trans ? C : R) + 15) / 16, KB = ((trans ? R : C) + 15) / 16;
    const long long blocks = (long long)T * KB;                       // 256 floats each
    hipLaunchKernelGGL(frag_pack, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, src, ld, R, C, T, KB, trans, out);
    out += blocks * 256;
}

// ---- device side: the products that read this layout -----------------------------------------------------------
__device__ __forceinline__ f32x4 mfma4(f32x4 w, f32x4 b, f32x4 acc) {
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], b[s], acc, 0, 0, 0);
    return acc;
}

// output tile jt of a packed matrix with KB k-blocks times the lane's LDS row piece `in` (= row + 4 q)
__device__ __forceinline__ f32x4 tile_prod(const float* wp, int jt, int KB, const float* in, f32x4 acc, int lane) {
    const float* w = wp + ((long long)jt * KB * 64 + lane) * 4;
    for (int kb = 0; kb < KB; ++kb) acc = mfma4(ld4(w + (long long)kb * 256), ld4(in + 16 * kb), acc);
    return acc;
}

// b[col .. col + 3], zero from n_out on: the start of a chain whose tile is ragged
__device__ __forceinline__ f32x4 bias4(const float* b, int col, int n_out) {
    f32x4 v;
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = col + s < n_out ? b[col + s] : 0.f;
    return v;
}

}  // namespace sgp
