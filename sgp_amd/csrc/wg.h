// Wave and workgroup primitives of the scalar (non-MFMA) kernels, and their host launch arithmetic.
// Every tree here has ONE fixed order, so a result does not change from run to run or with the launch.
//
// There are two fp64 sum trees and both stay, because every call site keeps the tree it was written with and so keeps
// the bits of its result: wg_reduce (a halving tree over T slots of LDS; scalers.hip, gwnet.hip's softmax) and
// wg_sum_waves (a shuffle-down tree per wave, then the waves in wave order; train.hip).  Making them one tree would
// change the last bit of one side's sums and is not attempted here.  The xor butterflies of spmm.hip, gated_gn.hip and
// gwnet.hip's layer norm leave the sum in EVERY lane; they are a different tool and live with their kernels.
#pragma once
#include "common.h"

namespace sgp {

// ---------------------------------------------------------------------------------------------------------- host
// workgroups for `items` at `per_block` each, between 1 and `cap`
inline unsigned grid_for(long long items, long long per_block, long long cap = 2048) {
    long long g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    return (unsigned)(g > cap ? cap : g);
}

// 0 <= v < n as ONE unsigned compare (n >= 0): the test in front of everything a device-side id indexes
__host__ __device__ __forceinline__ bool in_range(int v, long long n) { return (unsigned)v < (unsigned long long)n; }
__host__ __device__ __forceinline__ bool in_range(long long v, long long n) {
    return (unsigned long long)v < (unsigned long long)n;
}

// ---------------------------------------------------------------------------------------------------------- wave
// shuffle-down tree over the 64 lanes; lane 0 holds the sum
template <class V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// xor butterflies over the 64 lanes: EVERY lane holds the minimum / maximum
template <class V>
__device__ __forceinline__ V wave_min(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const V o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
template <class V>
__device__ __forceinline__ V wave_max(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const V o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

// the flag scan of one wave: the number of lanes below this one whose flag is set; total = all of them (every lane)
__device__ __forceinline__ int wave_rank(bool flag, int& total) {
    const unsigned long long m = __ballot(flag);
    total = __popcll(m);
    return __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// ---------------------------------------------------------------------------------------------------- reductions
// Halving tree over T slots of LDS that the caller has filled (slot = thread): fold(a, b) folds slot b into slot a,
// for as many quantities and element-wise operations (sum, min, max, or) as the caller keeps per slot.  Slot 0 holds
// the result, visible to every thread on return.
template <int T, class Fold>
__device__ __forceinline__ void wg_reduce(Fold fold) {
    __syncthreads();
    for (int w = T / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) fold((int)threadIdx.x, (int)threadIdx.x + w);
        __syncthreads();
    }
}

// one value per thread through wg_reduce, returned to every thread; `sh` [T] may be reused right after
template <int T, class V, class Op>
__device__ __forceinline__ V wg_reduce(V v, V* sh, Op op) {
    sh[threadIdx.x] = v;
    wg_reduce<T>([&](int a, int b) { sh[a] = op(sh[a], sh[b]); });
    const V r = sh[0];
    __syncthreads();
    return r;
}

// Sums of NV values per thread over the T / 64 waves of a workgroup: wave_sum, then the waves in wave order.  The
// result is valid in thread 0.  `lds` holds NV * T / 64 values and may come straight from an earlier sum.
template <int T, int NV, class V>
__device__ __forceinline__ void wg_sum_waves(V (&v)[NV], V* lds) {
    constexpr int W = T / 64;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) lds[k * W + wave] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            V s = lds[k * W];
#pragma unroll
            for (int w = 1; w < W; ++w) s += lds[k * W + w];
            v[k] = s;
        }
}

// ---------------------------------------------------------------------------------------------------------- scan
// Exclusive scan of NQ quantities over items 0 .. n by ONE workgroup of T threads.  Thread t owns the contiguous chunk
// [min(t per, n), min((t + 1) per, n)) with per = ceil(n / T): it adds its chunk up, a Hillis-Steele scan over the T
// chunk sums in LDS gives every chunk its start, and the thread walks its chunk again.  load(i, v) fills v[NQ] for
// item i (called in both walks; in the second one before store(i, .), so the scan may run in place); store(i, run)
// gets the sums of the items below i.  total[NQ] is returned to every thread.  `sums` is [NQ][T] of LDS.
template <int T, int NQ, class S, class Load, class Store>
__device__ __forceinline__ void wg_exclusive_scan(long long n, S (*sums)[T], Load load, Store store, S (&total)[NQ]) {
    const int t = threadIdx.x;
    const long long per = (n + T - 1) / T;
    const long long lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    S s[NQ], v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) s[q] = 0;
    for (long long i = lo; i < hi; ++i) {
        load(i, v);
#pragma unroll
        for (int q = 0; q < NQ; ++q) s[q] += v[q];
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) sums[q][t] = s[q];
    __syncthreads();
    for (int off = 1; off < T; off <<= 1) {
        S add[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) add[q] = t >= off ? sums[q][t - off] : (S)0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; ++q) sums[q][t] += add[q];
        __syncthreads();
    }
    S run[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) { run[q] = sums[q][t] - s[q]; total[q] = sums[q][T - 1]; }
    for (long long i = lo; i < hi; ++i) {
        load(i, v);
        store(i, run);
#pragma unroll
        for (int q = 0; q < NQ; ++q) run[q] += v[q];
    }
}

}  // namespace sgp
