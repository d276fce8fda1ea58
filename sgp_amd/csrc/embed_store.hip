// The 16-bit embedding store: fp32 -> bf16 / fp16 packing of the encoder's product after the hops have
// written their fp32 slots, and the row gather that widens a 16-bit embedding back to fp32 for the samplers
// (lib/datasets/iid_dataset.py:57-99 on a store of half the bytes).  The pack is HBM-bound (0.71 of the roofline on a
// 2.6 GB chunk); a 4096-row gather is bound by its launch and its index -> row loads, not by its bytes.
#include "wg.h"

using sgp::f32x4;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Round-to-nearest-even in integer arithmetic, bit-equal to torch's CPU cast: the half-way bias 0x7FFF plus the kept
// mantissa's last bit carries into the exponent where it must (up to infinity from the largest finite values);
// +-inf have a zero low half and pass through; every NaN becomes the quiet NaN 0x7FC0.
__device__ __forceinline__ unsigned to_bf16(float x) {
    const unsigned u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// The hardware convert (v_cvt_f16_f32) under the default round mode: nearest-even, fp16 subnormals kept, overflow to
// infinity, NaN stays NaN.  (NOT the packed convert v_cvt_pkrtz_f16_f32, which rounds toward zero.)
__device__ __forceinline__ unsigned to_f16(float x) {
    const _Float16 h = (_Float16)x;
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

template <int FMT>
__device__ __forceinline__ unsigned narrow(float x, int& overflow) {
    if constexpr (FMT == SGP_STORE_BF16) {
        return to_bf16(x);
    } else {
        const unsigned h = to_f16(x);
        // a finite fp32 value that became +-inf
        overflow += ((h & 0x7FFFu) == 0x7C00u && (__float_as_uint(x) & 0x7FFFFFFFu) < 0x7F800000u) ? 1 : 0;
        return h;
    }
}

// Widening is exact in both formats: bf16 is the upper half of the fp32 pattern, every fp16 value (subnormals
// included) is an fp32 value.
template <int FMT>
__device__ __forceinline__ float widen(unsigned h) {
    if constexpr (FMT == SGP_STORE_BF16) return __uint_as_float(h << 16);
    else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

// item i of `total` = (row, piece of the row); 32-bit division where the count allows it
__device__ __forceinline__ void split_index(long long i, long long total, int per_row, long long& r, int& c) {
    if (total <= 0x7FFFFFFFll) {
        const unsigned q = (unsigned)i / (unsigned)per_row;
        r = q;
        c = (int)((unsigned)i - q * (unsigned)per_row);
    } else {
        r = i / per_row;
        c = (int)(i - r * per_row);
    }
}

// Y[b, r, :] = narrow(X[b, r, :]).  V = 8: a thread takes 8 consecutive features with two 16-byte loads and one
// 16-byte store; V = 1: any feat, stride and element alignment.  COUNT (fp16): the finite values that became infinite
// are summed over the workgroup and added to *overflow with one atomic (none when the sum is zero).
template <int FMT, int V, bool COUNT>
__global__ __launch_bounds__(256) void pack_rows_kernel(
        const float* __restrict__ X, long long xrs, long long xbs,
        unsigned short* __restrict__ Y, long long yrs, long long ybs,
        int n_rows, int feat, unsigned long long* overflow) {
    const int b = blockIdx.y;
    const int per_row = (feat + V - 1) / V;
    const long long total = (long long)n_rows * per_row;
    const float* xb = X + (long long)b * xbs;
    unsigned short* yb = Y + (long long)b * ybs;
    int lost = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long r; int c;
        split_index(i, total, per_row, r, c);
        const float* xp = xb + r * xrs + (long long)c * V;
        unsigned short* yp = yb + r * yrs + (long long)c * V;
        if constexpr (V == 8) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(xp);
            const f32x4 d = *reinterpret_cast<const f32x4*>(xp + 4);
            u32x4 o;
            o.x = narrow<FMT>(a.x, lost) | (narrow<FMT>(a.y, lost) << 16);
            o.y = narrow<FMT>(a.z, lost) | (narrow<FMT>(a.w, lost) << 16);
            o.z = narrow<FMT>(d.x, lost) | (narrow<FMT>(d.y, lost) << 16);
            o.w = narrow<FMT>(d.z, lost) | (narrow<FMT>(d.w, lost) << 16);
            *reinterpret_cast<u32x4*>(yp) = o;
        } else {
            yp[0] = (unsigned short)narrow<FMT>(xp[0], lost);
        }
    }
    if constexpr (COUNT) {
        __shared__ int part[4];
        int v[1] = {lost};
        sgp::wg_sum_waves<256, 1>(v, part);
        if (threadIdx.x == 0 && v[0] > 0) atomicAdd(overflow, (unsigned long long)v[0]);
    }
}

// out[b, k, :] = widen(X[step ? step[k] : b, node[k], :])
template <int FMT, int V>
__global__ __launch_bounds__(256) void gather_rows_16_kernel(
        const unsigned short* __restrict__ X, long long xrs, long long xbs,
        const int* __restrict__ step, const int* __restrict__ node, int n_index,
        float* __restrict__ out, long long ors, long long obs, int feat) {
    const int b = blockIdx.y;
    const int per_row = (feat + V - 1) / V;
    const long long total = (long long)n_index * per_row;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        long long k; int c;
        split_index(i, total, per_row, k, c);
        const int sb = step ? step[k] : b;
        const unsigned short* xp = X + (long long)sb * xbs + (long long)node[k] * xrs + (long long)c * V;
        float* op = out + (long long)b * obs + k * ors + (long long)c * V;
        if constexpr (V == 8) {
            const u32x4 h = *reinterpret_cast<const u32x4*>(xp);
            f32x4 a, d;
            a.x = widen<FMT>(h.x & 0xFFFFu); a.y = widen<FMT>(h.x >> 16);
            a.z = widen<FMT>(h.y & 0xFFFFu); a.w = widen<FMT>(h.y >> 16);
            d.x = widen<FMT>(h.z & 0xFFFFu); d.y = widen<FMT>(h.z >> 16);
            d.z = widen<FMT>(h.w & 0xFFFFu); d.w = widen<FMT>(h.w >> 16);
            *reinterpret_cast<f32x4*>(op) = a;
            *reinterpret_cast<f32x4*>(op + 4) = d;
        } else {
            op[0] = widen<FMT>(xp[0]);
        }
    }
}

// the 8-element path: whole 16-byte pieces on both sides (8 fp32 = 32 bytes, 8 halves = 16 bytes)
inline bool vec8_ok(const void* p, long long s0, long long s1, int feat) {
    return feat % 8 == 0 && s0 % 8 == 0 && s1 % 8 == 0 && sgp::aligned16(p);
}

template <int FMT>
void launch_pack(bool vec, bool count, dim3 grid, hipStream_t s, const float* X, long long xrs, long long xbs,
                 unsigned short* Y, long long yrs, long long ybs, int n_rows, int feat, unsigned long long* overflow) {
    if constexpr (FMT == SGP_STORE_F16) {                    // (only float16 has counting kernels)
        if (count) {
            if (vec)
                hipLaunchKernelGGL((pack_rows_kernel<FMT, 8, true>), grid, dim3(256), 0, s, X, xrs, xbs, Y, yrs, ybs, n_rows, feat, overflow);
            else
                hipLaunchKernelGGL((pack_rows_kernel<FMT, 1, true>), grid, dim3(256), 0, s, X, xrs, xbs, Y, yrs, ybs, n_rows, feat, overflow);
            return;
        }
    }
    if (vec)
        hipLaunchKernelGGL((pack_rows_kernel<FMT, 8, false>), grid, dim3(256), 0, s, X, xrs, xbs, Y, yrs, ybs, n_rows, feat, overflow);
    else
        hipLaunchKernelGGL((pack_rows_kernel<FMT, 1, false>), grid, dim3(256), 0, s, X, xrs, xbs, Y, yrs, ybs, n_rows, feat, overflow);
}

template <int FMT>
void launch_gather(bool vec, dim3 grid, hipStream_t s, const unsigned short* X, long long xrs, long long xbs,
                   const int* step, const int* node, int n_index, float* out, long long ors, long long obs, int feat) {
    if (vec)
        hipLaunchKernelGGL((gather_rows_16_kernel<FMT, 8>), grid, dim3(256), 0, s, X, xrs, xbs, step, node, n_index, out, ors, obs, feat);
    else
        hipLaunchKernelGGL((gather_rows_16_kernel<FMT, 1>), grid, dim3(256), 0, s, X, xrs, xbs, step, node, n_index, out, ors, obs, feat);
}

}  // namespace

extern "C" {

int sgp_pack_rows_16(const float* X, int64_t xrs, int64_t xbs, int32_t batch, int32_t n_rows, int32_t feat,
                     int32_t fmt, void* Y, int64_t yrs, int64_t ybs, int64_t* overflow_count, sgp_stream_t stream) {
    SGP_REQUIRE(fmt == SGP_STORE_BF16 || fmt == SGP_STORE_F16, "sgp_pack_rows_16: fmt must be SGP_STORE_BF16 or SGP_STORE_F16");
    SGP_REQUIRE(n_rows >= 0 && batch >= 0 && feat >= 0 && batch <= 65535, "sgp_pack_rows_16: bad size");
    if (!n_rows || !batch || !feat) return 0;
    SGP_REQUIRE(X && Y, "sgp_pack_rows_16: null pointer");
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(X) & 3u) == 0 && (reinterpret_cast<uintptr_t>(Y) & 1u) == 0,
                "sgp_pack_rows_16: X must be 4-byte and Y 2-byte aligned");
    SGP_REQUIRE(!overflow_count || (reinterpret_cast<uintptr_t>(overflow_count) & 7u) == 0,
                "sgp_pack_rows_16: overflow_count must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec8_ok(X, xrs, xbs, feat) && vec8_ok(Y, yrs, ybs, feat);
    const bool count = overflow_count != nullptr && fmt == SGP_STORE_F16;
    // four items per thread where there is that much: fewer workgroups, hence fewer counter atomics
    const dim3 grid(sgp::grid_for((long long)n_rows * (vec ? feat / 8 : feat), 1024, 4096), batch);
    unsigned short* y = static_cast<unsigned short*>(Y);
    unsigned long long* oc = reinterpret_cast<unsigned long long*>(overflow_count);
    if (fmt == SGP_STORE_BF16) launch_pack<SGP_STORE_BF16>(vec, false, grid, s, X, xrs, xbs, y, yrs, ybs, n_rows, feat, oc);
    else launch_pack<SGP_STORE_F16>(vec, count, grid, s, X, xrs, xbs, y, yrs, ybs, n_rows, feat, oc);
    return sgp::check_launch("pack_rows_16");
}

int sgp_gather_rows_16(const void* X, int64_t xrs, int64_t xbs, const int32_t* step, const int32_t* node,
                       int32_t n_index, int32_t fmt, float* out, int64_t ors, int64_t obs,
                       int32_t batch, int32_t feat, sgp_stream_t stream) {
    SGP_REQUIRE(fmt == SGP_STORE_BF16 || fmt == SGP_STORE_F16, "sgp_gather_rows_16: fmt must be SGP_STORE_BF16 or SGP_STORE_F16");
    SGP_REQUIRE(n_index >= 0 && batch >= 0 && feat >= 0 && batch <= 65535, "sgp_gather_rows_16: bad size");
    if (step) batch = 1;
    if (!n_index || !batch || !feat) return 0;          // (an empty index tensor has no address)
    SGP_REQUIRE(X && node && out, "sgp_gather_rows_16: null pointer");
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(X) & 1u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
                "sgp_gather_rows_16: X must be 2-byte and out 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec8_ok(X, xrs, xbs, feat) && vec8_ok(out, ors, obs, feat);
    const dim3 grid(sgp::grid_for((long long)n_index * (vec ? feat / 8 : feat), 256, 4096), batch);
    const unsigned short* x = static_cast<const unsigned short*>(X);
    if (fmt == SGP_STORE_BF16) launch_gather<SGP_STORE_BF16>(vec, grid, s, x, xrs, xbs, step, node, n_index, out, ors, obs, feat);
    else launch_gather<SGP_STORE_F16>(vec, grid, s, x, xrs, xbs, step, node, n_index, out, ors, obs, feat);
    return sgp::check_launch("gather_rows_16");
}

}  // extern "C"
