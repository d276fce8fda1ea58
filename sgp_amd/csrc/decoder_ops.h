// Element-wise pieces shared by the decoder kernels (decoder.hip: the grouped input layer,
// decoder_mlp.hip: the dense layers of the MLP and readout): activations, their derivatives and the
// Philox dropout mask, so that every layer of the model draws its mask from the same (seed, flat index)
// scheme and the backward passes recompute it instead of storing it.
#pragma once
#include "common.h"
#include "device_math.h"

namespace {

// Philox4x32-10 keyed by the call's seed, counter = flat element index (row * width + column): the
// backward pass recomputes the mask from (seed, index) instead of storing it.
__device__ __forceinline__ unsigned philox_word(unsigned long long idx, unsigned k0, unsigned k1) {
    unsigned c0 = (unsigned)idx, c1 = (unsigned)(idx >> 32), c2 = 0x53475021u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
__device__ __forceinline__ float keep_factor(unsigned long long idx, unsigned thresh, unsigned k0, unsigned k1, float scale) {
    if (thresh == 0u) return 1.f;
    return philox_word(idx, k0, k1) >= thresh ? scale : 0.f;
}

__device__ __forceinline__ float activate(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);                                   // relu
    if (act == 2) return v * sgp::sigmoid_f32(v);                        // silu = x * sigmoid(x)
    if (act == 3) return v > 0.f ? v : sgp::expm1_f32(v);                // elu, alpha = 1
    return v;
}

__device__ __forceinline__ float dactivate(float z, int act) {
    if (act == 1) return z > 0.f ? 1.f : 0.f;
    if (act == 2) { const float sg = sgp::sigmoid_f32(z); return sg * (1.f + z * (1.f - sg)); }
    if (act == 3) return z > 0.f ? 1.f : sgp::exp_f32(z);
    return 1.f;
}

}  // namespace

static inline void set_dropout(unsigned& thresh, unsigned& k0, unsigned& k1, float& scale, double p, uint64_t seed) {
    double t = p * 4294967296.0;
    thresh = p > 0.0 ? (unsigned)(t < 1.0 ? 1.0 : (t > 4294967295.0 ? 4294967295.0 : t)) : 0u;
    k0 = (unsigned)seed; k1 = (unsigned)(seed >> 32);
    scale = (float)(1.0 / (1.0 - p));
}
