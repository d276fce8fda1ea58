// Small device helpers with more than one user: the tanh family of the reservoir kernels (also the tanh of the DCRNN,
// Graph WaveNet and LSTM / GRU cells), the sigmoid of every gate and of silu, the full-accuracy exponential family of
// the attention softmax and of ELU, and the 16-byte load / store.
#pragma once
#include "common.h"

namespace sgp {

__device__ __forceinline__ float sigmoid_f32(float v) { return __builtin_amdgcn_rcpf(1.f + __expf(-v)); }
// the library's exp / log / expm1 (about 1 ulp, every range), not the fast hardware approximations: a softmax weight is
// exp(s - max) with s of any size, and ELU's expm1 has to be relative-accurate near zero
__device__ __forceinline__ float exp_f32(float v) { return expf(v); }
__device__ __forceinline__ float log_f32(float v) { return logf(v); }
__device__ __forceinline__ float expm1_f32(float v) { return expm1f(v); }
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

}  // namespace sgp

namespace sgp_res {
using sgp::f32x4;

// tanh(x) = 1 - 2 r(x), r(x) = 1 / (1 + e^{2x}): mul, v_exp_f32, add, v_rcp_f32 (two of them quarter-rate) + one fma --
// and the fma disappears into the leak,
//     h' = (1-a) h + a tanh(x) = fma(-2a, r, fma(1-a, h, a)),
// so activation + leak are 6 VALU instructions per value.  No branch, no overflow case: e^{2x} -> inf gives r = 0, -> 0
// gives r = 1.  ABSOLUTE error < 3e-7 everywhere (tested): fine for states of order 1 -- every reservoir whose bias is
// the reference's U(-1, 1) -- but not for a reservoir whose bias AND input scaling are tiny (states of 1e-6 came out 6 %
// off where the reference's tanh is relative-accurate; tests/test_gpu_split_contract.py found it).  Such layers are
// run with SGP_ACT_TANH_REL (the Python layer picks it when max |bias| < 0.25):
//   |x| >= 0.25: 1 - 2 / (1 + e^{2x})                                  (absolute 1.2e-7, i.e. relative <= 5e-7 there)
//   |x| <  0.25: x (1 + x^2 (-1/3 + x^2 (2/15 - x^2 17/315)))          (next term 62/2835 x^8 <= 9e-8 relative)
// 12 instructions + 2 for the leak -- measured +15 % on the large-N bf16-piece layer, +4-7 % on the split-J form, which
// is why it is not the default form.
__device__ __forceinline__ float tanh_r(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(x * 2.885390081777927f));
}
// four at a time: the multiply and the add as packed instructions (same results: the operations are the same)
__device__ __forceinline__ f32x4 tanh_r4(f32x4 x) {
    const f32x4 y = x * 2.885390081777927f;
    f32x4 e = {__builtin_amdgcn_exp2f(y[0]), __builtin_amdgcn_exp2f(y[1]), __builtin_amdgcn_exp2f(y[2]), __builtin_amdgcn_exp2f(y[3])};
    e = e + 1.f;
    return f32x4{__builtin_amdgcn_rcpf(e[0]), __builtin_amdgcn_rcpf(e[1]), __builtin_amdgcn_rcpf(e[2]), __builtin_amdgcn_rcpf(e[3])};
}
__device__ __forceinline__ float tanh_f32(float x) { return fmaf(-2.f, tanh_r(x), 1.f); }
__device__ __forceinline__ float leak_tanh_r(float h, float r, float alpha, float one_minus_alpha) {
    return fmaf(-2.f * alpha, r, fmaf(one_minus_alpha, h, alpha));
}
__device__ __forceinline__ float tanh_rel(float x) {
    const float big = fmaf(-2.f, tanh_r(x), 1.f);
    const float x2 = x * x;
    const float p = fmaf(x2, fmaf(x2, fmaf(x2, -17.f / 315.f, 2.f / 15.f), -1.f / 3.f), 1.f);
    return fabsf(x) < 0.25f ? x * p : big;
}
// leak with the activation value `v` (any activation)
__device__ __forceinline__ float leak(float h, float v, float alpha, float one_minus_alpha) {
    return one_minus_alpha * h + alpha * v;
}

}  // namespace sgp_res

namespace sgp {

// the gates of the LSTM / GRU cells, four features of a lane at a time
__device__ __forceinline__ f32x4 sigmoid4(f32x4 v) { return f32x4{sigmoid_f32(v[0]), sigmoid_f32(v[1]), sigmoid_f32(v[2]), sigmoid_f32(v[3])}; }
__device__ __forceinline__ f32x4 tanh4(f32x4 v) {
    return f32x4{sgp_res::tanh_f32(v[0]), sgp_res::tanh_f32(v[1]), sgp_res::tanh_f32(v[2]), sgp_res::tanh_f32(v[3])};
}

}  // namespace sgp
