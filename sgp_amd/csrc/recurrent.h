// What the window kernels of rnn_window.hip and rnn_impute.hip share: which sequence and which hidden columns a lane
// owns, the GRU cell forward and backward, and the store of a gate row's four blocks.  Weights are read in the
// fragment order of frag.h.
#pragma once
#include "frag.h"

namespace sgp {

// A workgroup owns ONE tile of 16 sequences for the whole window; its waves split the JT = H / 16 column tiles of the
// hidden state, CT consecutive tiles per wave, all gates of a column in the same wave.  Lane (n = lane & 15,
// q = lane >> 4) holds features col(c) + 0 .. 3 of sequence m for each of its tiles c: 16 contiguous bytes of every
// [.., M, H] buffer.  Lanes past the end of the batch (!ok) and tiles past the end of H (!tv[c], wave-uniform) compute
// on a valid row (mc) and a valid tile (jt[c]) -- they take part in the MFMAs and the barriers -- and store nothing.
template <int CT>
struct SeqTile {
    int lane, wave, n, q;
    long long m, mc;
    bool ok;
    int jt[CT];
    bool tv[CT];
    __device__ __forceinline__ SeqTile(long long M, int JT)
        : lane(threadIdx.x & 63), wave(threadIdx.x >> 6), n(lane & 15), q(lane >> 4),
          m((long long)blockIdx.x * 16 + n), mc(m < M ? m : M - 1), ok(m < M) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            tv[c] = wave * CT + c < JT;
            jt[c] = tv[c] ? wave * CT + c : JT - 1;
        }
    }
    __device__ __forceinline__ int col(int c) const { return 16 * jt[c] + 4 * q; }
};

// GRU, one step:  r, z = s(.), n = tanh(gx_n + r hn), h' = (1 - z) n + z h;  hn = W_hn h + b_hn.
// The expressions of both directions are written once, here, in the order the kernels always had them: under
// -ffp-contract=fast the backend fuses what it sees after inlining, and it has to see the same thing in every kernel.
struct GruStep { f32x4 r, z, n, h; };
__device__ __forceinline__ GruStep gru_step(f32x4 r_pre, f32x4 z_pre, f32x4 gxn, f32x4 hn, f32x4 h) {
    const f32x4 r = sigmoid4(r_pre), z = sigmoid4(z_pre);
    const f32x4 nn = tanh4(gxn + r * hn);
    return GruStep{r, z, nn, (1.f - z) * nn + z * h};
}

// Its adjoint at the saved r, z, n, hn: the gradients of the three pre-activations, of hn (= dn r, the hidden side's
// third block) and keep = dh z, the direct path to dh of the step before.
struct GruStepBwd { f32x4 dar, daz, dan, dhn, keep; };
__device__ __forceinline__ GruStepBwd gru_step_bwd(f32x4 dh, f32x4 r, f32x4 z, f32x4 nn, f32x4 hn, f32x4 h_prev) {
    const f32x4 dan = dh * (1.f - z) * (1.f - nn * nn);
    const f32x4 daz = dh * (h_prev - nn) * z * (1.f - z);
    const f32x4 dar = dan * hn * r * (1.f - r), dhn = dan * r;
    return GruStepBwd{dar, daz, dan, dhn, dh * z};
}

// the four blocks of a gate row [4 H] (global, or its copy in LDS) at a lane's columns
__device__ __forceinline__ void st_gates(float* grow, int H, int col, f32x4 g0, f32x4 g1, f32x4 g2, f32x4 g3) {
    st4(grow + col, g0); st4(grow + H + col, g1); st4(grow + 2 * H + col, g2); st4(grow + 3 * H + col, g3);
}

}  // namespace sgp
