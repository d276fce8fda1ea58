// Windowed reservoir, last state only: the echo-state baseline's call shape (reference:
// lib/nn/models/esn_model.py:41-43 -> lib/nn/reservoir/reservoir.py:158-186 with return_last_state=True).
//
//   h_l[t] = (1 - a_l) h_l[t-1] + a_l act(W_ih,l x_l[t] + b_l + W_hh,l h_l[t-1]),  x_0[t] = [x[t] | u[t]],  x_l[t] = h_{l-1}[t]
//
// for M = B * N independent sequences of S = 12 .. 24 steps; only h_l[S-1] is wanted.  The sequence kernels
// (reservoir_impl.h, reservoir_stack.hip) are built for few long chains; this is the opposite regime: tens of
// thousands of short ones.  Mapping: a wave owns ONE tile of 16 sequences and runs ALL layers of a step itself.
// Every layer's state stays in registers for the whole window in the accumulator layout of
// v_mfma_f32_16x16x4_f32 (lane = sequence n + 16 q, register r <-> feature 16 jt + 4 q + r), which is also the
// B-operand layout of the next contraction (reservoir_impl.h's header): the recurrent part of layer l and the
// input part of layer l + 1 both consume h_l's registers directly, so nothing of a step leaves the wave (three
// instance classes -- <8, 1>, <1, 6..8>, <16, 1> -- do not fit 256 VGPRs and pass part of it through scratch:
// DESIGN 4.1e).  HBM is
// touched for the input rows of layer 0 -- read where they lie, by (batch, step, node) strides, from up to two
// sources (x and the exogenous u) -- and for one final store per layer.
// Weights: fragment order, in LDS when all layers fit (R <= 64), else read in the same order from the packed
// global buffer (L2-resident: every wave of the launch reads the same few hundred KB, coalesced 1 KB per operand).
// Arithmetic: exact fp32 products on the fp32 matrix cores, fp32 accumulation (the contract of sgp_reservoir_f32).

#pragma once
#include "reservoir_impl.h"
#include <utility>

namespace sgp_win {
using sgp::f32x4;
using namespace sgp_res;

constexpr int kMaxLayers = 8;
constexpr int kMaxStateTiles = 24;      // L * JT register tiles of state per wave (96 VGPRs)

// ---- packed layout (floats), layer after layer ----------------------------------------------------------
//   bias [JT][4 q][4 r]                 = b[16 jt + 4 q + r]
//   Wx   [JT][NK][64 lanes][4 s]        = W_ih[16 jt + (l&15)][16 kb + 4 (l>>4) + s]   NK = ceil(F / 16) (layer 0), JT (deeper)
//   Wh   [JT][JT][64 lanes][4 s]        = W_hh[16 jt + (l&15)][16 kb + 4 (l>>4) + s]
// (zero past R / F).  The input part uses the k order of the recurrent part, so a deeper layer reads its input
// from the registers of the layer below.
__host__ __device__ constexpr long long layer_floats(int JT, int NK) {
    return (long long)JT * 16 + (long long)JT * NK * 256 + (long long)JT * JT * 256;
}
__host__ __device__ constexpr long long pack_floats(int JT, int NK0, int L) {
    return layer_floats(JT, NK0) + (long long)(L - 1) * layer_floats(JT, JT);
}
// register tiles per layer: the widths the kernels are instantiated for
__host__ __device__ constexpr int pad_jt(int R) {
    const int jt = (R + 15) / 16;
    return jt <= 4 ? jt : (jt <= 8 ? 8 : 16);
}

struct WinArgs {
    const float* x; long long xbs, xss, xns; int Fx;      // features 0 .. Fx-1 of layer 0
    const float* u; long long ubs, uss, uns; int Fu;      // features Fx .. Fx+Fu-1 (null: none)
    const int* step_start;                                // [B] first step of batch item b (null: 0)
    const float* wp;                                      // packed weights of the layers this launch runs
    const float* h0; long long h0_layer;                  // initial states [L][M][R] (null: zeros), floats per layer
    float* out; long long ors;                            // last states: out[m * ors + l * R + j]
    float* seq;                                           // L == 1 only: every step's state [S][M][R] (null: none)
    float alpha[kMaxLayers], one_minus_alpha[kMaxLayers];
    int act, S, N, R, nk0, ovec;
    long long M;
};

template <int JT, int L, bool WLDS>
__global__ __launch_bounds__(256) void reservoir_window(WinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float* wsrc = a.wp;
    if constexpr (WLDS) {
        const int total4 = (int)(pack_floats(JT, a.nk0, L) / 4);
        for (int i = threadIdx.x; i < total4; i += blockDim.x)
            reinterpret_cast<f32x4*>(lds)[i] = reinterpret_cast<const f32x4*>(a.wp)[i];
        __syncthreads();
        wsrc = lds;
    }
    constexpr int NH = JT == 16 ? 2 : 1;                   // halves each summation chain is cut into
    const int lane = threadIdx.x & 63;
    const int n_in = lane & 15, q = lane >> 4;
    const long long tile = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long m = tile * 16 + n_in;
    if (tile * 16 >= a.M) return;                          // wave-uniform (after the only barrier)
    const bool ok = m < a.M;
    const long long mc = ok ? m : a.M - 1;                 // lanes past the end compute on a valid row, store nothing
    const long long bi = mc / a.N, ni = mc - bi * a.N;
    const int F = a.Fx + a.Fu;
    const long long t0 = a.step_start ? a.step_start[bi] : 0;
    const float* xrow = a.x + bi * a.xbs + t0 * a.xss + ni * a.xns;
    const float* urow = a.u ? a.u + bi * a.ubs + t0 * a.uss + ni * a.uns : a.x;

    f32x4 h[L][JT];
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            h[l][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.h0) {
                const int j0 = 16 * jt + 4 * q;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (j0 + r < a.R) h[l][jt][r] = a.h0[l * a.h0_layer + mc * a.R + j0 + r];
            }
        }
    // one chunk of 16 input features: this lane's four (k = 16 kb + 4 q + s), zero past F
    auto load_x = [&](int t, int kb, float (&v)[4]) {
        const float* xp = xrow + (long long)t * a.xss;
        const float* up = urow + (long long)t * a.uss;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = 16 * kb + 4 * q + s;
            v[s] = k < a.Fx ? xp[k] : (k < F ? up[k - a.Fx] : 0.f);
        }
    };
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0): retire the initial-state loads here (reservoir_impl.h)
    for (int t = 0; t < a.S; ++t) {
        int wo = 0;
        asm volatile("" : "+v"(wo));                       // keep the weight fragments in LDS / L2, not hoisted into VGPRs
        const float* wl = wsrc + wo;
        float xc[NH][4];
#pragma unroll
        for (int c = 0; c < NH; ++c) {                     // lands under the recurrent part of layer 0
#pragma unroll
            for (int s = 0; s < 4; ++s) xc[c][s] = 0.f;
            if (c < a.nk0) load_x(t, c, xc[c]);
        }
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int nk = l == 0 ? a.nk0 : JT;
            const float* bias = wl;
            const float* wx = wl + JT * 16;
            const float* wh = wx + (long long)JT * nk * 256;
            wl = wh + JT * JT * 256;
            // separate summation chains for the recurrent and the input part (NH of each): a single fp32 chain over
            // up to 512 products is where a wide non-contractive (relu) layer loses its digits
            f32x4 acc[NH][JT], accx[NH][JT];
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                acc[0][jt] = *reinterpret_cast<const f32x4*>(bias + jt * 16 + q * 4);
                accx[0][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 1; c < NH; ++c) acc[c][jt] = accx[c][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // recurrent part: k-step (kb, s) <-> register s of state tile kb
#pragma unroll
            for (int kb = 0; kb < JT; ++kb) {
                f32x4 wf[JT];
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
                    wf[jt] = *reinterpret_cast<const f32x4*>(wh + ((jt * JT + kb) * 64 + lane) * 4);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
                        acc[kb * NH / JT][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[jt][s], h[l][kb][s], acc[kb * NH / JT][jt], 0, 0, 0);
            }
            // input part
            if (l == 0) {
                for (int kb = 0; kb < nk; kb += NH) {
                    float xn[NH][4];
#pragma unroll
                    for (int c = 0; c < NH; ++c) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) xn[c][s] = 0.f;
                        if (kb + NH + c < nk) load_x(t, kb + NH + c, xn[c]);
                    }
#pragma unroll
                    for (int c = 0; c < NH; ++c) {
                        if (kb + c >= nk) continue;        // wave-uniform
#pragma unroll
                        for (int jt = 0; jt < JT; ++jt) {
                            const f32x4 wv = *reinterpret_cast<const f32x4*>(wx + ((long long)(jt * nk + kb + c) * 64 + lane) * 4);
#pragma unroll
                            for (int s = 0; s < 4; ++s)
                                accx[c][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xc[c][s], accx[c][jt], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < NH; ++c)
#pragma unroll
                        for (int s = 0; s < 4; ++s) xc[c][s] = xn[c][s];
                }
            } else {
#pragma unroll
                for (int kb = 0; kb < JT; ++kb) {
                    f32x4 wf[JT];
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
                        wf[jt] = *reinterpret_cast<const f32x4*>(wx + ((jt * JT + kb) * 64 + lane) * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int jt = 0; jt < JT; ++jt)
                            accx[kb * NH / JT][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[jt][s], h[l > 0 ? l - 1 : 0][kb][s],
                                                                                     accx[kb * NH / JT][jt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
                for (int c = 1; c < NH; ++c) { acc[0][jt] += acc[c][jt]; accx[0][jt] += accx[c][jt]; }
                acc[0][jt] += accx[0][jt];
            }
            // activation (reservoir_impl.h's forms)
            if (a.act == SGP_ACT_TANH) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][jt][r] = tanh_r(acc[0][jt][r]);
            } else if (a.act == SGP_ACT_RELU) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][jt][r] = fmaxf(acc[0][jt][r], 0.f);
            } else if (a.act == SGP_ACT_TANH_REL) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][jt][r] = tanh_rel(acc[0][jt][r]);
            } else if (a.act == SGP_ACT_SELF_NORM) {
                float ss = 0.f;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ss = fmaf(acc[0][jt][r], acc[0][jt][r], ss);
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);   // F.normalize(eps=1e-12)
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[0][jt][r] *= inv;
            }
            const float al = a.alpha[l], oma = a.one_minus_alpha[l];
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    h[l][jt][r] = a.act == SGP_ACT_TANH ? leak_tanh_r(h[l][jt][r], acc[0][jt][r], al, oma)
                                                        : leak(h[l][jt][r], acc[0][jt][r], al, oma);
        }
        if constexpr (L == 1) {
            // layer-by-layer form (L R > 256): the sequence of this layer for the next one, [S][M][R]
            if (a.seq && ok) {
                float* sp = a.seq + ((long long)t * a.M + m) * a.R;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) {
                    const int j0 = 16 * jt + 4 * q;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (j0 + r < a.R) sp[j0 + r] = h[0][jt][r];
                }
            }
        }
    }
    if (!ok) return;
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j0 = 16 * jt + 4 * q;
            float* op = a.out + m * a.ors + (long long)l * a.R + j0;
            if (a.ovec) {
                if (j0 < a.R) *reinterpret_cast<f32x4*>(op) = h[l][jt];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (j0 + r < a.R) op[r] = h[l][jt][r];
            }
        }
}

using WinKernel = void (*)(WinArgs);
// instantiated per width class in reservoir_window.hip (JT 1, 2), reservoir_window_mid.hip (3, 4) and
// reservoir_window_wide.hip (8, 16); nullptr: not built
WinKernel resolve_narrow(int jt, int L);
WinKernel resolve_mid(int jt, int L);
WinKernel resolve_mid_stream(int jt, int L);
WinKernel resolve_wide(int jt, int L);

template <int JT, bool WLDS, int... Ls>
WinKernel pick_layers(int L, std::integer_sequence<int, Ls...>) {
    WinKernel k = nullptr;
    ((L == Ls + 1 ? (k = reservoir_window<JT, Ls + 1, WLDS>, 0) : 0), ...);
    return k;
}

}  // namespace sgp_win
