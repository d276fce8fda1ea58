// Leaky echo-state layer with the whole time loop on the device (reference:
// lib/nn/reservoir/reservoir.py:77-81 stepped by the Python loop at :170-183).
//
//   h[t] = (1-a) h[t-1] + a * act( x[t] W_ih^T + b + h[t-1] W_hh^T )
//
// Mapping to gfx950: nodes are independent, time is sequential.  A wave owns NT tiles of 16
// nodes and keeps their state in registers for all T steps.  The contraction is computed
// TRANSPOSED on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32):
//     D[j, n] += W[j, k] * hT[k, n]
// so that the accumulator layout (lane = node n + 16*q, register r  <->  feature 16*jt+4*q+r)
// is already the B-operand layout the next step needs: k-step (kb, s) of the recurrent part
// consumes register s of state tile kb directly, with the k order of every 16-block permuted
// to (4*q + s).  The same permutation is baked into the packed W_hh fragments, so the state
// never leaves its registers and there is no transpose, shuffle or LDS round trip per step.
// Weights live in LDS in fragment order (one conflict-free ds_read per MFMA operand); when a
// layer's weights exceed the LDS they are read in the same order from a global workspace
// (L2-resident, coalesced 256 B per operand).

#pragma once
#include "common.h"
#include "device_math.h"
#include <stdlib.h>

namespace sgp_res {
using sgp::f32x4;


// ---- packed layout (floats) ---------------------------------------------------------------
//   bias  [JT][4 q][4 r]                      = b[16 jt + 4 q + r]
//   Wx    [JT][NKX/4][64 lanes][4]            = W_ih[16 jt + (l&15)][(l>>4) * NKX + ks], ks = 4 k4 + s
//         ([JT][NKX][64 lanes] when NKX < 4): one 16-byte read per lane serves 4 MFMAs
//   Wh    [JT][JT kb][64 lanes][4 s]          = W_hh[16 jt + (l&15)][16 kb + 4 (l>>4) + s]
// (zero where the index runs past R or F).
__host__ __device__ constexpr long long packed_floats(int JT, int NKX) {
    return (long long)JT * 16 + (long long)JT * NKX * 64 + (long long)JT * JT * 256;
}

// sizes and shape classes of the other packs (their layouts: reservoir_bf3.h, reservoir_splitj_bf3.h)
__host__ __device__ constexpr int bf3_kbh(int JT) { return (JT + 1) / 2; }
__host__ __device__ constexpr int bf3_kbx(int NKX) { return (NKX + 7) / 8; }
__host__ __device__ constexpr long long bf3_packed_bytes(int JT, int NKX) {
    return (long long)JT * 64 + (long long)JT * (bf3_kbh(JT) + bf3_kbx(NKX)) * 3 * 1024;
}
// narrow reservoirs and inputs: the state (16 JT), the input rows (4 NKX values per node) and the pieces of one
// k-block fit the 128 registers of four waves per SIMD
__host__ __device__ constexpr bool bf3_supported(int JT, int NKX) {
    return (JT == 2 || JT == 4) && (NKX == 4 || NKX == 8 || NKX == 16) && bf3_packed_bytes(JT, NKX) <= 64 * 1024;
}
// wide reservoirs (reservoir_layer_stream_bf3): bias [256] fp32, then per (k-block, half of the
// output tiles) 8 tiles x 3 pieces x 64 lanes x 16 bytes -- the order the kernel streams them through the LDS
__host__ __device__ constexpr bool sbf3_supported(int JT, int NKX) { return JT == 16 && NKX % 8 == 0 && NKX <= 32; }
__host__ __device__ constexpr long long sbf3_packed_bytes(int JT, int NKX) {
    return 1024 + 2ll * (JT / 2 + NKX / 8) * 8 * 3 * 1024;
}
__host__ __device__ constexpr bool sjbf3_supported(int JT, int NKX) { return (JT == 4 || JT == 8) && (NKX <= 8 || NKX == 16); }
// fp16 fragments of the recurrent blocks: [JT x 16 row scales 2^(-e_j - 14)] [JT][KBH][2 pieces][64 lanes][16 B]
__host__ __device__ constexpr long long sj16_packed_bytes(int JT) { return JT * 64ll + (long long)JT * bf3_kbh(JT) * 2 * 1024; }

// ---- workspace layout (bytes) ---------------------------------------------------------------
// Every region of the sgp_reservoir_workspace_bytes(F, R) scratch buffer, for the host, the pack kernels and the layer
// kernels alike (a region a shape class has no use for stays 0).  A kernel that holds a pack's base pointer reaches the
// regions behind it by the difference of two members.
struct ResLayout {
    long long fp32 = 0;                                  // exact-fp32 fragments (pack_weights)
    long long bf3 = 0, sj16 = 0;                         // bf16-piece fragments; split-J two-piece fp16 pack of W_hh
    long long bf3h = 0, bf3h_scales = 0, bf3h_state = 0; // large-N fp16 pack, its JT x 16 row scales (contiguous: one LDS copy), state-test word
    long long sbf3 = 0, sbf3_dump = 0;                   // streamed bf16 pack + the kernel's dump KB
    long long sbf3h = 0, sbf3h_dump = 0, sbf3h_scales = 0, sbf3h_state = 0;   // its fp16 copy, dump KB, row scales, state-test word
    long long splitj_dump = 0, total = 0;                // the split-J bf16-piece kernel's dump KB (last)
    __host__ __device__ constexpr ResLayout(int jt, int nkx) {
        long long at = (packed_floats(jt, nkx) * 4 + 255) / 256 * 256;
        if (bf3_supported(jt, nkx) || sjbf3_supported(jt, nkx)) { bf3 = at; at += bf3_packed_bytes(jt, nkx); }
        if (sjbf3_supported(jt, nkx)) { sj16 = at; at += sj16_packed_bytes(jt); }
        if (bf3_supported(jt, nkx)) {
            bf3h = at; bf3h_scales = bf3h + bf3_packed_bytes(jt, nkx); bf3h_state = bf3h_scales + jt * 64;
            at = bf3h_state + 256;
        }
        if (sbf3_supported(jt, nkx)) {
            sbf3 = at; sbf3_dump = sbf3 + sbf3_packed_bytes(jt, nkx);
            sbf3h = sbf3_dump + 1024; sbf3h_dump = sbf3h + sbf3_packed_bytes(jt, nkx);
            sbf3h_scales = sbf3h_dump + 1024; sbf3h_state = sbf3h_scales + 1024;
            at = sbf3h_state + 256;
        }
        splitj_dump = (at + 255) / 256 * 256;
        total = splitj_dump + 1024;
    }
};

struct ResArgs {
    const float* x; long long xrs, xss;
    const float* wp;                 // packed weights (global workspace)
    const void* wp_bf3;              // the same weights as bf16 piece fragments (reservoir_bf3.h), or null
    const void* wp_h16;              // W_hh as scaled two-piece fp16 fragments (reservoir_splitj_bf3.h), or null
    const void* wp_h16l;             // large-N form of the same: pack_weights_bf3h's buffer (reservoir_bf3.h), or null
    const void* wp_h16s;             // wide (R = 256) form of the same: pack_weights_sbf3h's buffer, or null
    float* dump;                     // 1 KB of device scratch: unconditional stores of lanes that own no row (split-J bf16 form)
    const int* bad_state;            // device word: 1 = some initial state lies outside [-1, 1] (null: no initial state given)
    const int* pred; int pred_want;  // launch predicate of reservoir_layer_bf3 (the kernel exits unless *pred == pred_want)
    float* out; long long ors, oss;
    float* h_state;
    float alpha, one_minus_alpha;
    int act, T, N, F, R;
    int tiles_per_wave, n_tiles;
    // time pieces side by side (sgp_reservoir_pieces_f32; split-J bf16-piece kernel only): workgroup (tile, p) runs piece p
    // -- x + p * px, out + p * po, h_state + p * ps, T steps (the last piece: t_last) -- and with no_store leaves only its
    // final state behind (the warm-up of a piece that starts from zero)
    int n_pieces, t_last, no_store;
    long long px, po, ps;
};

// ---- launch plan (built by plan_reservoir, reservoir.hip; shown by sgp_reservoir_describe) ----------------------
enum ResForm { kFormLayer, kFormBf3, kFormSplitj, kFormSplitjBf3, kFormStream, kFormStream8, kFormStreamBf3 };
enum ResPack { kPackFp32 = 1, kPackBf3 = 2, kPackSj16 = 4, kPackBf3h = 8, kPackSbf3 = 16, kPackSbf3h = 32 };
// launch predicate of a part: none, the caller's (pieces entry), or the state-test word "some initial state lies outside
// [-1, 1] (or is NaN)" == 0 / == 1 (the instance whose predicate fails exits at its first instruction)
enum ResPred { kPredNone, kPredCaller, kPredStateInside, kPredStateOutside };
struct ResPart {
    int form, nt;                         // kernel form; tiles per wave of the instance (kFormLayer / kFormBf3)
    bool pair, h16, xvec, ovec, act_tanh; // instance flags: two-tile pair form, two-piece fp16 state, 16-byte x loads /
                                          // out stores, activation compiled in (split-J bf16-piece form)
    long long n0; int n;                  // node range [n0, n0 + n)
    int tiles_per_wave;                   // exact deal: tiles per SIMD (streamed forms: full workgroups), else 0
    unsigned grid, grid_y, block; int lds;
    int pred; bool side;                  // ResPred; runs on the side lane beside the parts after it
};
struct ResPlan {
    int jt, nkx;
    unsigned packs;                       // ResPack bits: exactly what the parts read
    bool state_test;                      // exactly when a part is predicated on the state word
    int n_parts; ResPart part[4];
};
using ResKernel = void (*)(ResArgs);

// waves per SIMD the register budget is sized for (more co-resident waves = the MFMA pipe
// stays busy while another wave runs its activation / loads / stores)
constexpr int min_waves(int JT, int NT) { return JT <= 4 ? 4 : (JT <= 8 ? 2 : 1); }

// XVEC / OVEC: 16-byte input loads / state stores (strides and pointers checked on the host).  A compile
// time switch, not a branch inside the time loop: with both paths in one loop body the compiler's
// s_waitcnt bookkeeping merges their pending loads and serialises every step on vmcnt(0).
template <int JT, int NKX, int NT, bool WLDS, bool XVEC, bool OVEC>
__global__ __launch_bounds__(JT <= 4 ? 1024 : 256, min_waves(JT, NT)) void reservoir_layer(ResArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const float* wsrc = a.wp;
    if constexpr (WLDS) {
        const int total4 = (int)(packed_floats(JT, NKX) / 4);
        for (int i = threadIdx.x; i < total4; i += blockDim.x)
            reinterpret_cast<f32x4*>(lds)[i] = reinterpret_cast<const f32x4*>(a.wp)[i];
        __syncthreads();
        wsrc = lds;
    }
    const float* bias = wsrc;
    const float* wx = wsrc + JT * 16;
    const float* wh = wx + JT * NKX * 64;

    const int lane = threadIdx.x & 63;
    const int n_in = lane & 15, q = lane >> 4;
    // tiles are dealt to waves as evenly as possible: wave w owns [w*n/W, (w+1)*n/W), 0..NT tiles
    int tile0, tile1;
    if (a.tiles_per_wave > 0) {
        // exact deal (16-wave workgroups, one per CU): waves w, w + 4, w + 8, w + 12 share a SIMD and
        // together own `per` consecutive tiles, as evenly as NT allows -- every SIMD of the chip carries
        // the same number of tiles (plan_reservoir; the tiles beyond 1024 x per go to the split-J kernel)
        const int per = a.tiles_per_wave;
        const int wl = threadIdx.x >> 6, c = wl & 3, k = wl >> 2;
        const int base = per >> 2, extra = per & 3;
        tile0 = (blockIdx.x * 4 + c) * per + k * base + min(k, extra);
        tile1 = min(tile0 + base + (k < extra ? 1 : 0), a.n_tiles);
    } else {
        const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        const int n_waves = gridDim.x * (blockDim.x >> 6);
        tile0 = (int)((long long)wave * a.n_tiles / n_waves);
        tile1 = (int)((long long)(wave + 1) * a.n_tiles / n_waves);
    }
    if (tile0 >= tile1) return;

    int node[NT];
    bool ok[NT];
    f32x4 h[NT][JT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        node[i] = (tile0 + i) * 16 + n_in;
        ok[i] = (tile0 + i) < tile1 && node[i] < a.N;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            h[i][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (a.h_state && ok[i]) {
                const int j0 = 16 * jt + 4 * q;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (j0 + r < a.R) h[i][jt][r] = a.h_state[(long long)node[i] * a.R + j0 + r];
            }
        }
    }
    constexpr bool x_vec = XVEC && (NKX % 4 == 0);
    constexpr bool o_vec = OVEC;

    // Retire the initial-state loads HERE, with a wait the compiler can see: otherwise it carries
    // "h may still be in flight" into the loop and, because loads and stores are both pending
    // there, guards the first MFMA of every step with s_waitcnt vmcnt(0) -- which waits for the
    // input rows that were requested a moment ago instead of letting them land under the
    // recurrent part.
    __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0)
    for (int t = 0; t < a.T; ++t) {
        // Keep the weight fragments in LDS/L2: without this the compiler hoists all of them
        // out of the time loop into ~128 VGPRs and occupancy drops to one wave per SIMD.
        int wo = 0;
        asm volatile("" : "+v"(wo));
        const float* bias_t = bias + wo;
        const float* wx_t = wx + wo;
        const float* wh_t = wh + wo;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (tile0 + i >= tile1) continue;          // wave-uniform
            // input operands of this tile: issued first, consumed after the recurrent part so
            // their latency hides under its MFMAs (and under the other waves of the SIMD)
            float xr[NKX];
            {
                const float* xp = a.x + (long long)t * a.xss + (long long)node[i] * a.xrs + q * NKX;
                if constexpr (x_vec) {
#pragma unroll
                    for (int k4 = 0; k4 < NKX / 4; ++k4) {
                        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                        if (ok[i] && q * NKX + 4 * k4 < a.F) v = *reinterpret_cast<const f32x4*>(xp + 4 * k4);
                        xr[4 * k4 + 0] = v.x; xr[4 * k4 + 1] = v.y;
                        xr[4 * k4 + 2] = v.z; xr[4 * k4 + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int ks = 0; ks < NKX; ++ks)
                        xr[ks] = (ok[i] && q * NKX + ks < a.F) ? xp[ks] : 0.f;
                }
            }
            f32x4 acc[JT];
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
                acc[jt] = *reinterpret_cast<const f32x4*>(bias_t + jt * 16 + q * 4);
            // recurrent part: k-step (kb, s) <-> register s of state tile kb
#pragma unroll
            for (int kb = 0; kb < JT; ++kb) {
                f32x4 wf[JT];
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
                    wf[jt] = *reinterpret_cast<const f32x4*>(wh_t + ((jt * JT + kb) * 64 + lane) * 4);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
                        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[jt][s], h[i][kb][s], acc[jt], 0, 0, 0);
                }
            }
            // input part
            if constexpr (NKX % 4 == 0) {
#pragma unroll
                for (int k4 = 0; k4 < NKX / 4; ++k4) {
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt) {
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(wx_t + ((jt * (NKX / 4) + k4) * 64 + lane) * 4);
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[s], xr[4 * k4 + s], acc[jt], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < NKX; ++ks) {
#pragma unroll
                    for (int jt = 0; jt < JT; ++jt)
                        acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wx_t[(jt * NKX + ks) * 64 + lane], xr[ks],
                                                                       acc[jt], 0, 0, 0);
                }
            }
            // activation
            if (a.act == SGP_ACT_TANH) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] = tanh_r(acc[jt][r]);
            } else if (a.act == SGP_ACT_RELU) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] = fmaxf(acc[jt][r], 0.f);
            } else if (a.act == SGP_ACT_TANH_REL) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] = tanh_rel(acc[jt][r]);
            } else if (a.act == SGP_ACT_SELF_NORM) {
                float ss = 0.f;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ss = fmaf(acc[jt][r], acc[jt][r], ss);
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);   // F.normalize(eps=1e-12)
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] *= inv;
            }
            // leak + store
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    h[i][jt][r] = a.act == SGP_ACT_TANH ? leak_tanh_r(h[i][jt][r], acc[jt][r], a.alpha, a.one_minus_alpha)
                                                        : leak(h[i][jt][r], acc[jt][r], a.alpha, a.one_minus_alpha);
                const int j0 = 16 * jt + 4 * q;
                if (ok[i] && j0 < a.R) {
                    float* op = a.out + (long long)t * a.oss + (long long)node[i] * a.ors + j0;
                    if constexpr (o_vec) {
                        *reinterpret_cast<f32x4*>(op) = h[i][jt];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (j0 + r < a.R) op[r] = h[i][jt][r];
                    }
                }
            }
        }
    }
    if (a.h_state) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const int j0 = 16 * jt + 4 * q;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ok[i] && j0 + r < a.R) a.h_state[(long long)node[i] * a.R + j0 + r] = h[i][jt][r];
            }
    }
}


constexpr int kLdsLimit = 160 * 1024;

#include "reservoir_bf3.h"

#ifdef SGP_RES_STREAM_TU
// ---- wide reservoirs (R = 256): weights do not fit the LDS, stream them THROUGH it ----------
// One workgroup = 4 waves (one per SIMD), each wave owns up to 2 node tiles for all T steps.
// The packed weights of a step are cut into blocks of 16 KB -- the fragments of all JT output
// tiles for one k-block of W_hh (JT blocks), then for 4 input k-steps of W_ih (NKX/4 blocks) --
// and the 4 waves fetch every block ONCE per workgroup by LDS-DMA (each wave 4 pieces of 1 KiB)
// into a ring of RING slots, AHEAD blocks ahead of the one being consumed (ring positions run on across the
// steps: the number of blocks per step need not be a multiple of the ring length); all 8 node tiles of the
// workgroup then read it with ds_read_b128.  Before, every wave pulled its own copy of the
// 384 KB through L1/L2 each step (4x the traffic, one wave per SIMD to hide it).
template <int I> struct IntC { static constexpr int value = I; };
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (B < E) { f(IntC<B>{}); static_for<B + 1, E>(f); }
}

__device__ __forceinline__ void res_dma16(const void* sbase, unsigned voff, unsigned lds_off) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(voff), "s"(sbase), "s"(lds_off) : "memory");
}

template <int JT, int NKX, bool XVEC, bool OVEC>
__global__ __launch_bounds__(256, 1) void reservoir_layer_stream(ResArgs a) {
    static_assert(JT % 4 == 0 && NKX % 4 == 0, "stream kernel: 4 pieces per wave, 16-byte input fragments");
    constexpr int NT = 2;
    // 4 slots / 2 ahead.  Round 4 measured 8 / 4 (128 KB): 58.4 against 57-58 ms per 256 steps at N = 100k -- the
    // 37 % of parked wave cycles are not waits for weight blocks
    constexpr int RING = 4, AHEAD = 2;
    constexpr int NB = JT + NKX / 4;                     // blocks per step
    constexpr int SLOT = JT * 1024;                      // bytes per block
    constexpr int PPW = JT / 4;                          // 1-KiB pieces of a block per wave
    static_assert(PPW == 4 || PPW == 2, "stream kernel: 8 or 16 output tiles");
    static_assert((RING & (RING - 1)) == 0 && NB >= AHEAD && AHEAD < RING, "ring positions run on across the steps");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* bias_l = lds + RING * SLOT / 4;               // after the ring slots
    for (int i = threadIdx.x; i < JT * 16; i += 256) bias_l[i] = a.wp[i];
    const float* wx = a.wp + JT * 16;
    const float* wh = wx + JT * NKX * 64;

    const int lane = threadIdx.x & 63;
    const int n_in = lane & 15, q = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile assignment (host: plan_reservoir): full workgroups own 8 tiles, the tail ones 4
    const int full = a.tiles_per_wave;                   // number of workgroups with 2 tiles per wave
    int tile0, tile1;
    if ((int)blockIdx.x < full) { tile0 = ((int)blockIdx.x * 4 + wv) * 2; tile1 = tile0 + 2; }
    else { tile0 = full * 8 + ((int)blockIdx.x - full) * 4 + wv; tile1 = tile0 + 1; }
    tile1 = min(tile1, a.n_tiles);

    int node[NT];
    bool ok[NT];
    f32x4 h[NT][JT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        node[i] = (tile0 + i) * 16 + n_in;
        ok[i] = (tile0 + i) < tile1 && node[i] < a.N;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            float hv[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.h_state && ok[i]) {
                const int j0 = 16 * jt + 4 * q;
                const float* hp = a.h_state + (long long)node[i] * a.R + j0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    hv[r] = hp[r];
            }
            h[i][jt] = f32x4{hv[0], hv[1], hv[2], hv[3]};
        }
    }
    const bool two = tile0 + 1 < tile1;                  // wave-uniform: second tile present
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;
    const unsigned voff = (unsigned)lane * 16u;
    // block b of a step -> the PPW pieces of this wave (jt = PPW wv .. PPW wv + PPW - 1).  The two base
    // pointers are re-laundered every call so that the compiler forms the 96 piece addresses of a
    // step with scalar adds on the spot instead of keeping them all in (spilled) SGPRs.
    const unsigned lds_w = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(PPW * wv) * 1024u);
    const float* wh_w = wh + (long long)(PPW * wv) * JT * 256;
    const float* wx_w = wx + (long long)(PPW * wv) * (NKX / 4) * 256;
    auto fetch = [&](int b, int pos) {                   // block b of a step into ring position pos
        const float* hb = wh_w;
        const float* xb = wx_w;
        unsigned l0 = lds_w;
        asm volatile("" : "+s"(hb), "+s"(xb), "+s"(l0));
        const unsigned slot = l0 + (unsigned)(pos & (RING - 1)) * SLOT;
#pragma unroll
        for (int pjt = 0; pjt < PPW; ++pjt) {
            const float* src = b < JT ? hb + (pjt * JT + b) * 256
                                      : xb + (pjt * (NKX / 4) + (b - JT)) * 256;
            res_dma16(src, voff, slot + (unsigned)pjt * 1024u);
        }
    };
    __builtin_amdgcn_s_waitcnt(0x0F70);                  // initial-state loads retired (see above)
    __syncthreads();
#pragma unroll
    for (int b = 0; b < AHEAD; ++b) fetch(b, b);
    int cnt = 0;                                         // blocks consumed so far (ring position of the next one)

    for (int t = 0; t < a.T; ++t) {
        float xr[NT][NKX];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const float* xp = a.x + (long long)t * a.xss + (long long)node[i] * a.xrs + q * NKX;
            if constexpr (XVEC) {
#pragma unroll
                for (int k4 = 0; k4 < NKX / 4; ++k4) {
                    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (ok[i]) v = *reinterpret_cast<const f32x4*>(xp + 4 * k4);   // F == 4 NKX (host check)
                    xr[i][4 * k4 + 0] = v.x; xr[i][4 * k4 + 1] = v.y;
                    xr[i][4 * k4 + 2] = v.z; xr[i][4 * k4 + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < NKX; ++ks)
                    xr[i][ks] = ok[i] ? xp[ks] : 0.f;
            }
        }
        f32x4 acc[NT][JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_l + jt * 16 + q * 4);
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i][jt] = bv;
        }
        // (compile-time block index: h[.][b] and xr[.][ks] must be register names, a runtime
        // loop here turns both arrays into scratch memory)
        static_for<0, NB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            // AHEAD blocks ahead (the sequence repeats every step, the ring positions run on): position cnt + AHEAD
            // was last read RING - AHEAD blocks ago, which every wave finished before it passed an earlier barrier
            fetch((b + AHEAD) % NB, cnt + AHEAD);
            // block b: its PPW pieces were issued AHEAD fetches ago.  Once per step everything is drained
            // (the input-row loads and state stores of the step boundary share the counter).
            if constexpr (b == 0) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(AHEAD * PPW) : "memory");
            const float* slot = lds + (cnt & (RING - 1)) * (SLOT / 4);
            ++cnt;
            // Round 4: the weight fragment of output tile jt + 1 is requested BEFORE the MFMAs of tile jt issue, and
            // the "second node tile present" test is made once per block instead of once per MFMA pair.  Before,
            // every tile's 8 MFMAs (256 cycles) sat behind a ds_read_b128 + lgkmcnt(0) issued right in front of them
            // and four scalar branches: SQ_WAIT_ANY 37 % of the wave cycles.
            auto run = [&](auto two_c) {
                constexpr bool TWO = decltype(two_c)::value;
                f32x4 wf = *reinterpret_cast<const f32x4*>(slot + lane * 4);
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) {
                    f32x4 wn = wf;
                    if (jt + 1 < JT) wn = *reinterpret_cast<const f32x4*>(slot + ((jt + 1) * 64 + lane) * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if constexpr (b < JT) {
                            acc[0][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], h[0][b][s], acc[0][jt], 0, 0, 0);
                            if constexpr (TWO)
                                acc[1][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], h[1][b][s], acc[1][jt], 0, 0, 0);
                        } else {
                            acc[0][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], xr[0][4 * (b - JT) + s], acc[0][jt], 0, 0, 0);
                            if constexpr (TWO)
                                acc[1][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], xr[1][4 * (b - JT) + s], acc[1][jt], 0, 0, 0);
                        }
                    }
                    wf = wn;
                }
            };
            if (two) run(IntC<1>{}); else run(IntC<0>{});
        });
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (i == 1 && !two) continue;
            if (a.act == SGP_ACT_TANH) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] = tanh_r(acc[i][jt][r]);
            } else if (a.act == SGP_ACT_RELU) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] = fmaxf(acc[i][jt][r], 0.f);
            } else if (a.act == SGP_ACT_TANH_REL) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] = tanh_rel(acc[i][jt][r]);
            } else if (a.act == SGP_ACT_SELF_NORM) {
                float ss = 0.f;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ss = fmaf(acc[i][jt][r], acc[i][jt][r], ss);
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] *= inv;
            }
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    h[i][jt][r] = a.act == SGP_ACT_TANH ? leak_tanh_r(h[i][jt][r], acc[i][jt][r], a.alpha, a.one_minus_alpha)
                                                        : leak(h[i][jt][r], acc[i][jt][r], a.alpha, a.one_minus_alpha);
                const int j0 = 16 * jt + 4 * q;
                if (ok[i]) {                                  // R == 16 JT (host check)
                    float* op = a.out + (long long)t * a.oss + (long long)node[i] * a.ors + j0;
                    if constexpr (OVEC) {
                        *reinterpret_cast<f32x4*>(op) = h[i][jt];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) op[r] = h[i][jt][r];
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the two blocks fetched ahead of the end
    if (a.h_state) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const int j0 = 16 * jt + 4 * q;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ok[i]) a.h_state[(long long)node[i] * a.R + j0 + r] = h[i][jt][r];
            }
    }
}

// ---- 8-wave form (round 4): one node tile per wave, two waves per SIMD --------------------------------------
template <int JT, int NKX, bool XVEC, bool OVEC>
__global__ __launch_bounds__(512, 2) void reservoir_layer_stream8(ResArgs a) {
    static_assert(JT % 8 == 0 && NKX % 4 == 0, "stream8 kernel: JT / 8 pieces per wave, 16-byte input fragments");
    constexpr int NT = 1;
    // 4 slots / 2 ahead.  Round 4 measured 8 / 4 (128 KB): 58.4 against 57-58 ms per 256 steps at N = 100k -- the
    // 37 % of parked wave cycles are not waits for weight blocks
    constexpr int RING = 4, AHEAD = 2;
    constexpr int NB = JT + NKX / 4;                     // blocks per step
    constexpr int SLOT = JT * 1024;                      // bytes per block
    constexpr int PPW = JT / 8;                          // 1-KiB pieces of a block per wave
    static_assert(PPW == 2 || PPW == 1, "stream8 kernel: 8 or 16 output tiles");
    static_assert((RING & (RING - 1)) == 0 && NB >= AHEAD && AHEAD < RING, "ring positions run on across the steps");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* bias_l = lds + RING * SLOT / 4;               // after the ring slots
    for (int i = threadIdx.x; i < JT * 16; i += 512) bias_l[i] = a.wp[i];
    const float* wx = a.wp + JT * 16;
    const float* wh = wx + JT * NKX * 64;

    const int lane = threadIdx.x & 63;
    const int n_in = lane & 15, q = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile assignment (host: plan_reservoir): one tile per wave; full workgroups own 8 tiles (two waves per SIMD:
    // one multiplies while the other requests weight pieces, loads its input row or evaluates tanh), the tail
    // ones 4 (waves 0-3, one per SIMD; waves 4-7 only carry their share of the weight pieces)
    const int full = a.tiles_per_wave;                   // number of workgroups with 8 tiles
    int tile0, tile1;
    if ((int)blockIdx.x < full) { tile0 = (int)blockIdx.x * 8 + wv; tile1 = tile0 + 1; }
    else { tile0 = full * 8 + ((int)blockIdx.x - full) * 4 + wv; tile1 = wv < 4 ? tile0 + 1 : tile0; }
    tile1 = min(tile1, a.n_tiles);
    const bool busy = tile0 < tile1;                     // wave-uniform: this wave owns a tile

    int node[NT];
    bool ok[NT];
    f32x4 h[NT][JT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        node[i] = (tile0 + i) * 16 + n_in;
        ok[i] = (tile0 + i) < tile1 && node[i] < a.N;
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            float hv[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.h_state && ok[i]) {
                const int j0 = 16 * jt + 4 * q;
                const float* hp = a.h_state + (long long)node[i] * a.R + j0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    hv[r] = hp[r];
            }
            h[i][jt] = f32x4{hv[0], hv[1], hv[2], hv[3]};
        }
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;
    const unsigned voff = (unsigned)lane * 16u;
    // block b of a step -> the PPW pieces of this wave (jt = PPW wv .. PPW wv + PPW - 1).  The two base
    // pointers are re-laundered every call so that the compiler forms the 96 piece addresses of a
    // step with scalar adds on the spot instead of keeping them all in (spilled) SGPRs.
    const unsigned lds_w = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(PPW * wv) * 1024u);
    const float* wh_w = wh + (long long)(PPW * wv) * JT * 256;
    const float* wx_w = wx + (long long)(PPW * wv) * (NKX / 4) * 256;
    auto fetch = [&](int b, int pos) {                   // block b of a step into ring position pos
        const float* hb = wh_w;
        const float* xb = wx_w;
        unsigned l0 = lds_w;
        asm volatile("" : "+s"(hb), "+s"(xb), "+s"(l0));
        const unsigned slot = l0 + (unsigned)(pos & (RING - 1)) * SLOT;
#pragma unroll
        for (int pjt = 0; pjt < PPW; ++pjt) {
            const float* src = b < JT ? hb + (pjt * JT + b) * 256
                                      : xb + (pjt * (NKX / 4) + (b - JT)) * 256;
            res_dma16(src, voff, slot + (unsigned)pjt * 1024u);
        }
    };
    __builtin_amdgcn_s_waitcnt(0x0F70);                  // initial-state loads retired (see above)
    __syncthreads();
#pragma unroll
    for (int b = 0; b < AHEAD; ++b) fetch(b, b);
    int cnt = 0;                                         // blocks consumed so far (ring position of the next one)

    for (int t = 0; t < a.T; ++t) {
        float xr[NT][NKX];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const float* xp = a.x + (long long)t * a.xss + (long long)node[i] * a.xrs + q * NKX;
            if constexpr (XVEC) {
#pragma unroll
                for (int k4 = 0; k4 < NKX / 4; ++k4) {
                    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (ok[i]) v = *reinterpret_cast<const f32x4*>(xp + 4 * k4);   // F == 4 NKX (host check)
                    xr[i][4 * k4 + 0] = v.x; xr[i][4 * k4 + 1] = v.y;
                    xr[i][4 * k4 + 2] = v.z; xr[i][4 * k4 + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int ks = 0; ks < NKX; ++ks)
                    xr[i][ks] = ok[i] ? xp[ks] : 0.f;
            }
        }
        f32x4 acc[NT][JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_l + jt * 16 + q * 4);
#pragma unroll
            for (int i = 0; i < NT; ++i) acc[i][jt] = bv;
        }
        // (compile-time block index: h[.][b] and xr[.][ks] must be register names, a runtime
        // loop here turns both arrays into scratch memory)
        static_for<0, NB>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            // AHEAD blocks ahead (the sequence repeats every step, the ring positions run on): position cnt + AHEAD
            // was last read RING - AHEAD blocks ago, which every wave finished before it passed an earlier barrier
            fetch((b + AHEAD) % NB, cnt + AHEAD);
            // block b: its PPW pieces were issued AHEAD fetches ago.  Once per step everything is drained
            // (the input-row loads and state stores of the step boundary share the counter).
            if constexpr (b == 0) asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(AHEAD * PPW) : "memory");
            const float* slot = lds + (cnt & (RING - 1)) * (SLOT / 4);
            ++cnt;
            // Round 4: the weight fragment of output tile jt + 1 is requested BEFORE the MFMAs of tile jt issue, and
            // the "second node tile present" test is made once per block instead of once per MFMA pair.  Before,
            // every tile's 8 MFMAs (256 cycles) sat behind a ds_read_b128 + lgkmcnt(0) issued right in front of them
            // and four scalar branches: SQ_WAIT_ANY 37 % of the wave cycles.
            if (busy) {
                // two output tiles at a time: their MFMAs alternate, so a tile's next MFMA finds its accumulator ready
                f32x4 wa = *reinterpret_cast<const f32x4*>(slot + lane * 4);
                f32x4 wb = *reinterpret_cast<const f32x4*>(slot + (64 + lane) * 4);
#pragma unroll
                for (int jt = 0; jt < JT; jt += 2) {
                    f32x4 na = wa, nb = wb;
                    if (jt + 2 < JT) {
                        na = *reinterpret_cast<const f32x4*>(slot + ((jt + 2) * 64 + lane) * 4);
                        nb = *reinterpret_cast<const f32x4*>(slot + ((jt + 3) * 64 + lane) * 4);
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if constexpr (b < JT) {
                            acc[0][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], h[0][b][s], acc[0][jt], 0, 0, 0);
                            acc[0][jt + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[s], h[0][b][s], acc[0][jt + 1], 0, 0, 0);
                        } else {
                            acc[0][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], xr[0][4 * (b - JT) + s], acc[0][jt], 0, 0, 0);
                            acc[0][jt + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[s], xr[0][4 * (b - JT) + s], acc[0][jt + 1], 0, 0, 0);
                        }
                    }
                    wa = na; wb = nb;
                }
            }
        });
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (!busy) continue;
            if (a.act == SGP_ACT_TANH) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] = tanh_r(acc[i][jt][r]);
            } else if (a.act == SGP_ACT_RELU) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] = fmaxf(acc[i][jt][r], 0.f);
            } else if (a.act == SGP_ACT_TANH_REL) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] = tanh_rel(acc[i][jt][r]);
            } else if (a.act == SGP_ACT_SELF_NORM) {
                float ss = 0.f;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ss = fmaf(acc[i][jt][r], acc[i][jt][r], ss);
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][jt][r] *= inv;
            }
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    h[i][jt][r] = a.act == SGP_ACT_TANH ? leak_tanh_r(h[i][jt][r], acc[i][jt][r], a.alpha, a.one_minus_alpha)
                                                        : leak(h[i][jt][r], acc[i][jt][r], a.alpha, a.one_minus_alpha);
                const int j0 = 16 * jt + 4 * q;
                if (ok[i]) {                                  // R == 16 JT (host check)
                    float* op = a.out + (long long)t * a.oss + (long long)node[i] * a.ors + j0;
                    if constexpr (OVEC) {
                        *reinterpret_cast<f32x4*>(op) = h[i][jt];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) op[r] = h[i][jt][r];
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the two blocks fetched ahead of the end
    if (a.h_state) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
                const int j0 = 16 * jt + 4 * q;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ok[i]) a.h_state[(long long)node[i] * a.R + j0 + r] = h[i][jt][r];
            }
    }
}

// ---- wide reservoirs on the 16-bit matrix cores: the three-piece bf16 products of reservoir_bf3.h with the weight
// fragments streamed through the LDS as above.  A step's fragments -- [k-block][half of the output tiles][tile][3
// pieces][64 lanes][16 B], 24 KB per sub-block (k-block, half), input k-blocks first -- pass through a ring of 4 slots;
// each of the 8 waves fetches 3 KB of every slot by LDS-DMA and multiplies its own node tile against all of it.  The
// state's pieces are cut once per k-block (36 VALU instructions), the chains of two output tiles alternate on the matrix
// pipe: 1152 MFMAs of 17 cycles per tile and step instead of 1536 of 32.
// Memory: a CU moves 24 KB of rows per tile and step (8 KB in, 16 KB out) through a path that turns ~7-10 B/clk around --
// a quarter of the step if the step waits for it.  So nothing waits: the state of step t - 1 is stored one 1-KB piece
// per sub-block DURING step t (the registers hold it until the end of step t anyway), the input rows of step t + 1 are
// requested one piece per sub-block once the input k-blocks of step t are done, and every s_waitcnt counts exactly the
// operations issued since the fetch it needs (all loads and stores unconditional: lanes without a node read row 0 and
// store to a dump area behind the packed weights).
// H16 (tanh, launched under the predicate of reservoir_layer_bf3's H16 instance): the recurrent sub-blocks hold two fp16
// pieces per fragment (16 of their 24 KB: two DMA pieces per wave instead of three) and multiply three products per tile
// instead of six; the accumulators carry the rows' 2^(e_j + 14) (pack_weights_sbf3h) and are scaled back once per step.
template <int JT, int NKX, bool H16 = false>
__global__ __launch_bounds__(512, 2) void reservoir_layer_stream_bf3(ResArgs a) {
    static_assert(sbf3_supported(JT, NKX), "stream bf3 kernel: R = 256, F = 32 .. 128");
    if (a.pred != nullptr && a.pred[0] != a.pred_want) return;
    constexpr int RING = 4, AHEAD = 3;
    constexpr int KBH = JT / 2, KBX = NKX / 8, NSB = 2 * (KBH + KBX);    // sub-blocks per step: (k-block, half), input first
    constexpr int NXL = NKX / 4;                         // 16-byte input loads per lane and step
    constexpr int SLOT = 8 * 3 * 1024;                   // bytes per sub-block
    constexpr int PPW = 3;                               // 1-KiB pieces of a (three-piece) sub-block per wave
    auto two = [](int sb) constexpr { return H16 && sb >= 2 * KBX; };          // a two-piece (recurrent fp16) sub-block
    auto ppw = [two](int sb) constexpr { return two(sb) ? 2 : 3; };
    static_assert(NSB >= JT && 2 * KBX + NXL <= NSB, "one store / one load per sub-block");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* bias_l = lds + RING * SLOT / 4;               // after the ring slots (H16: + the rows' way back behind it)
    constexpr ResLayout L(JT, NKX);
    const char* wpb = static_cast<const char*>(H16 ? a.wp_h16s : a.wp_bf3);
    for (int i = threadIdx.x; i < JT * 16; i += 512) {
        bias_l[i] = reinterpret_cast<const float*>(wpb)[i];
        if constexpr (H16) bias_l[JT * 16 + i] = reinterpret_cast<const float*>(wpb + (L.sbf3h_scales - L.sbf3h))[i];
    }
    float hscale = kSj16StateScale;
    if constexpr (H16) asm("" : "+s"(hscale));

    const int lane = threadIdx.x & 63;
    const int n_in = lane & 15, q = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // tile assignment of reservoir_layer_stream8: full workgroups own 8 tiles, the tail ones 4 (waves 0-3)
    const int full = a.tiles_per_wave;
    int tile0, tile1;
    if ((int)blockIdx.x < full) { tile0 = (int)blockIdx.x * 8 + wv; tile1 = tile0 + 1; }
    else { tile0 = full * 8 + ((int)blockIdx.x - full) * 4 + wv; tile1 = wv < 4 ? tile0 + 1 : tile0; }
    tile1 = min(tile1, a.n_tiles);
    const bool busy = tile0 < tile1;                     // wave-uniform: this wave owns a tile
    const int node = tile0 * 16 + n_in;
    const bool ok = busy && node < a.N;
    float* const dump = reinterpret_cast<float*>(const_cast<char*>(wpb) + (H16 ? L.sbf3h_dump - L.sbf3h : L.sbf3_dump - L.sbf3)) + lane * 4;
    const float* const xrow = a.x + (long long)(ok ? node : 0) * a.xrs + 4 * q;
    float* const orow = a.out + (long long)(ok ? node : 0) * a.ors + 4 * q;

    f32x4 h[JT];
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        h[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a.h_state && ok) h[jt] = *reinterpret_cast<const f32x4*>(a.h_state + (long long)node * a.R + 16 * jt + 4 * q);
    }
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lds;
    const unsigned voff = (unsigned)lane * 16u;
    const unsigned lds_w = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(PPW * wv) * 1024u);
    const char* src_w = wpb + 1024 + (long long)(PPW * wv) * 1024;
    const unsigned lds_w2 = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(2 * wv) * 1024u);      // (two-piece sub-blocks: 16 pieces)
    const char* src_w2 = wpb + 1024 + (long long)(2 * wv) * 1024;
    auto fetch_piece = [&](int sb, int pos, int p, bool tw) {     // this wave's piece p of sub-block sb into ring position pos
        const char* sp = tw ? src_w2 : src_w;
        unsigned l0 = tw ? lds_w2 : lds_w;
        asm volatile("" : "+s"(sp), "+s"(l0));
        const unsigned slot = l0 + (unsigned)(pos & (RING - 1)) * SLOT;
        if constexpr (bf3_abl(64)) return;               // experiment: no weight stream
        res_dma16(sp + (long long)sb * SLOT + p * 1024, voff, slot + (unsigned)p * 1024u);
    };
    auto fetch = [&](int sb, int pos, int np) {
#pragma unroll
        for (int p = 0; p < PPW; ++p)
            if (p < np) fetch_piece(sb, pos, p, np == 2);
    };
    // input rows: register 4 k4 + s <-> feature 16 k4 + 4 q + s (bf3_feature); loaded by hand so that the compiler
    // puts no s_waitcnt of its own between the counted ones
    f32x4 xr[NXL];
    auto load_x = [&](int k4, int t) {
        const float* p = xrow + (long long)t * a.xss + 16 * k4;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(xr[k4]) : "v"(p) : "memory");
    };
    __builtin_amdgcn_s_waitcnt(0x0F70);                  // initial-state loads retired
    __syncthreads();
    static_for<0, AHEAD>([&](auto bc) { constexpr int b = decltype(bc)::value; fetch(b, b, ppw(b)); });
#pragma unroll
    for (int k4 = 0; k4 < NXL; ++k4) load_x(k4, 0);
    int cnt = 0;                                         // sub-blocks consumed so far (ring position of the next one)
    // Sub-block sb + 1 is complete in the LDS before the MFMAs of sub-block sb start (barrier at the top of sb), so the
    // first fragments of sb + 1 are read under the last MFMAs of sb instead of behind the barrier with the pipe idle.
    u32x4 f[6];
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = (reinterpret_cast<const u32x4*>(lds) + lane)[k * 64];

    // memory operations a wave issues in sub-block sb, after its barrier: the 3 DMA pieces of sub-block sb + 3, one
    // 16-byte-per-lane store of the state of the step before (sb < JT), one input load for the next step
    auto ops = [ppw](int sb) constexpr { return ppw((sb + AHEAD) % NSB) + (sb < JT ? 1 : 0) + (sb >= 2 * KBX && sb < 2 * KBX + NXL ? 1 : 0); };

    for (int t = 0; t <= a.T; ++t) {                     // iteration T only stores the last state
        f32x4 acc[JT];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) acc[jt] = *reinterpret_cast<const f32x4*>(bias_l + jt * 16 + q * 4);
        float* const op = (ok && t > 0) ? orow + (long long)(t - 1) * a.oss : dump;      // rows of step t - 1
        const bool real = t < a.T;
        const int tn = t + 1 < a.T ? t + 1 : (a.T > 0 ? a.T - 1 : 0);                     // rows to request: step t + 1
        u32x4 v1, v2, v3;
        static_for<0, NSB>([&](auto sc) {
            constexpr int sb = decltype(sc)::value, blk = sb / 2, half = sb % 2;
            // sub-block sb + 1 (requested two sub-blocks ago, its last piece the last memory operation of that
            // sub-block) must have landed: what may still be in flight is what the sub-block before this one issued
            constexpr int allowed = ops((sb + NSB - 1) % NSB);
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" :: "n"(allowed) : "memory");
            if constexpr (sb < JT) *reinterpret_cast<f32x4*>((ok && t > 0) ? op + 16 * sb : op) = h[sb];
            if constexpr (sb >= 2 * KBX && sb < 2 * KBX + NXL) load_x(sb - 2 * KBX, tn);
            // the pieces of sub-block sb + 3 go into the slot of sub-block sb - 1, which every wave has left; a busy
            // wave requests them one per pair of output tiles INSIDE its MFMA phase (an issue that stalls on a full
            // memory queue then waits under queued matrix work, not in front of it)
            constexpr int fsb = (sb + AHEAD) % NSB;
            const int fpos = cnt + AHEAD;
            if (!(busy && real)) fetch(fsb, fpos, ppw(fsb));
            const u32x4* slot = reinterpret_cast<const u32x4*>(lds + (cnt & (RING - 1)) * (SLOT / 4)) + lane;
            ++cnt;
            const u32x4* next_slot = reinterpret_cast<const u32x4*>(lds + (cnt & (RING - 1)) * (SLOT / 4)) + lane;
            if (busy && real) {
                if constexpr (half == 0) {               // the pieces of a new k-block
                    float v[8];
                    if constexpr (blk < KBX) {
                        asm volatile("" : "+v"(xr[2 * blk]), "+v"(xr[2 * blk + 1]));      // (landed: see `allowed`)
#pragma unroll
                        for (int s = 0; s < 8; ++s) v[s] = xr[2 * blk + (s >> 2)][s & 3];
                    } else {
#pragma unroll
                        for (int s = 0; s < 8; ++s) v[s] = h[2 * (blk - KBX) + (s >> 2)][s & 3];
                    }
                    constexpr bool R = two(sb);
                    if constexpr (R) {
#pragma unroll
                        for (int d = 0; d < 4; ++d) {
                            unsigned hi, lo;
                            sj16_split2s(v[2 * d], v[2 * d + 1], hscale, hi, lo);
                            v1[d] = hi; v2[d] = lo;
                        }
                    } else if constexpr (bf3_abl(2)) {
#pragma unroll
                        for (int d = 0; d < 4; ++d) { v1[d] = __builtin_bit_cast(unsigned, v[2 * d]); v2[d] = __builtin_bit_cast(unsigned, v[2 * d + 1]); v3[d] = v1[d] ^ v2[d]; }
                    } else {
                        bf3_split8(v, v1, v2, v3);
                    }
                }
                // fragment (tile j8 of this half, piece pc) = slot[(j8 * NP + pc) * 64], NP = 3 pieces (2 in a two-piece
                // sub-block).  Pairs of tiles, their chains alternating; the leading pieces multiply first, so that each of
                // the six fragment registers is free for the next pair's piece 6-10 MFMAs before that is used (no second
                // set of registers).  f[3 tile + pc]; a two-piece pair leaves f[2], f[5] alone.
                constexpr bool R = two(sb), Rn = two((sb + 1) % NSB);
                constexpr int NPc = R ? 2 : 3;
                static_for<0, 4>([&](auto jc) {
                    constexpr int jp = decltype(jc)::value;
                    constexpr bool lastp = jp == 3, Rx = lastp ? Rn : R;      // the pair whose fragments are requested now
                    constexpr int NPx = Rx ? 2 : 3;
                    const u32x4* nx = lastp ? next_slot : slot + (jp + 1) * 2 * NPc * 64;
                    auto ldf = [&](auto kc) {
                        constexpr int k = decltype(kc)::value;
                        if constexpr (!bf3_abl(32)) f[k] = nx[((k / 3) * NPx + (k % 3)) * 64];
                    };
                    f32x4& A = acc[8 * half + 2 * jp];
                    f32x4& B = acc[8 * half + 2 * jp + 1];
                    if constexpr (!R) {
                        A = bf3_mfma(f[0], v3, A); B = bf3_mfma(f[3], v3, B);
                        A = bf3_mfma(f[0], v2, A); B = bf3_mfma(f[3], v2, B);
                        A = bf3_mfma(f[0], v1, A); B = bf3_mfma(f[3], v1, B);
                        ldf(Bf3C<0>{}); ldf(Bf3C<3>{});
                        A = bf3_mfma(f[1], v2, A); B = bf3_mfma(f[4], v2, B);
                        A = bf3_mfma(f[1], v1, A); B = bf3_mfma(f[4], v1, B);
                        ldf(Bf3C<1>{}); ldf(Bf3C<4>{});
                        A = bf3_mfma(f[2], v1, A); B = bf3_mfma(f[5], v1, B);
                        if constexpr (!Rx) { ldf(Bf3C<2>{}); ldf(Bf3C<5>{}); }
                    } else {
                        A = sj16_mfma(f[1], v1, A); B = sj16_mfma(f[4], v1, B);        // lo hi
                        ldf(Bf3C<1>{}); ldf(Bf3C<4>{});
                        A = sj16_mfma(f[0], v2, A); B = sj16_mfma(f[3], v2, B);        // hi lo
                        A = sj16_mfma(f[0], v1, A); B = sj16_mfma(f[3], v1, B);        // hi hi
                        ldf(Bf3C<0>{}); ldf(Bf3C<3>{});
                        if constexpr (!Rx) { ldf(Bf3C<2>{}); ldf(Bf3C<5>{}); }            // (an input pair comes next: its third pieces)
                    }
                    if constexpr (jp < ppw(fsb)) fetch_piece(fsb, fpos, jp, two(fsb));
                });
            }
        });
        if (busy && real) {
            if constexpr (H16) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt) acc[jt] *= *reinterpret_cast<const f32x4*>(bias_l + JT * 16 + jt * 16 + q * 4);
            }
            if (H16 || a.act == SGP_ACT_TANH) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] = tanh_r(acc[jt][r]);
            } else if (a.act == SGP_ACT_RELU) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] = fmaxf(acc[jt][r], 0.f);
            } else if (a.act == SGP_ACT_TANH_REL) {
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] = tanh_rel(acc[jt][r]);
            } else if (a.act == SGP_ACT_SELF_NORM) {
                float ss = 0.f;
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) ss = fmaf(acc[jt][r], acc[jt][r], ss);
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
                for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[jt][r] *= inv;
            }
#pragma unroll
            for (int jt = 0; jt < JT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    h[jt][r] = (H16 || a.act == SGP_ACT_TANH) ? leak_tanh_r(h[jt][r], acc[jt][r], a.alpha, a.one_minus_alpha)
                                                              : leak(h[jt][r], acc[jt][r], a.alpha, a.one_minus_alpha);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the sub-blocks and rows requested ahead of the end
    if (a.h_state && ok) {
#pragma unroll
        for (int jt = 0; jt < JT; ++jt)
            *reinterpret_cast<f32x4*>(a.h_state + (long long)node * a.R + 16 * jt + 4 * q) = h[jt];
    }
}

template <int JT, int NKX>
ResKernel resolve_stream(const ResPart& p) {
    if (p.form == kFormStream) return reservoir_layer_stream<JT, NKX, true, true>;
    if (p.form == kFormStream8) return reservoir_layer_stream8<JT, NKX, true, true>;
    if constexpr (sbf3_supported(JT, NKX)) {
        if (p.form == kFormStreamBf3) return p.h16 ? reservoir_layer_stream_bf3<JT, NKX, true> : reservoir_layer_stream_bf3<JT, NKX>;
    }
    return nullptr;
}

#endif  // SGP_RES_STREAM_TU

// ---- small-N variant: one node tile per workgroup, the j-tiles split over its 4 waves -------
// With a few hundred nodes (METR-LA 207, PEMS-BAY 325) there are only a dozen node tiles, and a
// single wave stepping all JT output tiles is a serial chain of JT*(4*JT+NKX) MFMAs per time
// step.  Here the 4 waves of a workgroup (one per SIMD) each compute JT/4 of the output tiles
// for the SAME 16 nodes, then exchange the new state through a double-buffered LDS slab (the
// C-layout tile of a wave is written as-is: it is already the B-operand layout every wave
// needs), one barrier per step.
// Input-row ring of the split-J kernel (time steps): 8 deep when three workgroups fit a CU's LDS anyway
// (narrow inputs), else the deepest of 4 / 3 / 2 that lets three fit (F = R = 64: ring 3, 54 KB per
// workgroup; the split-J tail of a large problem shares its CU's LDS with nothing and lost nothing to
// the shorter ring: N = 100k 4.48 -> 4.30 ms per 256 steps).
constexpr long long splitj_fixed_bytes(int JT, int NKX) {
    return ((long long)JT * 16 + (long long)JT * NKX * 64 + (long long)JT * JT * 256) * 4 + 2ll * JT * 64 * 16 + 2 * 64 * 4;
}
constexpr int splitj_ring(int JT, int NKX) {
    const int opts[] = {8, 4, 3, 2};
    for (int o : opts)
        if (3 * (splitj_fixed_bytes(JT, NKX) + (long long)o * NKX * 64 * 4) <= 160 * 1024) return o;
    return 8;
}

template <int JT, int NKX, bool OVEC>
__global__ __launch_bounds__(256) void reservoir_layer_splitj(ResArgs a) {
    static_assert(JT % 4 == 0, "split-J needs at least one j-tile per wave");
    constexpr int JW = JT / 4;                           // j-tiles per wave
    constexpr int PFD = splitj_ring(JT, NKX);
    extern __shared__ __attribute__((aligned(16))) float lds[];
    {
        const int total4 = (int)(packed_floats(JT, NKX) / 4);
        for (int i = threadIdx.x; i < total4; i += 256)
            reinterpret_cast<f32x4*>(lds)[i] = reinterpret_cast<const f32x4*>(a.wp)[i];
    }
    const float* bias = lds;
    const float* wx = lds + JT * 16;
    const float* wh = wx + JT * NKX * 64;
    f32x4* hbuf = reinterpret_cast<f32x4*>(lds + packed_floats(JT, NKX));   // [2][JT][64] f32x4
    float* red_base = reinterpret_cast<float*>(hbuf + 2 * JT * 64);         // [2][64] self_norm partials
    float* xring = red_base + 2 * 64;                                       // [PFD][NKX][64] input rows

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_in = lane & 15, q = lane >> 4;
    const int node = blockIdx.x * 16 + n_in;
    const bool ok = node < a.N;

    f32x4 h[JT];                                         // full state as B operands
#pragma unroll
    for (int jt = 0; jt < JT; ++jt) {
        float hv[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.h_state && ok) {
            const int j0 = 16 * jt + 4 * q;
            const float* hp = a.h_state + (long long)node * a.R + j0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (j0 + r < a.R) hv[r] = hp[r];
        }
        h[jt] = f32x4{hv[0], hv[1], hv[2], hv[3]};
    }

    // The step is a serial chain (MFMAs -> activation -> LDS exchange -> barrier), so nothing in it
    // may wait for HBM.  Input rows: wave 0 requests the row of step t + PFD - 1 by LDS-DMA
    // (global_load_lds_dword, one per k-step: lane (n, q) fetches x[node n][q NKX + ks]) into a ring
    // of PFD slots and retires the row of step t + 1 with a hand-counted vmcnt before the step's
    // barrier, which publishes it to the other waves.  Results: the state of step t-1 is stored at
    // the top of step t.  The barrier is a bare `s_waitcnt lgkmcnt(0); s_barrier`: hipcc's
    // __syncthreads also drains vmcnt, i.e. waited every step (0.7-1.5 us) for the store and the
    // input request that had just been issued.
    bool x_ok[NKX];
    long long x_off[NKX];
    {
        const int nodec = min(node, a.N - 1);
#pragma unroll
        for (int ks = 0; ks < NKX; ++ks) {
            x_ok[ks] = ok && q * NKX + ks < a.F;
            x_off[ks] = (long long)nodec * a.xrs + min(q * NKX + ks, a.F - 1);
        }
    }
    const unsigned xring_lds = __builtin_amdgcn_readfirstlane(
        (unsigned)(size_t)(__attribute__((address_space(3))) float*)xring);
    auto dma_x = [&](int t) {
        const float* xp = a.x + (long long)min(t, a.T - 1) * a.xss;
        const unsigned base = xring_lds + (unsigned)((t % PFD) * NKX * 256);
#pragma unroll
        for (int ks = 0; ks < NKX; ++ks) {
            const float* src = xp + x_off[ks];
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
                         :: "v"(src), "s"(base + (unsigned)ks * 256u) : "memory");
        }
    };
    bool st_ok[JW];
#pragma unroll
    for (int w = 0; w < JW; ++w) st_ok[w] = ok && 16 * (wave * JW + w) + 4 * q < a.R;
    auto store_h = [&](int t, const f32x4 (&hv)[JW]) {
#pragma unroll
        for (int w = 0; w < JW; ++w) {
            const int j0 = 16 * (wave * JW + w) + 4 * q;
            if (st_ok[w]) {
                float* op = a.out + (long long)t * a.oss + (long long)node * a.ors + j0;
                if constexpr (OVEC) {
                    *reinterpret_cast<f32x4*>(op) = hv[w];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (j0 + r < a.R) op[r] = hv[w][r];
                }
            }
        }
    };
    f32x4 hprev[JW];
#pragma unroll
    for (int w = 0; w < JW; ++w) hprev[w] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();                                     // weights in LDS
    __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0), visible to the compiler
    if (wave == 0) {
        for (int p = 0; p < PFD - 1; ++p) dma_x(p);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // rows 0 .. PFD-2 published

    for (int t = 0; t < a.T; ++t) {
        int wo = 0;
        asm volatile("" : "+v"(wo));                     // keep the fragments in LDS (see above)
        const float* bias_t = bias + wo;
        const float* wx_t = wx + wo;
        const float* wh_t = wh + wo;
        if (t > 0) store_h(t - 1, hprev);
        if (wave == 0) dma_x(t + PFD - 1);               // into the slot consumed one step ago
        f32x4 acc[JW];
#pragma unroll
        for (int w = 0; w < JW; ++w)
            acc[w] = *reinterpret_cast<const f32x4*>(bias_t + (wave * JW + w) * 16 + q * 4);
#pragma unroll
        for (int kb = 0; kb < JT; ++kb) {
            f32x4 wf[JW];
#pragma unroll
            for (int w = 0; w < JW; ++w)
                wf[w] = *reinterpret_cast<const f32x4*>(wh_t + (((wave * JW + w) * JT + kb) * 64 + lane) * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int w = 0; w < JW; ++w)
                    acc[w] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[w][s], h[kb][s], acc[w], 0, 0, 0);
        }
        const float* xrow = xring + (t % PFD) * NKX * 64;
        if constexpr (NKX % 4 == 0) {
#pragma unroll
            for (int k4 = 0; k4 < NKX / 4; ++k4)
#pragma unroll
                for (int w = 0; w < JW; ++w) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(
                        wx_t + (((wave * JW + w) * (NKX / 4) + k4) * 64 + lane) * 4);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc[w] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            wv[s], x_ok[4 * k4 + s] ? xrow[(4 * k4 + s) * 64 + lane] : 0.f, acc[w], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int ks = 0; ks < NKX; ++ks)
#pragma unroll
                for (int w = 0; w < JW; ++w)
                    acc[w] = __builtin_amdgcn_mfma_f32_16x16x4f32(wx_t[((wave * JW + w) * NKX + ks) * 64 + lane],
                                                                   x_ok[ks] ? xrow[ks * 64 + lane] : 0.f, acc[w], 0, 0, 0);
        }
        if (a.act == SGP_ACT_TANH) {
#pragma unroll
            for (int w = 0; w < JW; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[w][r] = tanh_r(acc[w][r]);
        } else if (a.act == SGP_ACT_RELU) {
#pragma unroll
            for (int w = 0; w < JW; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[w][r] = fmaxf(acc[w][r], 0.f);
        } else if (a.act == SGP_ACT_TANH_REL) {
#pragma unroll
            for (int w = 0; w < JW; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[w][r] = tanh_rel(acc[w][r]);
        }
        f32x4* hb = hbuf + (t & 1) * JT * 64;
        if (a.act == SGP_ACT_SELF_NORM) {
            // norm over all R features: partial sums of the 4 waves meet in LDS
            float ss = 0.f;
#pragma unroll
            for (int w = 0; w < JW; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) ss = fmaf(acc[w][r], acc[w][r], ss);
            ss += __shfl_xor(ss, 16);
            ss += __shfl_xor(ss, 32);
            float* red = red_base + (t & 1) * 64;
            if (q == 0) red[wave * 16 + n_in] = ss;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            const float tot = red[n_in] + red[16 + n_in] + red[32 + n_in] + red[48 + n_in];
            const float inv = 1.f / fmaxf(sqrtf(tot), 1e-12f);
#pragma unroll
            for (int w = 0; w < JW; ++w)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[w][r] *= inv;
        }
        // leak, publish my tiles (they are stored to HBM at the top of the next step)
#pragma unroll
        for (int w = 0; w < JW; ++w) {
            const int jt = wave * JW + w;
            f32x4 hn;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                hn[r] = a.act == SGP_ACT_TANH ? leak_tanh_r(h[jt][r], acc[w][r], a.alpha, a.one_minus_alpha)
                                              : leak(h[jt][r], acc[w][r], a.alpha, a.one_minus_alpha);
            hb[jt * 64 + lane] = hn;
            hprev[w] = hn;
        }
        // wave 0: the row of step t + 1 has landed once at most the (PFD - 2) NKX younger requests
        // (+ this step's stores, which only make the wait stricter) are outstanding
        if (wave == 0)
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"((PFD - 2) * NKX < 63 ? (PFD - 2) * NKX : 63) : "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) h[jt] = hb[jt * 64 + lane];
    }
    if (a.T > 0) store_h(a.T - 1, hprev);
    if (a.h_state && wave == 0) {
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            const int j0 = 16 * jt + 4 * q;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (ok && j0 + r < a.R) a.h_state[(long long)node * a.R + j0 + r] = h[jt][r];
        }
    }
}

constexpr long long splitj_lds_bytes(int JT, int NKX) {
    return splitj_fixed_bytes(JT, NKX) + (long long)splitj_ring(JT, NKX) * NKX * 64 * 4;
}
// shapes the split-J kernels are built for, and those whose fp32 fragments exceed the LDS and stream from the workspace
constexpr bool splitj_built(int JT, int NKX) { return JT % 4 == 0 && splitj_lds_bytes(JT, NKX) <= kLdsLimit; }
constexpr bool stream_built(int JT, int NKX) { return packed_floats(JT, NKX) * 4 > kLdsLimit && JT % 4 == 0 && NKX % 4 == 0; }

#include "reservoir_splitj_bf3.h"

template <int JT, int NKX> ResKernel resolve_stream_ool(const ResPart& p);   // reservoir_stream.hip

// The kernel instance of one plan part.  plan_reservoir only asks for what is built (the same conditions select it);
// nullptr = it did not, which the caller reports.
template <int JT, int NKX, int NT>
ResKernel resolve_layer(const ResPart& p) {
    if constexpr (bf3_supported(JT, NKX)) {
        if (p.form == kFormBf3) {
            if constexpr (NT == 2) {
                if (p.pair) return p.h16 ? reservoir_layer_bf3<JT, NKX, NT, true, true> : reservoir_layer_bf3<JT, NKX, NT, true>;
            }
            return p.h16 ? reservoir_layer_bf3<JT, NKX, NT, false, true> : reservoir_layer_bf3<JT, NKX, NT>;
        }
    }
    if (p.form != kFormLayer) return nullptr;
    constexpr bool kLds = packed_floats(JT, NKX) * 4 <= kLdsLimit;
    if (p.xvec && p.ovec) return reservoir_layer<JT, NKX, NT, kLds, true, true>;
    return p.ovec ? reservoir_layer<JT, NKX, NT, kLds, false, true> : reservoir_layer<JT, NKX, NT, kLds, false, false>;
}

template <int JT, int NKX>
ResKernel resolve(const ResPart& p) {
    if constexpr (splitj_built(JT, NKX)) {
        if (p.form == kFormSplitj) return p.ovec ? reservoir_layer_splitj<JT, NKX, true> : reservoir_layer_splitj<JT, NKX, false>;
        if constexpr (sjbf3_supported(JT, NKX) && sjbf3_lds_bytes(JT, NKX) <= kLdsLimit) {
            if (p.form == kFormSplitjBf3) {
                if (p.act_tanh) return p.ovec ? reservoir_layer_splitj_bf3<JT, NKX, true, SGP_ACT_TANH> : reservoir_layer_splitj_bf3<JT, NKX, false, SGP_ACT_TANH>;
                return p.ovec ? reservoir_layer_splitj_bf3<JT, NKX, true, -1> : reservoir_layer_splitj_bf3<JT, NKX, false, -1>;
            }
        }
    }
    if constexpr (stream_built(JT, NKX)) {
        if (p.form == kFormStream || p.form == kFormStream8 || p.form == kFormStreamBf3) return resolve_stream_ool<JT, NKX>(p);
    }
    if constexpr (JT <= 4) {
        if (p.nt == 2) return resolve_layer<JT, NKX, 2>(p);
    }
    return p.nt == 1 ? resolve_layer<JT, NKX, 1>(p) : nullptr;
}

template <int JT>
ResKernel resolve_nkx(const ResPart& p, int nkx) {
    switch (nkx) {
        case 1: return resolve<JT, 1>(p);
        case 2: return resolve<JT, 2>(p);
        case 4: return resolve<JT, 4>(p);
        case 8: return resolve<JT, 8>(p);
        case 16: return resolve<JT, 16>(p);
        case 32: return resolve<JT, 32>(p);
        case 64: return resolve<JT, 64>(p);
    }
    return nullptr;
}


}  // namespace sgp_res
