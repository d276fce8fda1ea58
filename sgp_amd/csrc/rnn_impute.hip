// RNN imputers: the fill-in recurrence of RNNImputerModel (reference: tsl/nn/models/imputation/rnni_models.py:74-96), a
// GRU one-step-ahead predictor whose input at step s is its own prediction wherever the value is missing,
//
//   h_0 given,  p_s = W_r h_s + b_r,  xp_s = m_s ? x_s : p_s,  h_{s+1} = GRUCell([xp_s | u_s | m_s], h_s),  s = 0 .. S-2
//
// for M independent sequences of S steps with D fed-back columns, forward and backward through time.  The input of a
// step depends on the state of the same step, so the input projection cannot leave the time loop as it does in
// rnn_window.hip; but the dependence is a low-rank term.  With W_x the first D columns of W_ih,
//
//   W_ih in_s = [W_x (m_s . x_s) + W_u u_s + W_m m_s + b]  +  W_x ((1 - m_s) . p_s):
//
// the bracket is one sgp_dense_f32 launch for all S M rows into the gate buffer, and this file adds the second term
// inside the loop: per step ceil(D / 16) row tiles of W_r over H (h is in LDS for the recurrent product anyway), the
// select by the mask, and ceil(D / 16) further k-blocks of W_x per gate tile.
//
// Mapping (rnn_window.hip's): a workgroup owns ONE tile of 16 sequences for the whole window; its waves split the H
// hidden columns (CT column tiles of 16 per wave, all gates of a column in one wave) and deal the D tiles round robin.
// Every product is a v_mfma_f32_16x16x4_f32 with the weight as the A operand (rows = output features) and the state
// as the B operand (columns = sequences).  h passes between the waves through a double buffer in LDS, the masked
// prediction (backward: the gate gradients and dp) through a second LDS array; two barriers per step forward, three
// backward.  h and dh stay in registers from the first step to the last.  Weights are read every step from packed
// copies in fragment order (frag.h), zero padded to whole D tiles, resident in L2.
// LDS, floats: forward 2 * 16 (H + 4) + 16 (16 DT + 4), at most 66 KB; backward 16 (4 H + 4) + 16 (16 DT + 4), at most
// 97 KB (H = 256, D = 512) of the CU's 160 KB.
// Arithmetic: exact fp32 products, fp32 accumulation, one k-ordered chain per output (W_hh blocks, then the feedback
// blocks); no atomics, so both passes are bit-identical from run to run and independent of the tile and lane a
// sequence falls into.  `reverse` walks the window from its last step to its first, reading and writing rows at
// S-1-t: the backward model of BiRNNImputerModel needs no flipped copies.
#include "common.h"
#include "recurrent.h"

namespace {
using namespace sgp;

struct Sizes {                                              // floats of the packed parts of one direction
    long long whh, wx, wr;
    long long dir() const { return whh + wx + wr; }
};
Sizes sizes_of(int H, int D) {
    const long long DP = 16ll * ((D + 15) / 16);
    return Sizes{3ll * H * H, 3ll * H * DP, DP * H};
}

struct ImpArgs {
    float* gates;             // [S][M][4 H]: in the bracket, out (save) r, z, n, W_hn h + b_hn; backward: dgates in place
    const float *whh, *wx, *wr;   // packed, this direction's parts
    const float *bhn, *br;    // b_hn [H], b_r [D]
    const float* h0;          // [M][H] (null: zeros)
    const float* msk;         // 0 / 1 floats, rows in the window's own (b, s, n) order, D columns
    float* xp;                // merged input, same rows (save: written at the missing entries of steps 0 .. S-2)
    float* p;                 // predictions, same rows, [.., D] contiguous; backward: gx
    float* hseq;              // [S][M][H]
    const float* dP;          // backward: cotangent of p, rows as p
    const float* dH;          // backward: cotangent of h_seq [S][M][H] (null: none)
    float* dp;                // backward: the total dp [S][M][D]
    long long M, inner, ldm, ldx;
    int S, H, D, save, reverse, detach;
};

// row of (step tt, sequence m) in the window's own order: [b][S][inner] with m = b * inner + i
__device__ __forceinline__ long long src_row0(long long m, long long inner, int S) { return (m / inner) * S * inner + m % inner; }

template <int CT>
__global__ __launch_bounds__(256) void impute_fwd(ImpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, JT = H / 16, LDH = H + kPad, D = a.D, DT = (D + 15) / 16, LDD = 16 * DT + kPad;
    float* pbuf = lds + 2 * 16 * LDH;
    const SeqTile<CT> my(a.M, JT);
    const int nw = blockDim.x >> 6;
    const long long xr0 = src_row0(my.mc, a.inner, a.S);
    f32x4 h[CT], bn[CT];
    {
        const long long row = (long long)(a.reverse ? a.S - 1 : 0) * a.M + my.mc;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = my.col(c);
            h[c] = a.h0 ? ld4(a.h0 + my.mc * H + col) : f32x4{0.f, 0.f, 0.f, 0.f};
            bn[c] = ld4(a.bhn + col);
            if (my.tv[c]) st4(lds + my.n * LDH + col, h[c]);
            if (my.ok && my.tv[c]) st4(a.hseq + row * H + col, h[c]);
        }
    }
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < a.S; ++t) {
        const int tt = a.reverse ? a.S - 1 - t : t;
        const long long xrow = xr0 + (long long)tt * a.inner;
        const float* hb = lds + cur * 16 * LDH + my.n * LDH + 4 * my.q;
        // p_t = W_r h_t + b_r, stored; what is fed back goes to LDS with zeros at the observed entries
        for (int dt = my.wave; dt < DT; dt += nw) {
            const f32x4 acc = tile_prod(a.wr, dt, JT, hb, bias4(a.br, 16 * dt + 4 * my.q, D), my.lane);
            f32x4 pm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int d = 16 * dt + 4 * my.q + s;
                if (d < D) {
                    const bool seen = a.msk[xrow * a.ldm + d] != 0.f;
                    pm[s] = seen ? 0.f : acc[s];
                    if (my.ok) {
                        a.p[xrow * D + d] = acc[s];
                        if (a.save && !seen && t < a.S - 1) a.xp[xrow * a.ldx + d] = acc[s];
                    }
                }
            }
            st4(pbuf + my.n * LDD + 16 * dt + 4 * my.q, pm);
        }
        if (t == a.S - 1) break;                            // uniform: the last step's value is never an input
        __syncthreads();
        const long long row = (long long)tt * a.M + my.mc;
        float* grow = a.gates + row * 4 * H;
        f32x4 acc[CT][2], gxn[CT], hn[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = my.col(c);
            acc[c][0] = ld4(grow + col); acc[c][1] = ld4(grow + H + col); gxn[c] = ld4(grow + 2 * H + col);
            hn[c] = bn[c];
        }
        for (int kb = 0; kb < JT; ++kb) {
            const f32x4 b = ld4(hb + 16 * kb);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
#pragma unroll
                for (int g = 0; g < 2; ++g)
                    acc[c][g] = mfma4(ld4(a.whh + (((long long)(g * JT + my.jt[c]) * JT + kb) * 64 + my.lane) * 4), b, acc[c][g]);
                hn[c] = mfma4(ld4(a.whh + (((long long)(2 * JT + my.jt[c]) * JT + kb) * 64 + my.lane) * 4), b, hn[c]);
            }
        }
        const float* pb = pbuf + my.n * LDD + 4 * my.q;
        for (int kb = 0; kb < DT; ++kb) {
            const f32x4 b = ld4(pb + 16 * kb);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
#pragma unroll
                for (int g = 0; g < 2; ++g)
                    acc[c][g] = mfma4(ld4(a.wx + (((long long)(g * JT + my.jt[c]) * DT + kb) * 64 + my.lane) * 4), b, acc[c][g]);
                gxn[c] = mfma4(ld4(a.wx + (((long long)(2 * JT + my.jt[c]) * DT + kb) * 64 + my.lane) * 4), b, gxn[c]);
            }
        }
        float* hnext = lds + (cur ^ 1) * 16 * LDH + my.n * LDH;
        const long long nrow = (long long)(a.reverse ? tt - 1 : tt + 1) * a.M + my.mc;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = my.col(c);
            const bool st = my.ok && my.tv[c];
            const GruStep gs = gru_step(acc[c][0], acc[c][1], gxn[c], hn[c], h[c]);
            h[c] = gs.h;
            if (a.save && st) st_gates(grow, H, col, gs.r, gs.z, gs.n, hn[c]);
            if (st) st4(a.hseq + nrow * H + col, h[c]);
            if (my.tv[c]) st4(hnext + col, h[c]);
        }
        __syncthreads();                                    // h_{t+1} is complete; the other buffer and pbuf are free again
        cur ^= 1;
    }
}

// Backward through time.  Step t undoes h_t -> h_{t+1}: the gate gradients from dh_{t+1} and the saved gates overwrite
// the saved gates in place, [dr, dz, dn, dn r] (input side blocks 0 .. 2, hidden side 0, 1, 3), and go to LDS;
// dxp_t = W_x^T [dr, dz, dn];  gx_t = m_t . dxp_t;  dp_t = dP_t + (1 - m_t) . dxp_t (detach: dP_t alone), stored and to
// LDS;  dh_t = dh_{t+1} z + W_hh^T [dr, dz, dn r] + W_r^T dp_t + dH_t.  The last step has no transition: its gate row
// is zeroed (so the weight gradients over all S M rows need no slicing and S = 1 gives exact zeros) and gx is zero.
template <int CT>
__global__ __launch_bounds__(256) void impute_bwd(ImpArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, JT = H / 16, LDG = 4 * H + kPad, D = a.D, DT = (D + 15) / 16, LDD = 16 * DT + kPad;
    float* dpbuf = lds + 16 * LDG;
    const SeqTile<CT> my(a.M, JT);
    const int nw = blockDim.x >> 6;
    const long long xr0 = src_row0(my.mc, a.inner, a.S);
    f32x4 dh[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) dh[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* dgl = lds + my.n * LDG;
    for (int t = a.S - 1; t >= 0; --t) {
        const int tt = a.reverse ? a.S - 1 - t : t;
        const bool last = t == a.S - 1;                     // uniform
        const long long row = (long long)tt * a.M + my.mc, xrow = xr0 + (long long)tt * a.inner;
        float* grow = a.gates + row * 4 * H;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        f32x4 keep[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = my.col(c);
            const bool st = my.ok && my.tv[c];
            if (last) {
                keep[c] = zero;
                if (st) st_gates(grow, H, col, zero, zero, zero, zero);
            } else {
                const f32x4 r = ld4(grow + col), z = ld4(grow + H + col), nn = ld4(grow + 2 * H + col), hn = ld4(grow + 3 * H + col);
                const GruStepBwd d = gru_step_bwd(dh[c], r, z, nn, hn, ld4(a.hseq + row * H + col));
                keep[c] = d.keep;
                if (st) st_gates(grow, H, col, d.dar, d.daz, d.dan, d.dhn);
                if (my.tv[c]) st_gates(dgl, H, col, d.dar, d.daz, d.dan, d.dhn);
            }
        }
        if (!last) __syncthreads();
        for (int dt = my.wave; dt < DT; dt += nw) {
            f32x4 acc = zero;
            if (!last) acc = tile_prod(a.wx, dt, 3 * JT, dgl + 4 * my.q, acc, my.lane);
            f32x4 dpl = zero;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int d = 16 * dt + 4 * my.q + s;
                if (d < D) {
                    const bool seen = a.msk[xrow * a.ldm + d] != 0.f;
                    const float back = (seen || a.detach) ? 0.f : acc[s];
                    dpl[s] = a.dP[xrow * D + d] + back;
                    if (my.ok) {
                        a.dp[row * D + d] = dpl[s];
                        if (a.p) a.p[xrow * D + d] = seen ? acc[s] : 0.f;
                    }
                }
            }
            st4(dpbuf + my.n * LDD + 16 * dt + 4 * my.q, dpl);
        }
        if (t == 0) break;                                  // uniform: nothing is carried past the first step
        __syncthreads();
        f32x4 acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = keep[c];
        if (!last)
            for (int kb = 0; kb < 3 * JT; ++kb) {
                const f32x4 b = ld4(dgl + 4 * my.q + 16 * kb + (kb >= 2 * JT ? H : 0));
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[c] = mfma4(ld4(a.whh + (((long long)my.jt[c] * 3 * JT + kb) * 64 + my.lane) * 4), b, acc[c]);
            }
        for (int kb = 0; kb < DT; ++kb) {
            const f32x4 b = ld4(dpbuf + my.n * LDD + 4 * my.q + 16 * kb);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = mfma4(ld4(a.wr + (((long long)my.jt[c] * DT + kb) * 64 + my.lane) * 4), b, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            if (a.dH) acc[c] += ld4(a.dH + row * H + my.col(c));
            dh[c] = acc[c];
        }
        __syncthreads();                                    // all reads of this step's gate gradients and dp are done
    }
}

const char* domain_error(int H, int D) {
    if (H < 16 || H > 256 || H % 16) return "hidden size must be a multiple of 16 in 16 .. 256";
    if (D < 1 || D > 512) return "the fed-back width must be in 1 .. 512";
    return nullptr;
}
// column tiles per wave: at most 4 waves.  Unlike rnn_window.hip's ct_of, on purpose: the form with 3 is not
// instantiated (4 accumulator sets per tile here)
int ct_of(int H) { const int jt = H / 16; return jt <= 4 ? 1 : (jt <= 8 ? 2 : 4); }
size_t lds_bytes(bool bwd, int H, int D) {
    const size_t dd = (size_t)16 * (16 * ((D + 15) / 16) + kPad);
    return ((bwd ? (size_t)16 * (4 * H + kPad) : (size_t)2 * 16 * (H + kPad)) + dd) * 4;
}

template <int CT>
int launch_ct(bool bwd, const ImpArgs& a, dim3 grid, dim3 block, size_t shm, hipStream_t s) {
    const int cap = (int)lds_bytes(true, 256, 512);                    // the largest this file asks for
    if (bwd) {
        if (shm > 48 * 1024)
            if (int rc = raise_lds_limit<impute_bwd<CT>>(cap, "rnn_impute")) return rc;
        hipLaunchKernelGGL((impute_bwd<CT>), grid, block, shm, s, a);
    } else {
        if (shm > 48 * 1024)
            if (int rc = raise_lds_limit<impute_fwd<CT>>(cap, "rnn_impute")) return rc;
        hipLaunchKernelGGL((impute_fwd<CT>), grid, block, shm, s, a);
    }
    return 0;
}

int launch(bool bwd, const ImpArgs& a, hipStream_t s) {
    const int JT = a.H / 16, ct = ct_of(a.H), nw = (JT + ct - 1) / ct;
    const dim3 grid((unsigned)((a.M + 15) / 16)), block(64 * nw);
    const size_t shm = lds_bytes(bwd, a.H, a.D);
    switch (ct) {
        case 1: return launch_ct<1>(bwd, a, grid, block, shm, s);
        case 2: return launch_ct<2>(bwd, a, grid, block, shm, s);
        default: return launch_ct<4>(bwd, a, grid, block, shm, s);
    }
}

int check_shape(const char* what, int H, int D, int S, int64_t M, int64_t inner) {
    if (const char* e = domain_error(H, D)) return sgp::fail(SGP_EUNSUP, "%s: %s (H %d, D %d)", what, e, H, D);
    SGP_REQUIRE(S >= 1 && M >= 1 && M <= ((int64_t)1 << 31) * 16 - 16, "%s: bad size (S %d, M %lld)", what, S, (long long)M);
    SGP_REQUIRE(inner >= 1 && M % inner == 0, "%s: M %lld is no multiple of the inner row count %lld", what, (long long)M, (long long)inner);
    return 0;
}

}  // namespace

extern "C" {

int32_t sgp_rnn_impute_supported(int32_t H, int32_t D) {
    if (const char* e = domain_error(H, D)) {
        sgp::fail(SGP_EUNSUP, "sgp_rnn_impute_supported: %s (H %d, D %d)", e, H, D);
        return 0;
    }
    return 1;
}

int64_t sgp_rnn_impute_packed_floats(int32_t H, int32_t D) {
    if (domain_error(H, D)) return -1;
    return 2 * sizes_of(H, D).dir();
}

int64_t sgp_rnn_impute_workspace_bytes(int32_t H, int32_t D, int32_t S, int64_t M) {
    if (domain_error(H, D) || S < 1 || M < 1) return -1;
    return (int64_t)S * M * 4 * H * 4;
}

int sgp_rnn_impute_plan(int32_t H, int32_t D, int64_t M, int32_t* plan) {
    if (const char* e = domain_error(H, D)) return sgp::fail(SGP_EUNSUP, "sgp_rnn_impute_plan: %s (H %d, D %d)", e, H, D);
    SGP_REQUIRE(plan && M >= 1, "sgp_rnn_impute_plan: null pointer or bad size (M %lld)", (long long)M);
    const int JT = H / 16, ct = ct_of(H);
    plan[0] = ct;
    plan[1] = (JT + ct - 1) / ct;
    plan[2] = (D + 15) / 16;
    plan[3] = (int32_t)((M + 15) / 16 > 0x7fffffff ? 0x7fffffff : (M + 15) / 16);
    plan[4] = (int32_t)lds_bytes(false, H, D);
    plan[5] = (int32_t)lds_bytes(true, H, D);
    return 0;
}

int sgp_rnn_impute_pack_f32(const float* w_ih, int64_t w_ih_row_stride, const float* w_hh, const float* w_r, int32_t H,
                            int32_t D, float* packed, sgp_stream_t stream) {
    if (const char* e = domain_error(H, D)) return sgp::fail(SGP_EUNSUP, "sgp_rnn_impute_pack_f32: %s (H %d, D %d)", e, H, D);
    SGP_REQUIRE(w_ih && w_hh && w_r && packed, "sgp_rnn_impute_pack_f32: null pointer");
    SGP_REQUIRE(w_ih_row_stride >= D, "sgp_rnn_impute_pack_f32: weight_ih rows of %lld floats hold no %d columns", (long long)w_ih_row_stride, D);
    SGP_REQUIRE(sgp::aligned16(packed), "sgp_rnn_impute_pack_f32: packed must be 16-byte aligned");
    for (int trans = 0; trans < 2; ++trans) {                           // forward: W_hh, W_x, W_r; backward: their transposes
        frag_pack_to(packed, w_hh, H, 3 * H, H, trans, (hipStream_t)stream);
        frag_pack_to(packed, w_ih, w_ih_row_stride, 3 * H, D, trans, (hipStream_t)stream);
        frag_pack_to(packed, w_r, H, D, H, trans, (hipStream_t)stream);
    }
    return sgp::check_launch("sgp_rnn_impute_pack_f32");
}

int sgp_rnn_impute_fwd_f32(int32_t H, int32_t D, int32_t S, int64_t M, int64_t inner, int32_t reverse, float* gates,
                           const float* packed, const float* b_hn, const float* b_r, const float* h0, const float* mask,
                           int64_t mask_row_stride, float* xp, int64_t xp_row_stride, float* p, float* h_seq,
                           int32_t save, sgp_stream_t stream) {
    int rc = check_shape("sgp_rnn_impute_fwd_f32", H, D, S, M, inner);
    if (rc) return rc;
    SGP_REQUIRE(gates && packed && b_hn && b_r && mask && p && h_seq, "sgp_rnn_impute_fwd_f32: null pointer");
    SGP_REQUIRE(!save || xp, "sgp_rnn_impute_fwd_f32: save needs the merged-input buffer");
    SGP_REQUIRE(mask_row_stride >= D && (!xp || xp_row_stride >= D), "sgp_rnn_impute_fwd_f32: a row stride is below D");
    SGP_REQUIRE(sgp::aligned16(gates) && sgp::aligned16(packed) && sgp::aligned16(b_hn) && sgp::aligned16(h0) &&
                sgp::aligned16(h_seq), "sgp_rnn_impute_fwd_f32: gates, packed, b_hn, h0 and h_seq must be 16-byte aligned");
    const Sizes z = sizes_of(H, D);
    ImpArgs a{};
    a.gates = gates; a.whh = packed; a.wx = packed + z.whh; a.wr = packed + z.whh + z.wx;
    a.bhn = b_hn; a.br = b_r; a.h0 = h0; a.msk = mask; a.ldm = mask_row_stride; a.xp = xp; a.ldx = xp_row_stride;
    a.p = p; a.hseq = h_seq; a.M = M; a.inner = inner; a.S = S; a.H = H; a.D = D; a.save = save; a.reverse = reverse != 0;
    rc = launch(false, a, (hipStream_t)stream);
    return rc ? rc : sgp::check_launch("sgp_rnn_impute_fwd_f32");
}

int sgp_rnn_impute_bwd_f32(int32_t H, int32_t D, int32_t S, int64_t M, int64_t inner, int32_t reverse, int32_t detach,
                           float* gates, const float* packed, const float* h_seq, const float* mask,
                           int64_t mask_row_stride, const float* dP, const float* dH, float* dp, float* gx,
                           sgp_stream_t stream) {
    int rc = check_shape("sgp_rnn_impute_bwd_f32", H, D, S, M, inner);
    if (rc) return rc;
    SGP_REQUIRE(gates && packed && h_seq && mask && dP && dp, "sgp_rnn_impute_bwd_f32: null pointer");
    SGP_REQUIRE(mask_row_stride >= D, "sgp_rnn_impute_bwd_f32: the mask's row stride is below D");
    SGP_REQUIRE(sgp::aligned16(gates) && sgp::aligned16(packed) && sgp::aligned16(h_seq) && sgp::aligned16(dH),
                "sgp_rnn_impute_bwd_f32: gates, packed, h_seq and dH must be 16-byte aligned");
    const Sizes z = sizes_of(H, D);
    const float* b = packed + z.dir();
    ImpArgs a{};
    a.gates = gates; a.whh = b; a.wx = b + z.whh; a.wr = b + z.whh + z.wx;
    a.hseq = const_cast<float*>(h_seq); a.msk = mask; a.ldm = mask_row_stride; a.dP = dP; a.dH = dH; a.dp = dp; a.p = gx;
    a.M = M; a.inner = inner; a.S = S; a.H = H; a.D = D; a.reverse = reverse != 0; a.detach = detach != 0;
    rc = launch(true, a, (hipStream_t)stream);
    return rc ? rc : sgp::check_launch("sgp_rnn_impute_bwd_f32");
}

}  // extern "C"
