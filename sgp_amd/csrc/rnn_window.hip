// Trained recurrent baselines: the gated recurrence of an LSTM / GRU layer over a short window, forward and backward
// through time (reference: tsl/nn/blocks/encoders/rnn.py:41-62 -> torch.nn.LSTM / torch.nn.GRU, batch_first=False, zero
// initial state; selected by `--model-name rnn / fc_rnn` of experiments/run_traffic_baselines.py:28-31).
//
//   LSTM   a = W_ih x_t + b_ih + W_hh h + b_hh,  (i, f, g, o) = (s(a_i), s(a_f), tanh(a_g), s(a_o)),
//          c' = f c + i g,  h' = o tanh(c')
//   GRU    r = s(W_ir x + b_ir + W_hr h + b_hr),  z likewise,  n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
//          h' = (1 - z) n + z h
//
// for M = B * N independent sequences of S = 12 .. 24 steps.  The input part of all S * M rows is one sgp_dense_f32
// launch into the gate buffer [S][M][4 H] (GRU: blocks 0 .. 2); this file is the part that is sequential in time.
//
// Mapping.  A workgroup owns ONE tile of 16 sequences for the whole window; its waves split the H hidden columns
// (CT column tiles of 16 per wave, all gates of a column in the same wave, so the cell update is local to a lane).
// Every product is a v_mfma_f32_16x16x4_f32 with the weight as the A operand (rows = output features) and the state as
// the B operand (columns = sequences): a lane (n = lane & 15, q = lane >> 4) then holds features 16 jt + 4 q + 0..3 of
// sequence n -- 16 contiguous bytes of every [.., M, H] buffer, so gates, h, c and the cotangent move as float4.
// h (backward: the gate gradients) passes between the waves through LDS, one barrier per step (backward: two); h, c,
// dh and dc themselves stay in registers from the first step to the last.
// W_hh (256 KB at H = 128, 1 MB at H = 256) does not fit LDS: it is read every step from a packed copy in fragment
// order (frag.h), resident in L2 because every workgroup reads the same bytes.
// Arithmetic: exact fp32 products, fp32 accumulation, one k-ordered chain per output; no atomics anywhere, so forward
// and backward are bit-identical from run to run and independent of which tile a sequence falls into.
#include "common.h"
#include "decoder_ops.h"
#include "recurrent.h"

namespace {
using namespace sgp;

constexpr int CELL_LSTM = 0, CELL_GRU = 1;

// The packed buffer (frag.h), G H H floats each: W_hh [G H, H] for the forward kernel, then its transpose for the backward one.
struct RnnArgs {
    float* gates;             // [S][M][4 H]: in the input projection, out (save) what backward reads; backward: dgates in place
    const float* wp;          // packed W_hh (this direction's part)
    const float* bhn;         // GRU: b_hn [H]
    float* hseq;              // [S][M][H] (null: not stored)
    float* cseq;              // LSTM, [S][M][H] (null: not stored)
    float* hdrop;             // [S][M][H] dropped copy for the next layer (null: none)
    float* hlast;             // [M][H] (null: not stored)
    const float* dy;          // backward: cotangent of h, [M][H] (last step) or [S][M][H]
    long long M;
    int S, H, save, dy_full;
    unsigned thresh, k0, k1;
    float scale;
};

template <int CELL, int CT>
__global__ __launch_bounds__(256) void rnn_fwd(RnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int G = CELL == CELL_LSTM ? 4 : 3;
    const int H = a.H, JT = H / 16, LDH = H + kPad;
    const SeqTile<CT> my(a.M, JT);
    f32x4 h[CT], cst[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) h[c] = cst[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 bn[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) bn[c] = (CELL == CELL_GRU && a.bhn) ? ld4(a.bhn + my.col(c)) : f32x4{0.f, 0.f, 0.f, 0.f};
    int cur = 0;
    for (int t = 0; t < a.S; ++t) {
        const long long row = (long long)t * a.M + my.mc;
        float* grow = a.gates + row * 4 * H;
        f32x4 acc[CT][G], gxn[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
#pragma unroll
            for (int g = 0; g < G; ++g) acc[c][g] = ld4(grow + g * H + my.col(c));
            if constexpr (CELL == CELL_GRU) { gxn[c] = acc[c][2]; acc[c][2] = bn[c]; }
        }
        if (t > 0) {
            const float* hb = lds + cur * 16 * LDH + my.n * LDH + 4 * my.q;
            for (int kb = 0; kb < JT; ++kb) {
                const f32x4 b = ld4(hb + 16 * kb);
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        acc[c][g] = mfma4(ld4(a.wp + (((long long)(g * JT + my.jt[c]) * JT + kb) * 64 + my.lane) * 4), b, acc[c][g]);
            }
        }
        float* hnext = lds + (cur ^ 1) * 16 * LDH + my.n * LDH;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = my.col(c);
            const bool st = my.ok && my.tv[c];
            if constexpr (CELL == CELL_LSTM) {
                const f32x4 gi = sigmoid4(acc[c][0]), gf = sigmoid4(acc[c][1]), gg = tanh4(acc[c][2]), go = sigmoid4(acc[c][3]);
                cst[c] = gf * cst[c] + gi * gg;
                h[c] = go * tanh4(cst[c]);
                if (a.save && st) {
                    st_gates(grow, H, col, gi, gf, gg, go);
                    st4(a.cseq + row * H + col, cst[c]);
                }
            } else {
                const GruStep gs = gru_step(acc[c][0], acc[c][1], gxn[c], acc[c][2], h[c]);
                h[c] = gs.h;
                if (a.save && st) st_gates(grow, H, col, gs.r, gs.z, gs.n, acc[c][2]);
            }
            if (st) {
                if (a.hseq) st4(a.hseq + row * H + col, h[c]);
                if (a.hdrop) {
                    f32x4 d;
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        d[s] = h[c][s] * keep_factor((unsigned long long)(row * H + col + s), a.thresh, a.k0, a.k1, a.scale);
                    st4(a.hdrop + row * H + col, d);
                }
            }
            if (my.tv[c]) st4(hnext + col, h[c]);
        }
        __syncthreads();                                    // h of this step is complete; the other buffer is free again
        cur ^= 1;
    }
    if (a.hlast && my.ok) {
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (my.tv[c]) st4(a.hlast + my.m * H + my.col(c), h[c]);
    }
}

// Backward through time.  Per step: dh += the step's cotangent; the gate gradients (with respect to the pre-activations)
// from the saved gates; they overwrite the saved gates in place -- LSTM the 4 blocks; GRU [dr, dz, dn, dn r], of which
// the input side reads blocks 0 .. 2 and the hidden side 0, 1, 3 -- and go to LDS, where every wave reads all of them
// for its columns of dh_{t-1} = dgates W_hh (+ dh z for the GRU).
template <int CELL, int CT>
__global__ __launch_bounds__(256) void rnn_bwd(RnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int G = CELL == CELL_LSTM ? 4 : 3;
    const int H = a.H, JT = H / 16, LDG = G * H + kPad, KB = G * JT;
    const SeqTile<CT> my(a.M, JT);
    f32x4 dh[CT], dc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) dh[c] = dc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* dgl = lds + my.n * LDG;
    for (int t = a.S - 1; t >= 0; --t) {
        const long long row = (long long)t * a.M + my.mc;
        float* grow = a.gates + row * 4 * H;
        f32x4 keep[CT];                                     // GRU: dh z, the direct path to dh_{t-1}
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = my.col(c);
            const bool st = my.ok && my.tv[c];
            if (a.dy_full) dh[c] += ld4(a.dy + row * H + col);
            else if (t == a.S - 1) dh[c] += ld4(a.dy + my.mc * H + col);
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            if constexpr (CELL == CELL_LSTM) {
                const f32x4 gi = ld4(grow + col), gf = ld4(grow + H + col), gg = ld4(grow + 2 * H + col), go = ld4(grow + 3 * H + col);
                const f32x4 tc = tanh4(ld4(a.cseq + row * H + col));
                const f32x4 cp = t > 0 ? ld4(a.cseq + (row - a.M) * H + col) : zero;
                const f32x4 dcv = dc[c] + dh[c] * go * (1.f - tc * tc);
                const f32x4 dai = dcv * gg * gi * (1.f - gi), daf = dcv * cp * gf * (1.f - gf);
                const f32x4 dag = dcv * gi * (1.f - gg * gg), dao = dh[c] * tc * go * (1.f - go);
                dc[c] = dcv * gf;
                keep[c] = zero;
                if (st) st_gates(grow, H, col, dai, daf, dag, dao);
                if (my.tv[c]) st_gates(dgl, H, col, dai, daf, dag, dao);
            } else {
                const f32x4 r = ld4(grow + col), z = ld4(grow + H + col), nn = ld4(grow + 2 * H + col), hn = ld4(grow + 3 * H + col);
                const f32x4 hp = t > 0 ? ld4(a.hseq + (row - a.M) * H + col) : zero;
                const GruStepBwd d = gru_step_bwd(dh[c], r, z, nn, hn, hp);
                keep[c] = d.keep;
                if (st) st_gates(grow, H, col, d.dar, d.daz, d.dan, d.dhn);
                if (my.tv[c]) { st4(dgl + col, d.dar); st4(dgl + H + col, d.daz); st4(dgl + 2 * H + col, d.dhn); }   // the hidden side's three
            }
        }
        if (t == 0) break;                                  // uniform: nothing is carried past the first step
        __syncthreads();
        f32x4 acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = keep[c];
        const float* gb = dgl + 4 * my.q;
        for (int kb = 0; kb < KB; ++kb) {
            const f32x4 b = ld4(gb + 16 * kb);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = mfma4(ld4(a.wp + (((long long)my.jt[c] * KB + kb) * 64 + my.lane) * 4), b, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) dh[c] = acc[c];
        __syncthreads();                                    // all reads of this step's gate gradients are done
    }
}

const char* domain_error(int cell, int H) {
    if (cell != CELL_LSTM && cell != CELL_GRU) return "cell must be 0 (lstm) or 1 (gru)";
    if (H < 16 || H > 256 || H % 16) return "hidden size must be a multiple of 16 in 16 .. 256";
    return nullptr;
}
// column tiles per wave: at most 4 waves.  (rnn_impute.hip's ct_of differs on purpose: it has no form with 3.)
int ct_of(int H) { const int jt = H / 16; return jt <= 4 ? 1 : (jt <= 8 ? 2 : (jt <= 12 ? 3 : 4)); }

constexpr int kLdsCap = 16 * (4 * 256 + kPad) * 4;          // the largest this file asks for: the LSTM's backward at H = 256, 64.25 KB

template <int CELL>
int launch(bool bwd, const RnnArgs& a, hipStream_t s) {
    constexpr int G = CELL == CELL_LSTM ? 4 : 3;
    const int JT = a.H / 16, ct = ct_of(a.H), nw = (JT + ct - 1) / ct;
    const dim3 grid((unsigned)((a.M + 15) / 16)), block(64 * nw);
    const size_t shm = bwd ? (size_t)16 * (G * a.H + kPad) * 4 : (size_t)2 * 16 * (a.H + kPad) * 4;
#define SGP_RNN_LAUNCH(CT_)                                                                   \
    if (bwd) {                                                                                \
        if (shm > 48 * 1024)                                                                  \
            if (int rc = raise_lds_limit<rnn_bwd<CELL, CT_>>(kLdsCap, "rnn_bwd")) return rc;  \
        hipLaunchKernelGGL((rnn_bwd<CELL, CT_>), grid, block, shm, s, a);                     \
    } else hipLaunchKernelGGL((rnn_fwd<CELL, CT_>), grid, block, shm, s, a)
    switch (ct) {
        case 1: SGP_RNN_LAUNCH(1); break;
        case 2: SGP_RNN_LAUNCH(2); break;
        case 3: SGP_RNN_LAUNCH(3); break;
        default: SGP_RNN_LAUNCH(4); break;
    }
#undef SGP_RNN_LAUNCH
    return 0;
}

int check_shape(const char* what, int cell, int H, int S, int64_t M) {
    if (const char* e = domain_error(cell, H)) return sgp::fail(SGP_EUNSUP, "%s: %s (cell %d, H %d)", what, e, cell, H);
    SGP_REQUIRE(S >= 1 && M >= 1 && M <= ((int64_t)1 << 31) * 16 - 16, "%s: bad size (S %d, M %lld)", what, S, (long long)M);
    return 0;
}

}  // namespace

extern "C" {

int32_t sgp_rnn_window_supported(int32_t cell, int32_t H) {
    if (const char* e = domain_error(cell, H)) {
        sgp::fail(SGP_EUNSUP, "sgp_rnn_window_supported: %s (cell %d, H %d)", e, cell, H);
        return 0;
    }
    return 1;
}

int64_t sgp_rnn_window_packed_floats(int32_t cell, int32_t H) {
    if (domain_error(cell, H)) return -1;
    return (int64_t)2 * (cell == CELL_LSTM ? 4 : 3) * H * H;
}

int64_t sgp_rnn_window_workspace_bytes(int32_t cell, int32_t H, int32_t S, int64_t M) {
    if (domain_error(cell, H) || S < 1 || M < 1) return -1;
    return (int64_t)S * M * 4 * H * 4;
}

int sgp_rnn_window_pack_f32(const float* w_hh, int32_t cell, int32_t H, float* packed, sgp_stream_t stream) {
    if (const char* e = domain_error(cell, H)) return sgp::fail(SGP_EUNSUP, "sgp_rnn_window_pack_f32: %s (cell %d, H %d)", e, cell, H);
    SGP_REQUIRE(w_hh && packed, "sgp_rnn_window_pack_f32: null pointer");
    SGP_REQUIRE(sgp::aligned16(packed), "sgp_rnn_window_pack_f32: packed must be 16-byte aligned");
    const int G = cell == CELL_LSTM ? 4 : 3;
    frag_pack_to(packed, w_hh, H, G * H, H, 0, (hipStream_t)stream);
    frag_pack_to(packed, w_hh, H, G * H, H, 1, (hipStream_t)stream);
    return sgp::check_launch("sgp_rnn_window_pack_f32");
}

int sgp_rnn_window_fwd_f32(int32_t cell, int32_t H, int32_t S, int64_t M, float* gates, const float* packed,
                           const float* b_hn, float* h_seq, float* c_seq, float* h_drop, double dropout_p, uint64_t seed,
                           float* h_last, int32_t save, sgp_stream_t stream) {
    int rc = check_shape("sgp_rnn_window_fwd_f32", cell, H, S, M);
    if (rc) return rc;
    SGP_REQUIRE(gates && packed, "sgp_rnn_window_fwd_f32: null pointer");
    SGP_REQUIRE(cell != CELL_GRU || b_hn, "sgp_rnn_window_fwd_f32: the GRU needs b_hn");
    SGP_REQUIRE(h_seq || h_last, "sgp_rnn_window_fwd_f32: nothing to store (h_seq and h_last are null)");
    SGP_REQUIRE(!save || (h_seq && (cell != CELL_LSTM || c_seq)), "sgp_rnn_window_fwd_f32: save needs h_seq (and c_seq for the LSTM)");
    SGP_REQUIRE(!h_drop || (dropout_p > 0. && dropout_p <= 1.), "sgp_rnn_window_fwd_f32: h_drop needs 0 < dropout_p <= 1");
    SGP_REQUIRE(sgp::aligned16(gates) && sgp::aligned16(packed) && sgp::aligned16(b_hn) && sgp::aligned16(h_seq) &&
                sgp::aligned16(c_seq) && sgp::aligned16(h_drop) && sgp::aligned16(h_last),
                "sgp_rnn_window_fwd_f32: buffers must be 16-byte aligned");
    RnnArgs a{};
    a.gates = gates; a.wp = packed; a.bhn = b_hn; a.hseq = h_seq; a.cseq = c_seq; a.hdrop = h_drop; a.hlast = h_last;
    a.M = M; a.S = S; a.H = H; a.save = save;
    set_dropout(a.thresh, a.k0, a.k1, a.scale, h_drop ? dropout_p : 0., seed);
    if (h_drop && dropout_p >= 1.) { a.thresh = 0xFFFFFFFFu; a.scale = 0.f; }
    rc = cell == CELL_LSTM ? launch<CELL_LSTM>(false, a, (hipStream_t)stream) : launch<CELL_GRU>(false, a, (hipStream_t)stream);
    return rc ? rc : sgp::check_launch("sgp_rnn_window_fwd_f32");
}

int sgp_rnn_window_bwd_f32(int32_t cell, int32_t H, int32_t S, int64_t M, float* gates, const float* packed,
                           const float* h_seq, const float* c_seq, const float* dy, int32_t dy_full,
                           sgp_stream_t stream) {
    int rc = check_shape("sgp_rnn_window_bwd_f32", cell, H, S, M);
    if (rc) return rc;
    SGP_REQUIRE(gates && packed && dy, "sgp_rnn_window_bwd_f32: null pointer");
    SGP_REQUIRE(cell == CELL_LSTM ? c_seq != nullptr : h_seq != nullptr,
                "sgp_rnn_window_bwd_f32: the saved sequence is missing (c_seq for the LSTM, h_seq for the GRU)");
    SGP_REQUIRE(sgp::aligned16(gates) && sgp::aligned16(packed) && sgp::aligned16(h_seq) && sgp::aligned16(c_seq) &&
                sgp::aligned16(dy), "sgp_rnn_window_bwd_f32: buffers must be 16-byte aligned");
    const int G = cell == CELL_LSTM ? 4 : 3;
    RnnArgs a{};
    a.gates = gates; a.wp = packed + (int64_t)G * H * H; a.hseq = const_cast<float*>(h_seq);
    a.cseq = const_cast<float*>(c_seq); a.dy = dy; a.dy_full = dy_full;
    a.M = M; a.S = S; a.H = H;
    rc = cell == CELL_LSTM ? launch<CELL_LSTM>(true, a, (hipStream_t)stream) : launch<CELL_GRU>(true, a, (hipStream_t)stream);
    return rc ? rc : sgp::check_launch("sgp_rnn_window_bwd_f32");
}

}  // extern "C"
