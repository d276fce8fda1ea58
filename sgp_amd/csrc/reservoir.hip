// C ABI of the reservoir layer + weight packing.  Kernels: reservoir_impl.h, instantiated
// per reservoir width in reservoir_jt*.hip (separate translation units build in parallel).
#include "reservoir_impl.h"

namespace sgp_res {
ResKernel resolve_jt1(const ResPart&, int);
ResKernel resolve_jt2(const ResPart&, int);
ResKernel resolve_jt4(const ResPart&, int);
ResKernel resolve_jt8(const ResPart&, int);
ResKernel resolve_jt16(const ResPart&, int);
}

namespace {
using namespace sgp_res;
__global__ void pack_weights(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                             const float* __restrict__ b, float* __restrict__ out,
                             int F, int R, int JT, int NKX) {
    const long long n_bias = (long long)JT * 16;
    const long long n_wx = (long long)JT * NKX * 64;
    const long long total = packed_floats(JT, NKX);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < n_bias) {
            const int j = (int)i;
            v = j < R ? b[j] : 0.f;
        } else if (i < n_bias + n_wx) {
            const long long o = i - n_bias;
            int l, ks, jt;
            if (NKX % 4 == 0) {                      // [JT][NKX/4][64][4]
                const int s = (int)(o & 3);
                l = (int)((o >> 2) & 63);
                const int k4 = (int)((o >> 8) % (NKX / 4));
                jt = (int)((o >> 8) / (NKX / 4));
                ks = 4 * k4 + s;
            } else {                                 // [JT][NKX][64]
                l = (int)(o & 63);
                ks = (int)((o >> 6) % NKX);
                jt = (int)((o >> 6) / NKX);
            }
            const int j = 16 * jt + (l & 15);
            const int k = (l >> 4) * NKX + ks;
            v = (j < R && k < F) ? w_ih[(long long)j * F + k] : 0.f;
        } else {
            const long long o = i - n_bias - n_wx;
            const int s = (int)(o & 3);
            const int l = (int)((o >> 2) & 63);
            const int kb = (int)((o >> 8) % JT);
            const int jt = (int)((o >> 8) / JT);
            const int j = 16 * jt + (l & 15);
            const int k = 16 * kb + 4 * (l >> 4) + s;
            v = (j < R && k < R) ? w_hh[(long long)j * R + k] : 0.f;
        }
        out[i] = v;
    }
}

// one thread per (jt, kb, lane): 8 weights -> 3 x 16 bytes
__global__ void pack_weights_bf3(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                 const float* __restrict__ b, char* __restrict__ out, int F, int R, int JT, int NKX) {
    const int KBH = bf3_kbh(JT), KB = KBH + bf3_kbx(NKX);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < JT * 16) reinterpret_cast<float*>(out)[i] = i < R ? b[i] : 0.f;
    if (i >= JT * KB * 64) return;
    const int l = i & 63, kb = (i >> 6) % KB, jt = (i >> 6) / KB;
    const int j = 16 * jt + (l & 15), g = l >> 4;
    float w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (kb < KBH) {
            const int tt = 2 * kb + (s >> 2), k = 16 * tt + 4 * g + (s & 3);
            w[s] = (j < R && tt < JT && k < R) ? w_hh[(long long)j * R + k] : 0.f;
        } else {
            const int ks = 8 * (kb - KBH) + s, k = bf3_feature(NKX, g, ks);
            w[s] = (j < R && ks < NKX && k < F) ? w_ih[(long long)j * F + k] : 0.f;
        }
    }
    u32x4 p1, p2, p3;
    bf3_split8(w, p1, p2, p3);
    u32x4* o = reinterpret_cast<u32x4*>(out + (long long)JT * 64) + ((long long)(jt * KB + kb) * 3) * 64 + l;
    o[0] = p1; o[64] = p2; o[128] = p3;
}


// 1 into *bad when any of the n state values lies outside [-1, 1] or is NaN (the word is cleared by the launcher)
__global__ void state_outside_unit_interval(const float* __restrict__ h, long long n, int* __restrict__ bad) {
    int out = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out |= !(fabsf(h[i]) <= 1.f);
    if (__syncthreads_or(out) && threadIdx.x == 0) atomicOr(bad, 1);
}

// Large-N form of the bounded-state loop (reservoir_layer_bf3 with H16): pack_weights_bf3's layout with the recurrent blocks'
// first two piece slots holding fp16 hi / lo of w_hh[j, :] 2^e_j, the input blocks and the bias as bf16 pieces / fp32 of
// the values times 2^(e_j + 14) (the accumulator then carries that factor as a whole), and the way back 2^(-e_j - 14) of
// the JT x 16 rows in `scales` (ResLayout: right behind the fragments).  Exact widths (R = 16 JT, F = 4 NKX).
__global__ void pack_weights_bf3h(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b,
                                  char* __restrict__ out, float* __restrict__ scales, int F, int R, int JT, int NKX) {
    const int KBH = bf3_kbh(JT), KB = KBH + bf3_kbx(NKX);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= JT * KB * 64) return;
    const int l = i & 63, kb = (i >> 6) % KB, jt = (i >> 6) / KB;
    const int j = 16 * jt + (l & 15), g = l >> 4;
    float amax = 0.f;
    for (int k = 0; k < R; ++k) amax = fmaxf(amax, fabsf(w_hh[(long long)j * R + k]));
    int e = 0;
    if (amax > 0.f && amax < __builtin_inff()) {
        int k;
        const float mant = frexpf(amax, &k);
        e = (mant == 0.5f ? 15 : 14) - k;
        e = min(40, max(-40, e));                              // (keeps 2^(e + 14) |w_ih x| far inside fp32)
    }
    const float ws = ldexpf(1.f, e), up = ldexpf(1.f, e + 14);
    if (kb == 0 && g == 0) {
        reinterpret_cast<float*>(out)[j] = b[j] * up;
        scales[j] = ldexpf(1.f, -e - 14);
    }
    float w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (kb < KBH) {
            const int tt = 2 * kb + (s >> 2), k = 16 * tt + 4 * g + (s & 3);
            w[s] = (tt < JT && k < R) ? w_hh[(long long)j * R + k] : 0.f;
        } else {
            const int ks = 8 * (kb - KBH) + s, k = bf3_feature(NKX, g, ks);
            w[s] = (ks < NKX && k < F) ? w_ih[(long long)j * F + k] * up : 0.f;
        }
    }
    u32x4* o = reinterpret_cast<u32x4*>(out + (long long)JT * 64) + ((long long)(jt * KB + kb) * 3) * 64 + l;
    if (kb < KBH) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) sj16_split2(w[2 * d], w[2 * d + 1], ws, hi[d], lo[d]);
        o[0] = u32x4{hi[0], hi[1], hi[2], hi[3]}; o[64] = u32x4{lo[0], lo[1], lo[2], lo[3]}; o[128] = u32x4{0u, 0u, 0u, 0u};
    } else {
        u32x4 p1, p2, p3;
        bf3_split8(w, p1, p2, p3);
        o[0] = p1; o[64] = p2; o[128] = p3;
    }
}

// Two-piece fp16 fragments of W_hh for the split-J kernel's bounded-state loop (reservoir_splitj_bf3.h): one thread per
// (jt, kb, lane), row j scaled by the power of two that puts its largest entry at 2^13 .. 2^14 (computed here: a row is
// at most 128 floats), 2^(-e_j - 14) -- the way back, the state's 2^14 included -- in front of the fragments.
__global__ void pack_weights_sj16(const float* __restrict__ w_hh, char* __restrict__ out, int R, int JT) {
    const int KBH = bf3_kbh(JT);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= JT * KBH * 64) return;
    const int l = i & 63, kb = (i >> 6) % KBH, jt = (i >> 6) / KBH;
    const int j = 16 * jt + (l & 15), g = l >> 4;
    float amax = 0.f;
    if (j < R)
        for (int k = 0; k < R; ++k) amax = fmaxf(amax, fabsf(w_hh[(long long)j * R + k]));
    int e = 0;
    if (amax > 0.f && amax < __builtin_inff()) {
        int k;
        const float mant = frexpf(amax, &k);                   // amax = mant 2^k, mant in [0.5, 1)
        e = (mant == 0.5f ? 15 : 14) - k;                       // floor(log2(16384 / amax))
        e = min(100, max(-100, e));
    }
    const float ws = ldexpf(1.f, e);
    if (kb == 0 && g == 0) reinterpret_cast<float*>(out)[j] = ldexpf(1.f, -e - 14);
    unsigned hi[4], lo[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        float w[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = 2 * d + h, tt = 2 * kb + (s >> 2), k = 16 * tt + 4 * g + (s & 3);
            w[h] = (j < R && tt < JT && k < R) ? w_hh[(long long)j * R + k] : 0.f;
        }
        sj16_split2(w[0], w[1], ws, hi[d], lo[d]);
    }
    u32x4* o = reinterpret_cast<u32x4*>(out + (long long)JT * 64) + ((long long)(jt * KBH + kb) * 2) * 64 + l;
    o[0] = u32x4{hi[0], hi[1], hi[2], hi[3]}; o[64] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

// streamed layout of the wide reservoirs: one thread per (sub-block = 2 k-block + half, tile of the half, lane)
__global__ void pack_weights_sbf3(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                  const float* __restrict__ b, char* __restrict__ out, int F, int R, int JT, int NKX) {
    const int KBH = JT / 2, KBX = NKX / 8, NSB = 2 * (KBH + KBX);     // input k-blocks first
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < JT * 16) reinterpret_cast<float*>(out)[i] = i < R ? b[i] : 0.f;
    if (i >= NSB * 8 * 64) return;
    const int l = i & 63, j8 = (i >> 6) & 7, sb = i >> 9;
    const int kb = sb >> 1, jt = 8 * (sb & 1) + j8;
    const int j = 16 * jt + (l & 15), g = l >> 4;
    float w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (kb >= KBX) {
            const int k = 16 * (2 * (kb - KBX) + (s >> 2)) + 4 * g + (s & 3);
            w[s] = (j < R && k < R) ? w_hh[(long long)j * R + k] : 0.f;
        } else {
            const int k = bf3_feature(NKX, g, 8 * kb + s);
            w[s] = (j < R && k < F) ? w_ih[(long long)j * F + k] : 0.f;
        }
    }
    u32x4 p1, p2, p3;
    bf3_split8(w, p1, p2, p3);
    u32x4* o = reinterpret_cast<u32x4*>(out + 1024) + ((long long)(sb * 8 + j8) * 3) * 64 + l;
    o[0] = p1; o[64] = p2; o[128] = p3;
}

// Wide form of the bounded-state loop (reservoir_layer_stream_bf3 with H16): pack_weights_sbf3's streamed layout with the
// recurrent sub-blocks as [tile][2 fp16 pieces] in the first 16 of their 24 KB, bias and input fragments times 2^(e_j + 14)
// (pack_weights_bf3h), the rows' 2^(-e_j - 14) in `scales`.
__global__ void pack_weights_sbf3h(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b,
                                   char* __restrict__ out, float* __restrict__ scales, int F, int R, int JT, int NKX) {
    const int KBH = JT / 2, KBX = NKX / 8, NSB = 2 * (KBH + KBX);     // input k-blocks first
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    auto row_exp = [&](int j) {
        float amax = 0.f;
        for (int k = 0; k < R; ++k) amax = fmaxf(amax, fabsf(w_hh[(long long)j * R + k]));
        int e = 0;
        if (amax > 0.f && amax < __builtin_inff()) {
            int k;
            const float mant = frexpf(amax, &k);
            e = (mant == 0.5f ? 15 : 14) - k;
            e = min(40, max(-40, e));
        }
        return e;
    };
    if (i < JT * 16) {
        const int e = i < R ? row_exp(i) : 0;
        reinterpret_cast<float*>(out)[i] = i < R ? b[i] * ldexpf(1.f, e + 14) : 0.f;
        scales[i] = ldexpf(1.f, -e - 14);
    }
    if (i >= NSB * 8 * 64) return;
    const int l = i & 63, j8 = (i >> 6) & 7, sb = i >> 9;
    const int kb = sb >> 1, jt = 8 * (sb & 1) + j8;
    const int j = 16 * jt + (l & 15), g = l >> 4;
    const int e = j < R ? row_exp(j) : 0;
    const float ws = ldexpf(1.f, e), up = ldexpf(1.f, e + 14);
    float w[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (kb >= KBX) {
            const int k = 16 * (2 * (kb - KBX) + (s >> 2)) + 4 * g + (s & 3);
            w[s] = (j < R && k < R) ? w_hh[(long long)j * R + k] : 0.f;
        } else {
            const int k = bf3_feature(NKX, g, 8 * kb + s);
            w[s] = (j < R && k < F) ? w_ih[(long long)j * F + k] * up : 0.f;
        }
    }
    char* slot = out + 1024 + (long long)sb * (8 * 3 * 1024);
    if (kb >= KBX) {
        unsigned hi[4], lo[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) sj16_split2(w[2 * d], w[2 * d + 1], ws, hi[d], lo[d]);
        u32x4* o = reinterpret_cast<u32x4*>(slot) + (long long)(j8 * 2) * 64 + l;
        o[0] = u32x4{hi[0], hi[1], hi[2], hi[3]}; o[64] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    } else {
        u32x4 p1, p2, p3;
        bf3_split8(w, p1, p2, p3);
        u32x4* o = reinterpret_cast<u32x4*>(slot) + (long long)(j8 * 3) * 64 + l;
        o[0] = p1; o[64] = p2; o[128] = p3;
    }
}

int pick_nkx(int F) {
    const int need = (F + 3) / 4;
    const int opts[] = {1, 2, 4, 8, 16, 32, 64};
    for (int o : opts) if (o >= need) return o;
    return 0;
}
int pick_jt(int R) {
    const int need = (R + 15) / 16;
    const int opts[] = {1, 2, 4, 8, 16};
    for (int o : opts) if (o >= need) return o;
    return 0;
}

// SGP_TUNE switches of the reservoir dispatch (sgp_amd/tune.py), read once per process
struct ResTune { bool bf3, h16, pair, stream8, tail, beside; int splitj_max; };
const ResTune& res_tune() {
    static const ResTune t = {sgp::tune("res_bf3", 1) != 0, sgp::tune("res_h16", 1) != 0, sgp::tune("res_pair", 1) != 0,
                              sgp::tune("res_stream8", 1) != 0, sgp::tune("res_tail", 1) != 0,
                              sgp::tune("res_tail_beside", 1) != 0, (int)sgp::tune("res_splitj_max", 512)};
    return t;
}

// everything the choice of kernels depends on (x_align / out_align: the pointers' low four bits)
struct ResRequest {
    int F, R, N, T, act; double alpha; bool has_state;
    int n_pieces; bool no_store, has_pred;
    long long xrs, xss, ors, oss; int x_align, out_align;
};

// The ONE kernel selection of sgp_reservoir_f32 / sgp_reservoir_pieces_f32: which parts run on which nodes, with which
// launch shape, and which packs / state test they need.  0, or SGP_EUNSUP with the message set.
int plan_reservoir(const ResRequest& q, ResPlan& p) {
    const ResTune& tn = res_tune();
    const int jt = pick_jt(q.R), nkx = pick_nkx(q.F);
    if (!jt) return sgp::fail(SGP_EUNSUP, "sgp_reservoir_f32: reservoir size %d > 256 not supported", q.R);
    if (!nkx) return sgp::fail(SGP_EUNSUP, "sgp_reservoir_f32: input size %d > 256 not supported", q.F);
    p = ResPlan{};
    p.jt = jt; p.nkx = nkx;
    // padded units and features carry zero weights in the fp32 and split-J forms; the large-N bf16-piece and the
    // streamed forms carry no masks and need the exact widths
    const bool exact = q.R == 16 * jt && q.F == 4 * nkx;
    const bool x16 = q.xrs % 4 == 0 && q.xss % 4 == 0 && q.x_align == 0, o16 = q.ors % 4 == 0 && q.oss % 4 == 0 && q.out_align == 0;
    const bool xv = nkx % 4 == 0 && q.F % 4 == 0 && x16, ov = q.R % 4 == 0 && o16;
    // two fp16 pieces for the recurrent products: the state stays in [-1, 1] only under tanh and a convex leak (a
    // leaking rate outside [0, 1], which the reference accepts, keeps three bf16 pieces)
    const bool h16 = tn.h16 && q.act == SGP_ACT_TANH && q.alpha >= 0.0 && q.alpha <= 1.0;
    const bool pieces = q.n_pieces > 1 || q.no_store || q.has_pred;
    const int n_tiles = (q.N + 15) / 16;
    const bool sj_bf3 = tn.bf3 && sjbf3_supported(jt, nkx) && sjbf3_lds_bytes(jt, nkx) <= kLdsLimit;

    auto add = [&](const ResPart& r) {
        p.part[p.n_parts++] = r;
        p.state_test |= r.pred == kPredStateInside || r.pred == kPredStateOutside;
    };
    // the two-piece fp16 instance -- alone when the recurrence starts from zero, else under the state word == 0 with the
    // three-piece instance under == 1 behind it (no host round trip) -- or the three-piece instance alone
    auto add_bounded = [&](ResPart r, unsigned pack3, unsigned pack16) {
        if (h16) { r.h16 = true; r.pred = q.has_state ? kPredStateInside : kPredNone; add(r); p.packs |= pack16; }
        if (!h16 || q.has_state) { r.h16 = false; r.pred = h16 ? kPredStateOutside : kPredNone; add(r); p.packs |= pack3; }
    };
    // one node tile per workgroup, the j-tiles split over its 4 waves
    auto add_splitj = [&](long long n0, int n, bool side) -> int {
        ResPart r{};
        r.n0 = n0; r.n = n; r.grid = (n + 15) / 16; r.grid_y = 1; r.block = 256; r.ovec = ov; r.side = side;
        if (sj_bf3) {
            r.form = kFormSplitjBf3; r.act_tanh = q.act == SGP_ACT_TANH; r.h16 = h16;     // (h16: chosen per workgroup, on the device)
            r.grid_y = q.n_pieces > 1 ? q.n_pieces : 1;
            r.lds = (int)sjbf3_lds_bytes(jt, nkx);
            r.pred = q.has_pred ? kPredCaller : kPredNone;
            p.packs |= kPackBf3 | (h16 ? kPackSj16 : 0);
        } else if (pieces) {
            return sgp::fail(SGP_EUNSUP, "reservoir: time pieces / predicate need the split-J bf16-piece kernel");
        } else {
            r.form = kFormSplitj; r.lds = (int)splitj_lds_bytes(jt, nkx);
            p.packs |= kPackFp32;
        }
        add(r);
        return 0;
    };
    // a wave owns nt tiles.  Small ranges: one single-tile wave per workgroup (every wave gets its own CU).  Large ones: a
    // wave count that is a multiple of 1024 SIMDs, tiles dealt evenly -- narrow reservoirs (<= 128 VGPRs) as ONE 16-wave
    // workgroup per CU, so that the waves that share a SIMD (w, w+4, w+8, w+12) are consecutive in the tile deal.
    // per > 0, the exact deal: one workgroup per CU, `per` tiles on every SIMD.
    auto add_layer = [&](int nt, long long n0, int n, int per) {
        const int tiles = (n + 15) / 16;
        int wpw = 1, grid = tiles;
        if (per > 0) { wpw = 16; grid = 256; }
        else if (tiles > 1024) { wpw = jt <= 4 ? 16 : 4; grid = 1024 * ((tiles + 1024 * nt - 1) / (1024 * nt)) / wpw; }
        ResPart r{};
        r.nt = nt; r.n0 = n0; r.n = n; r.tiles_per_wave = per; r.grid_y = 1; r.xvec = xv && ov; r.ovec = ov;
        // three-piece bf16 products (reservoir_bf3.h), 3/8 of the matrix time of the exact-fp32 kernel: whole tiles,
        // 16-byte rows, row offsets in 32 bits; the nodes of a ragged last tile go to the exact-fp32 kernel
        const long long n16 = n / 16 * 16;
        if (tn.bf3 && bf3_supported(jt, nkx) && exact && xv && ov && n16 > 0 &&
            n16 * q.xrs * 4 < (1ll << 32) && n16 * q.ors * 4 < (1ll << 32)) {
            if (per <= 0 && n16 / 16 <= 1024) grid = (int)(n16 / 16);
            // as many waves per SIMD as share its tiles evenly (6 tiles: 3 waves of 2; same time as 2 + 2 + 1 + 1 on 4), and
            // with at most three two-tile waves the two tiles share every fragment read
            if (per > 0) wpw = 4 * ((per + nt - 1) / nt);
            r.form = kFormBf3; r.n = (int)n16; r.grid = grid; r.block = 64 * wpw;
            r.pair = nt == 2 && tn.pair && per > 0 && (per + nt - 1) / nt <= 3;
            r.lds = (int)(bf3_packed_bytes(jt, nkx) + jt * 64);               // (+ the row scales of the two-piece fp16 form)
            add_bounded(r, kPackBf3, kPackBf3h);
            if (n16 == n) return;
            r = ResPart{};
            r.nt = 1; r.n0 = n0 + n16; r.n = (int)(n - n16); r.grid_y = 1; r.xvec = r.ovec = true;
            grid = wpw = 1;
        }
        r.form = kFormLayer; r.grid = grid; r.block = 64 * wpw;
        r.lds = packed_floats(jt, nkx) * 4 <= kLdsLimit ? (int)(packed_floats(jt, nkx) * 4) : 0;   // else fragments from the workspace
        p.packs |= kPackFp32;
        add(r);
    };

    // up to 2 workgroups per CU.  (Three per CU -- 513-768 tiles in one round, which the 3-deep ring makes possible at
    // F = R = 64 -- measured slower than one single-tile wave per SIMD: N = 10 000, 1.53 vs 1.37 ms per 512 steps;
    // SGP_TUNE=res_splitj_max=768 selects it.)
    if (splitj_built(jt, nkx) && n_tiles <= tn.splitj_max) return add_splitj(0, q.N, false);
    if (pieces) return sgp::fail(SGP_EUNSUP, "reservoir: time pieces / predicate serve graphs of <= 512 node tiles");
    // Pieces and the caller's predicate end here: the layer, bf16-piece and streamed kernels below know neither, and their
    // parts' predicate is none or the state word, never the caller's.
    if (jt <= 4 && splitj_built(jt, nkx)) {
        // Large N: 1024 SIMDs x `per` tiles exactly, and the < 1024 tiles that are left as a split-J tail: 4 SIMDs share
        // a tile there, a workgroup steps through T in ~0.7 us per step -- a fraction of the per + 1'th tile that the
        // busiest SIMDs would otherwise carry while the others idle (N = 100k: 6250 tiles = 6.1 per SIMD, 7 on the busiest).
        const int per = n_tiles / 1024, left = n_tiles - per * 1024;
        if (tn.tail && per >= 1 && per <= 8 && left <= 512) {
            const int nt = per > 4 ? 2 : 1;
            if (!left) { add_layer(nt, 0, q.N, per); return 0; }
            // the tail is a chain of T short steps on `left` <= 512 workgroups (1.3 ms per 1024 steps whatever their
            // number): it goes onto a side lane and runs beside the main part (its workgroups fit next to the main
            // part's one workgroup per CU: 4 waves and ~50 KB of LDS each)
            const int n0 = per * 1024 * 16;
            if (tn.beside) add_splitj(n0, q.N - n0, true);
            add_layer(nt, 0, n0, per);
            if (!tn.beside) add_splitj(n0, q.N - n0, false);
            return 0;
        }
    }
    if (jt <= 4 && n_tiles > 4096) { add_layer(2, 0, q.N, 0); return 0; }
    if (stream_built(jt, nkx) && n_tiles >= 2048 && exact && x16 && o16) {
        // streamed weights: full rounds of 256 workgroups x 8 tiles; what is left gets one tile per wave if that is
        // enough to hold it, so the last (partial) round costs half a round
        int full = (n_tiles / (256 * 8)) * 256, tail_wgs = 0;
        const int rest = n_tiles - full * 8;
        if (rest > 1024) full += (rest + 7) / 8;
        else tail_wgs = (rest + 3) / 4;
        ResPart r{};
        r.n = q.N; r.tiles_per_wave = full; r.grid = full + tail_wgs; r.grid_y = 1; r.block = 512; r.xvec = r.ovec = true;
        if (tn.bf3 && sbf3_supported(jt, nkx)) {
            r.form = kFormStreamBf3; r.lds = 4 * 8 * 3 * 1024 + 2 * jt * 16 * 4;
            add_bounded(r, kPackSbf3, kPackSbf3h);
        } else {
            // 8 waves x 1 tile (two waves per SIMD) unless SGP_TUNE=res_stream8=0 asks for 4 waves x 2 tiles
            r.form = tn.stream8 ? kFormStream8 : kFormStream; r.block = tn.stream8 ? 512 : 256;
            r.lds = 4 * jt * 1024 + jt * 16 * 4;                     // ring slots + bias
            p.packs |= kPackFp32;
            add(r);
        }
        return 0;
    }
    add_layer(1, 0, q.N, 0);
    return 0;
}

const char* const kPackNames[] = {"pack_weights", "pack_weights_bf3", "pack_weights_sj16", "pack_weights_bf3h",
                                  "pack_weights_sbf3", "pack_weights_sbf3h"};

// kernel name of a part as a trace shows it
void part_name(const ResPlan& p, const ResPart& r, char* out, size_t cap) {
    auto b = [](bool v) { return v ? "true" : "false"; };
    switch (r.form) {
        case kFormLayer:
            snprintf(out, cap, "reservoir_layer<%d, %d, %d, %s, %s, %s>", p.jt, p.nkx, r.nt, b(r.lds > 0), b(r.xvec), b(r.ovec)); break;
        case kFormBf3: snprintf(out, cap, "reservoir_layer_bf3<%d, %d, %d, %s, %s>", p.jt, p.nkx, r.nt, b(r.pair), b(r.h16)); break;
        case kFormSplitj: snprintf(out, cap, "reservoir_layer_splitj<%d, %d, %s>", p.jt, p.nkx, b(r.ovec)); break;
        case kFormSplitjBf3:
            snprintf(out, cap, "reservoir_layer_splitj_bf3<%d, %d, %s, %d>", p.jt, p.nkx, b(r.ovec), r.act_tanh ? SGP_ACT_TANH : -1); break;
        case kFormStream: snprintf(out, cap, "reservoir_layer_stream<%d, %d, true, true>", p.jt, p.nkx); break;
        case kFormStream8: snprintf(out, cap, "reservoir_layer_stream8<%d, %d, true, true>", p.jt, p.nkx); break;
        default: snprintf(out, cap, "reservoir_layer_stream_bf3<%d, %d, %s>", p.jt, p.nkx, b(r.h16)); break;
    }
}

}  // namespace


extern "C" {

int64_t sgp_reservoir_workspace_bytes(int32_t F, int32_t R) {
    const int jt = pick_jt(R), nkx = pick_nkx(F);
    if (!jt || !nkx) return -1;
    return ResLayout(jt, nkx).total;
}

int sgp_reservoir_describe(int32_t F, int32_t R, int32_t N, int32_t T, int32_t act, double alpha, int32_t has_state,
                           int32_t n_pieces, int32_t no_store, int32_t has_pred,
                           int64_t xrs, int64_t xss, int32_t x_align, int64_t ors, int64_t oss, int32_t out_align,
                           char* text, int64_t capacity) {
    SGP_REQUIRE(text && capacity > 0, "sgp_reservoir_describe: no buffer");
    ResPlan p;
    const int rc = plan_reservoir(ResRequest{F, R, N, T, act, alpha, has_state != 0, n_pieces, no_store != 0, has_pred != 0,
                                             xrs, xss, ors, oss, x_align, out_align}, p);
    if (rc) return rc;
    static const char* const preds[] = {"none", "caller", "state_inside", "state_outside"};
    int64_t at = 0;
#define put(...) do { if (at < capacity) at += snprintf(text + at, (size_t)(capacity - at), __VA_ARGS__); } while (0)
    for (int i = 0; i < 6; ++i)
        if (p.packs & (1u << i)) put("{\"kernel\": \"%s\"}\n", kPackNames[i]);
    if (p.state_test) put("{\"kernel\": \"state_outside_unit_interval\"}\n");
    for (int i = 0; i < p.n_parts; ++i) {
        const ResPart& r = p.part[i];
        char name[96];
        part_name(p, r, name, sizeof name);
        put("{\"kernel\": \"%s\", \"nodes\": [%lld, %lld], \"grid\": [%u, %u], \"block\": %u, \"lds\": %d, \"pred\": \"%s\", "
            "\"lane\": \"%s\"}\n", name, r.n0, r.n0 + r.n, r.grid, r.grid_y, r.block, r.lds, preds[r.pred], r.side ? "side" : "main");
    }
#undef put
    SGP_REQUIRE(at < capacity, "sgp_reservoir_describe: buffer of %lld bytes too small", (long long)capacity);
    return 0;
}

struct Pieces { int n, t_last, no_store; long long px, po, ps; const int* pred; int run_if; };

static int reservoir_run(const float* x, int64_t xrs, int64_t xss,
                         const float* w_ih, const float* w_hh, const float* b,
                         double alpha, int32_t act,
                         float* out, int64_t ors, int64_t oss,
                         float* h_state, void* workspace,
                         int32_t T, int32_t N, int32_t F, int32_t R, const Pieces& pc,
                         sgp_stream_t stream);

int sgp_reservoir_f32(const float* x, int64_t xrs, int64_t xss,
                      const float* w_ih, const float* w_hh, const float* b,
                      double alpha, int32_t act,
                      float* out, int64_t ors, int64_t oss,
                      float* h_state, void* workspace,
                      int32_t T, int32_t N, int32_t F, int32_t R,
                      sgp_stream_t stream) {
    return reservoir_run(x, xrs, xss, w_ih, w_hh, b, alpha, act, out, ors, oss, h_state, workspace, T, N, F, R,
                         Pieces{1, T, 0, 0, 0, 0, nullptr, 0}, stream);
}

int sgp_reservoir_pieces_f32(const float* x, int64_t xrs, int64_t xss,
                             const float* w_ih, const float* w_hh, const float* b,
                             double alpha, int32_t act,
                             float* out, int64_t ors, int64_t oss,
                             float* h_state, void* workspace,
                             int32_t t_piece, int32_t t_last, int32_t n_pieces,
                             int64_t x_piece_stride, int64_t out_piece_stride, int32_t no_store,
                             int32_t N, int32_t F, int32_t R,
                             const int32_t* pred, int32_t run_if, sgp_stream_t stream) {
    SGP_REQUIRE(n_pieces >= 1 && t_piece >= 0 && t_last >= 0 && t_last <= t_piece, "sgp_reservoir_pieces_f32: bad piece sizes");
    SGP_REQUIRE(n_pieces == 1 || h_state, "sgp_reservoir_pieces_f32: several pieces need their states [n_pieces][N][R]");
    SGP_REQUIRE(n_pieces <= 65535, "sgp_reservoir_pieces_f32: at most 65535 pieces");
    return reservoir_run(x, xrs, xss, w_ih, w_hh, b, alpha, act, out, ors, oss, h_state, workspace, t_piece, N, F, R,
                         Pieces{n_pieces, n_pieces > 1 ? t_last : t_piece, no_store != 0, x_piece_stride, out_piece_stride,
                                (long long)N * R, pred, run_if}, stream);
}

}  // extern "C"

// validate, plan, pack what the plan names, launch its parts
static int reservoir_run(const float* x, int64_t xrs, int64_t xss,
                         const float* w_ih, const float* w_hh, const float* b,
                         double alpha, int32_t act,
                         float* out, int64_t ors, int64_t oss,
                         float* h_state, void* workspace,
                         int32_t T, int32_t N, int32_t F, int32_t R, const Pieces& pc,
                         sgp_stream_t stream) {
    SGP_REQUIRE(x && w_ih && w_hh && b && out && workspace, "sgp_reservoir_f32: null pointer");
    SGP_REQUIRE(T >= 0 && N >= 0 && F > 0 && R > 0, "sgp_reservoir_f32: bad size");
    SGP_REQUIRE(act >= SGP_ACT_TANH && act <= SGP_ACT_TANH_REL, "sgp_reservoir_f32: unknown activation %d", act);
    SGP_REQUIRE(sgp::aligned16(workspace), "sgp_reservoir_f32: workspace must be 16-byte aligned");
    if (T == 0 || N == 0) return 0;
    ResPlan p;
    int rc = plan_reservoir(ResRequest{F, R, N, T, act, alpha, h_state != nullptr, pc.n, pc.no_store != 0, pc.pred != nullptr,
                                       xrs, xss, ors, oss, (int)((uintptr_t)x & 15u), (int)((uintptr_t)out & 15u)}, p);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int jt = p.jt, nkx = p.nkx;
    const ResLayout L(jt, nkx);
    char* const ws = (char*)workspace;
    auto has = [&](unsigned pack) { return (p.packs & pack) != 0; };

    // one thread per (jt, kb, lane) of the bf16-piece layouts, per (sub-block, tile, lane) of the streamed ones
    const int bf3_blocks = (jt * (bf3_kbh(jt) + bf3_kbx(nkx)) * 64 + 255) / 256, sbf3_blocks = (2 * (jt / 2 + nkx / 8) * 8 * 64 + 255) / 256;
    if (has(kPackFp32)) {
        const long long blocks = (packed_floats(jt, nkx) + 255) / 256;
        hipLaunchKernelGGL(pack_weights, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s, w_ih, w_hh, b, (float*)(ws + L.fp32), F, R, jt, nkx);
    }
    if (has(kPackBf3)) hipLaunchKernelGGL(pack_weights_bf3, dim3(bf3_blocks), dim3(256), 0, s, w_ih, w_hh, b, ws + L.bf3, F, R, jt, nkx);
    if (has(kPackSj16)) hipLaunchKernelGGL(pack_weights_sj16, dim3((jt * bf3_kbh(jt) * 64 + 255) / 256), dim3(256), 0, s, w_hh, ws + L.sj16, R, jt);
    if (has(kPackBf3h))
        hipLaunchKernelGGL(pack_weights_bf3h, dim3(bf3_blocks), dim3(256), 0, s, w_ih, w_hh, b, ws + L.bf3h, (float*)(ws + L.bf3h_scales), F, R, jt, nkx);
    if (has(kPackSbf3)) hipLaunchKernelGGL(pack_weights_sbf3, dim3(sbf3_blocks), dim3(256), 0, s, w_ih, w_hh, b, ws + L.sbf3, F, R, jt, nkx);
    if (has(kPackSbf3h))
        hipLaunchKernelGGL(pack_weights_sbf3h, dim3(sbf3_blocks), dim3(256), 0, s, w_ih, w_hh, b, ws + L.sbf3h, (float*)(ws + L.sbf3h_scales), F, R, jt, nkx);
    rc = sgp::check_launch("pack_weights");
    if (rc) return rc;
    // the device word "some initial state lies outside [-1, 1] (or is NaN)" behind the pack whose instances it selects
    int* const bad = reinterpret_cast<int*>(ws + (has(kPackSbf3h) ? L.sbf3h_state : L.bf3h_state));
    if (p.state_test) {
        hipError_t e = hipMemsetAsync(bad, 0, sizeof(int), s);
        if (e != hipSuccess) return sgp::fail((int)e, "sgp_reservoir_f32: memset: %s", hipGetErrorString(e));
        const long long n = (long long)N * R;
        const long long want = (n + 256 * 16 - 1) / (256 * 16);
        hipLaunchKernelGGL(state_outside_unit_interval, dim3((unsigned)(want < 1024 ? want : 1024)), dim3(256), 0, s, h_state, n, bad);
        rc = sgp::check_launch("state_outside_unit_interval");
        if (rc) return rc;
    }

    ResArgs a;
    a.x = x; a.xrs = xrs; a.xss = xss;
    a.wp = (const float*)(ws + L.fp32);
    a.wp_bf3 = has(kPackBf3) ? ws + L.bf3 : has(kPackSbf3) ? ws + L.sbf3 : nullptr;
    a.wp_h16 = has(kPackSj16) ? ws + L.sj16 : nullptr;       // (the split-J bf16-piece kernel takes its fp16 loop when this is set)
    a.wp_h16l = has(kPackBf3h) ? ws + L.bf3h : nullptr;
    a.wp_h16s = has(kPackSbf3h) ? ws + L.sbf3h : nullptr;
    a.dump = reinterpret_cast<float*>(ws + L.splitj_dump);
    a.bad_state = p.state_test ? bad : nullptr;
    a.n_pieces = pc.n; a.t_last = pc.t_last; a.no_store = pc.no_store; a.px = pc.px; a.po = pc.po; a.ps = pc.ps;
    a.out = out; a.ors = ors; a.oss = oss;
    a.h_state = h_state;
    a.alpha = (float)alpha;                      // scalar operands are rounded to fp32 like
    a.one_minus_alpha = (float)(1.0 - alpha);    // torch does for `(1 - alpha) * h` (reservoir.py:80)
    a.act = act; a.T = T; a.F = F; a.R = R;

    // a part = the same arguments on its node range, under its predicate
    auto launch = [&](const ResPart& r, hipStream_t on) -> int {
        ResKernel kern = nullptr;
        switch (jt) {
            case 1: kern = resolve_jt1(r, nkx); break;
            case 2: kern = resolve_jt2(r, nkx); break;
            case 4: kern = resolve_jt4(r, nkx); break;
            case 8: kern = resolve_jt8(r, nkx); break;
            case 16: kern = resolve_jt16(r, nkx); break;
        }
        if (!kern) return sgp::fail(SGP_EUNSUP, "sgp_reservoir_f32: planned a kernel that is not built");
        ResArgs m = a;
        m.x = x + r.n0 * xrs; m.out = out + r.n0 * ors;
        if (h_state) m.h_state = h_state + r.n0 * R;
        m.N = r.n; m.n_tiles = (r.n + 15) / 16; m.tiles_per_wave = r.tiles_per_wave;
        m.pred = r.pred == kPredNone ? nullptr : r.pred == kPredCaller ? pc.pred : bad;
        m.pred_want = r.pred == kPredCaller ? pc.run_if : r.pred == kPredStateOutside;
        if (r.lds > 0) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, r.lds);
            if (e != hipSuccess) return sgp::fail((int)e, "reservoir: LDS opt-in: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(kern, dim3(r.grid, r.grid_y), dim3(r.block), (size_t)r.lds, on, m);
        return sgp::check_launch("reservoir_layer");
    };
    // a side part runs on the side lane beside the parts after it; without a lane it runs after them
    sgp::SideLane* lane = nullptr;
    const ResPart* deferred = nullptr;
    for (int i = 0; i < p.n_parts && !rc; ++i) {
        const ResPart& r = p.part[i];
        if (r.side) {
            lane = sgp::side_lane();
            if (!lane || !lane->fork(s)) { lane = nullptr; deferred = &r; continue; }
        }
        rc = launch(r, r.side ? lane->stream : s);
    }
    if (deferred && !rc) rc = launch(*deferred, s);
    if (lane && !lane->join(s)) return sgp::fail(SGP_EINVAL, "reservoir: side lane join failed");
    return rc;
}
