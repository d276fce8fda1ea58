// Multi-head scaled dot-product attention, forward and backward (include/sgp_amd.h, "Attention"):
//   O = softmax(Q K^T / sqrt(d) + causal mask) V   per (sequence, head), L tokens of d channels.
// Exact fp32: every product is a v_mfma_f32_16x16x4_f32, softmax statistics in fp32 with the row maximum subtracted.
//
// One WAVE owns one 16-token tile of one (sequence, head) and walks the other axis in tiles of 16 with the online
// softmax; there is no LDS and no barrier (a workgroup is four independent waves), so the length of a sequence is not
// bounded by anything on the chip, and what a wave computes depends on its own sequence only: alone or in a batch, the
// bits are the same, and every sum runs in tile order.
//
// MFMA operands (lane = 16 q + c; A lane supplies A[c][q], B lane supplies B[q][c], D lane holds D[4 q + r][c]):
//   scores   D[a, b] = sum_k X[a][k] Y[b][k]: lane (q, c) reads 16 bytes of row c of X and of row c of Y at column
//            16 kb + 4 q; the four values are the operands of four MFMAs (the contraction order inside a 16-block is
//            permuted to 4 q + s on both sides, which a sum does not see).
//   products D[ch, b] += sum_a Z[a][ch] W[a][b] with W the score tile a lane already holds: register r of lane (q, c) is
//            W[4 q + r][c], exactly the B operand of MFMA step r; the A operand is Z[4 q + r][16 dt + c], one dword.
// So the forward keeps S^T (lane = one query, 4 of 16 keys), P never leaves the registers, and O^T accumulates with
// the query on the lane: the running maximum, the rescale and the final division are per-lane scalars.  The backward
// runs twice over the score tiles: once with the query on the lane (dQ, and delta = rowsum(dO * O) into the
// workspace), once with the key on the lane (dK, dV); each output tile has one owner, nothing is added atomically.
#include "common.h"
#include "device_math.h"

using sgp::f32x4;

namespace {

constexpr int kWaves = 4;                 // waves (work items) per workgroup
constexpr long long kMaxItems = 0x7fffffffll;

struct Geo {
    long long inner, outer_rows, inner_rows, tok_rows;   // token t of sequence s: row (s / inner) outer_rows + (s % inner) inner_rows + t tok_rows
    long long n_seq, items;
    int L, d, heads, causal, q_first, qtiles, ktiles, dtiles;
    float scale;
};

struct FwdArgs {
    Geo g;
    const float* Q; const float* K; const float* V; float* O; float* lse;
    long long q_rs, k_rs, v_rs, o_rs;
};

struct BwdArgs {
    Geo g;
    const float* dO; const float* Q; const float* K; const float* V; const float* O; const float* lse;
    float* dQ; float* dK; float* dV; float* delta;
    long long do_rs, q_rs, k_rs, v_rs, o_rs, dq_rs, dk_rs, dv_rs;
};

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 frag(const float* row, bool ok, int col, int d) {
    return (ok && col < d) ? sgp::ld4(row + col) : f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ float elem(const float* row, bool ok, int col, int d) { return (ok && col < d) ? row[col] : 0.f; }
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {       // the four lanes of a column end with the same bits
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// D[a = 4 q + r][b = c] = sum_k X[a][k] Y[b][k]: lane (q, c) reads row c of X (xrow, valid when xok), yf are its
// fragments of row c of Y
template <int DT>
__device__ __forceinline__ f32x4 dot_tile(const float* xrow, bool xok, const f32x4 (&yf)[DT], int dtiles, int q, int d) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < DT; ++kb) {
        if (kb < dtiles) {
            const f32x4 xf = frag(xrow, xok, 16 * kb + 4 * q, d);
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = mfma(xf[s], yf[kb][s], acc);
        }
    }
    return acc;
}

// work item -> (sequence, head, tile) and the first row of the sequence
struct Item { long long seq, row0, stat; int h, tile; bool live; };
__device__ __forceinline__ Item item_of(const Geo& g, int tiles) {
    Item it;
    const long long id = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
    it.live = id < g.items;
    it.tile = (int)(id % tiles);
    const long long sh = id / tiles;
    it.h = (int)(sh % g.heads);
    it.seq = sh / g.heads;
    it.row0 = (it.seq / g.inner) * g.outer_rows + (it.seq % g.inner) * g.inner_rows;
    it.stat = (it.seq * g.heads + it.h) * (long long)g.L;     // its row of lse / delta
    return it;
}

template <int DT>
__global__ __launch_bounds__(64 * kWaves) void attn_fwd(FwdArgs a) {
    const Geo& g = a.g;
    const Item it = item_of(g, g.qtiles);
    if (!it.live) return;                                           // whole waves; no barrier anywhere
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int i0 = g.q_first + 16 * it.tile, i = i0 + c;
    const bool iok = i < g.L;
    const int hc = it.h * g.d;
    const float* qrow = a.Q + (it.row0 + (long long)(iok ? i : 0) * g.tok_rows) * a.q_rs + hc;
    f32x4 qf[DT], acc[DT];
#pragma unroll
    for (int kb = 0; kb < DT; ++kb) {
        qf[kb] = frag(qrow, iok && kb < g.dtiles, 16 * kb + 4 * q, g.d);
        acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, l = 0.f;
    const int jend = g.causal ? min(g.L, i0 + 16) : g.L;
    for (int j0 = 0; j0 < jend; j0 += 16) {
        const int jc = j0 + c;
        const bool kok = jc < g.L;
        const float* krow = a.K + (it.row0 + (long long)(kok ? jc : 0) * g.tok_rows) * a.k_rs + hc;
        const f32x4 st = dot_tile<DT>(krow, kok, qf, g.dtiles, q, g.d);       // S^T[key 4 q + r][query c]
        float sv[4], p[4];
        bool vis[4];
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * q + r;
            vis[r] = j < g.L && (!g.causal || j <= i);
            sv[r] = vis[r] ? st[r] * g.scale : -INFINITY;
            mt = fmaxf(mt, sv[r]);
        }
        mt = quad_max(mt);
        const float mn = fmaxf(m, mt);                              // finite from the first tile on: key 0 is visible
        const float alpha = sgp::exp_f32(m - mn);
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = vis[r] ? sgp::exp_f32(sv[r] - mn) : 0.f;
            ps += p[r];
        }
        ps = quad_sum(ps);
        l = l * alpha + ps;
        m = mn;
        const float* vrow[4];
        bool vok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * q + r;
            vok[r] = j < g.L;
            vrow[r] = a.V + (it.row0 + (long long)(vok[r] ? j : 0) * g.tok_rows) * a.v_rs + hc;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            if (dt < g.dtiles) {
                acc[dt] *= alpha;
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[dt] = mfma(elem(vrow[r], vok[r], 16 * dt + c, g.d), p[r], acc[dt]);
            }
        }
    }
    if (!iok) return;
    float* orow = a.O + (it.row0 + (long long)i * g.tok_rows) * a.o_rs + hc;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = 16 * dt + 4 * q;
        if (dt < g.dtiles && col < g.d) sgp::st4(orow + col, acc[dt] / l);
    }
    if (a.lse && q == 0) a.lse[it.stat + i] = m + sgp::log_f32(l);
}

// dQ of a query tile, rows below q_first zeroed by the wave of tile 0, delta = rowsum(dO * O) into the workspace
template <int DT>
__global__ __launch_bounds__(64 * kWaves) void attn_bwd_dq(BwdArgs a) {
    const Geo& g = a.g;
    const Item it = item_of(g, g.qtiles);
    if (!it.live) return;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int hc = it.h * g.d;
    if (it.tile == 0) {
        const int quads = g.d / 4;
        for (long long e = lane; e < (long long)g.q_first * quads; e += 64) {
            const long long t = e / quads;
            sgp::st4(a.dQ + (it.row0 + t * g.tok_rows) * a.dq_rs + hc + 4 * (int)(e % quads), f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
    const int i0 = g.q_first + 16 * it.tile, i = i0 + c;
    const bool iok = i < g.L;
    const long long irow = it.row0 + (long long)(iok ? i : 0) * g.tok_rows;
    const float* qrow = a.Q + irow * a.q_rs + hc;
    const float* dorow = a.dO + irow * a.do_rs + hc;
    const float* orow = a.O + irow * a.o_rs + hc;
    f32x4 qf[DT], dof[DT], acc[DT];
    float dsum = 0.f;
#pragma unroll
    for (int kb = 0; kb < DT; ++kb) {
        const bool ok = iok && kb < g.dtiles;
        qf[kb] = frag(qrow, ok, 16 * kb + 4 * q, g.d);
        dof[kb] = frag(dorow, ok, 16 * kb + 4 * q, g.d);
        const f32x4 of = frag(orow, ok, 16 * kb + 4 * q, g.d);
#pragma unroll
        for (int s = 0; s < 4; ++s) dsum = fmaf(dof[kb][s], of[s], dsum);
        acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float delta = quad_sum(dsum);
    const float lse = iok ? a.lse[it.stat + i] : 0.f;
    if (iok && q == 0) a.delta[it.stat + i] = delta;
    const int jend = g.causal ? min(g.L, i0 + 16) : g.L;
    for (int j0 = 0; j0 < jend; j0 += 16) {
        const int jc = j0 + c;
        const bool kok = jc < g.L;
        const long long jrow = it.row0 + (long long)(kok ? jc : 0) * g.tok_rows;
        const f32x4 st = dot_tile<DT>(a.K + jrow * a.k_rs + hc, kok, qf, g.dtiles, q, g.d);
        const f32x4 dpt = dot_tile<DT>(a.V + jrow * a.v_rs + hc, kok, dof, g.dtiles, q, g.d);
        float ds[4];
        const float* krow[4];
        bool ok4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + 4 * q + r;
            ok4[r] = j < g.L;
            const bool vis = ok4[r] && (!g.causal || j <= i);
            const float p = vis ? sgp::exp_f32(fmaf(st[r], g.scale, -lse)) : 0.f;
            ds[r] = p * (dpt[r] - delta);
            krow[r] = a.K + (it.row0 + (long long)(ok4[r] ? j : 0) * g.tok_rows) * a.k_rs + hc;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            if (dt < g.dtiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[dt] = mfma(elem(krow[r], ok4[r], 16 * dt + c, g.d), ds[r], acc[dt]);
            }
        }
    }
    if (!iok) return;
    float* dqrow = a.dQ + irow * a.dq_rs + hc;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = 16 * dt + 4 * q;
        if (dt < g.dtiles && col < g.d) sgp::st4(dqrow + col, acc[dt] * g.scale);
    }
}

// dK and dV of a key tile: the query tiles in order, the key on the lane
template <int DT>
__global__ __launch_bounds__(64 * kWaves) void attn_bwd_dkv(BwdArgs a) {
    const Geo& g = a.g;
    const Item it = item_of(g, g.ktiles);
    if (!it.live) return;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const int hc = it.h * g.d;
    const int j0 = 16 * it.tile, j = j0 + c;
    const bool jok = j < g.L;
    const long long jrow = it.row0 + (long long)(jok ? j : 0) * g.tok_rows;
    f32x4 kf[DT], vf[DT], dk[DT], dv[DT];
#pragma unroll
    for (int kb = 0; kb < DT; ++kb) {
        const bool ok = jok && kb < g.dtiles;
        kf[kb] = frag(a.K + jrow * a.k_rs + hc, ok, 16 * kb + 4 * q, g.d);
        vf[kb] = frag(a.V + jrow * a.v_rs + hc, ok, 16 * kb + 4 * q, g.d);
        dk[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        dv[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int qt = 0; qt < g.qtiles; ++qt) {
        const int i0 = g.q_first + 16 * qt;
        if (g.causal && i0 + 15 < j0) continue;                     // every key of the tile lies after every query
        const int ic = i0 + c;
        const bool icok = ic < g.L;
        const long long crow = it.row0 + (long long)(icok ? ic : 0) * g.tok_rows;
        const f32x4 st = dot_tile<DT>(a.Q + crow * a.q_rs + hc, icok, kf, g.dtiles, q, g.d);     // S[query 4 q + r][key c]
        const f32x4 dpt = dot_tile<DT>(a.dO + crow * a.do_rs + hc, icok, vf, g.dtiles, q, g.d);
        float p[4], ds[4];
        const float* qrow[4];
        const float* dorow[4];
        bool ok4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = i0 + 4 * q + r;
            ok4[r] = i < g.L;
            const bool vis = ok4[r] && jok && (!g.causal || j <= i);
            const float lse = ok4[r] ? a.lse[it.stat + i] : 0.f;
            const float delta = ok4[r] ? a.delta[it.stat + i] : 0.f;
            p[r] = vis ? sgp::exp_f32(fmaf(st[r], g.scale, -lse)) : 0.f;
            ds[r] = p[r] * (dpt[r] - delta);
            const long long row = it.row0 + (long long)(ok4[r] ? i : 0) * g.tok_rows;
            qrow[r] = a.Q + row * a.q_rs + hc;
            dorow[r] = a.dO + row * a.do_rs + hc;
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            if (dt < g.dtiles) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dv[dt] = mfma(elem(dorow[r], ok4[r], 16 * dt + c, g.d), p[r], dv[dt]);
                    dk[dt] = mfma(elem(qrow[r], ok4[r], 16 * dt + c, g.d), ds[r], dk[dt]);
                }
            }
        }
    }
    if (!jok) return;
    float* dkrow = a.dK + jrow * a.dk_rs + hc;
    float* dvrow = a.dV + jrow * a.dv_rs + hc;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
        const int col = 16 * dt + 4 * q;
        if (dt < g.dtiles && col < g.d) {
            sgp::st4(dkrow + col, dk[dt] * g.scale);
            sgp::st4(dvrow + col, dv[dt]);
        }
    }
}

// ---- host
const char* domain_error(int32_t L, int32_t d, int32_t heads, int64_t n_seq, int32_t causal, int32_t q_first) {
    if (d < 8 || d > 128 || d % 8) return "the head width d must be a multiple of 8 in 8 .. 128";
    if (heads < 1 || (int64_t)heads * d > 256) return "heads * d must lie in 8 .. 256";
    if (L < 1 || L > 0x7fffffff - 32) return "the sequence length L must be at least 1";
    if (n_seq < 1) return "n_seq must be at least 1";
    if (causal != 0 && causal != 1) return "causal must be 0 or 1";
    if (q_first < 0 || q_first >= L) return "q_first must lie in 0 .. L - 1";
    const long long tiles = ((long long)L + 15) / 16;               // the key tiles: at least as many as the query tiles
    if (n_seq > kMaxItems / heads / tiles) return "n_seq * heads * ceil(L / 16) must stay below 2^31";
    return nullptr;
}

int form_of(int d) { return d <= 16 ? 1 : (d <= 32 ? 2 : (d <= 64 ? 4 : 8)); }

Geo make_geo(int32_t L, int32_t d, int32_t heads, int64_t n_seq, int64_t inner, int64_t outer_rows, int64_t inner_rows,
             int64_t tok_rows, int32_t causal, int32_t q_first) {
    Geo g;
    g.inner = inner; g.outer_rows = outer_rows; g.inner_rows = inner_rows; g.tok_rows = tok_rows;
    g.n_seq = n_seq; g.L = L; g.d = d; g.heads = heads; g.causal = causal; g.q_first = q_first;
    g.qtiles = (L - q_first + 15) / 16; g.ktiles = (L + 15) / 16; g.dtiles = (d + 15) / 16;
    g.items = 0;
    g.scale = (float)(1.0 / sqrt((double)d));
    return g;
}

bool vec_ok(const void* p, int64_t rs) { return p && sgp::aligned16(p) && rs % 4 == 0; }

template <typename Args, typename K1, typename K2, typename K4, typename K8>
void launch(int form, long long items, hipStream_t s, const Args& a, K1 k1, K2 k2, K4 k4, K8 k8) {
    const dim3 grid((unsigned)((items + kWaves - 1) / kWaves)), block(64 * kWaves);
    if (form == 1) hipLaunchKernelGGL(k1, grid, block, 0, s, a);
    else if (form == 2) hipLaunchKernelGGL(k2, grid, block, 0, s, a);
    else if (form == 4) hipLaunchKernelGGL(k4, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k8, grid, block, 0, s, a);
}

}  // namespace

extern "C" {

int sgp_attention_plan(int32_t L, int32_t d, int32_t heads, int64_t n_seq, int32_t causal, int32_t q_first, int32_t* plan) {
    if (const char* e = domain_error(L, d, heads, n_seq, causal, q_first))
        return sgp::fail(SGP_EUNSUP, "sgp_attention_plan: %s (L %d, d %d, heads %d, n_seq %lld, causal %d, q_first %d)", e, L,
                         d, heads, (long long)n_seq, causal, q_first);
    SGP_REQUIRE(plan, "sgp_attention_plan: null pointer");
    const Geo g = make_geo(L, d, heads, n_seq, 1, 0, 0, 0, causal, q_first);
    plan[0] = form_of(d);
    plan[1] = g.dtiles;
    plan[2] = g.qtiles;
    plan[3] = g.ktiles;
    plan[4] = kWaves;
    plan[5] = (int32_t)((n_seq * heads * g.qtiles + kWaves - 1) / kWaves);
    plan[6] = (int32_t)((n_seq * heads * g.ktiles + kWaves - 1) / kWaves);
    plan[7] = 0;
    return 0;
}

int64_t sgp_attention_workspace_bytes(int32_t L, int32_t heads, int64_t n_seq) {
    if (L < 1 || heads < 1 || n_seq < 1) return -1;
    return n_seq * heads * (int64_t)L * (int64_t)sizeof(float);
}

int sgp_attention_fwd_f32(const float* Q, int64_t q_row_stride, const float* K, int64_t k_row_stride,
                          const float* V, int64_t v_row_stride, float* O, int64_t o_row_stride, float* lse,
                          int32_t L, int32_t d, int32_t heads, int64_t n_seq,
                          int64_t inner, int64_t outer_rows, int64_t inner_rows, int64_t tok_rows,
                          int32_t causal, int32_t q_first, sgp_stream_t stream) {
    if (const char* e = domain_error(L, d, heads, n_seq, causal, q_first))
        return sgp::fail(SGP_EUNSUP, "sgp_attention_fwd_f32: %s (L %d, d %d, heads %d, n_seq %lld, causal %d, q_first %d)", e,
                         L, d, heads, (long long)n_seq, causal, q_first);
    SGP_REQUIRE(vec_ok(Q, q_row_stride) && vec_ok(K, k_row_stride) && vec_ok(V, v_row_stride) && vec_ok(O, o_row_stride),
                "sgp_attention_fwd_f32: Q, K, V and O must be non-null, 16-byte aligned, with row strides in whole float4s");
    SGP_REQUIRE(inner >= 1 && outer_rows >= 0 && inner_rows >= 0 && tok_rows >= 0, "sgp_attention_fwd_f32: bad token map");
    const int64_t E = (int64_t)heads * d;
    SGP_REQUIRE(q_row_stride >= E && k_row_stride >= E && v_row_stride >= E && o_row_stride >= E,
                "sgp_attention_fwd_f32: a row stride below heads * d");
    FwdArgs a;
    a.g = make_geo(L, d, heads, n_seq, inner, outer_rows, inner_rows, tok_rows, causal, q_first);
    a.g.items = n_seq * heads * a.g.qtiles;
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.lse = lse;
    a.q_rs = q_row_stride; a.k_rs = k_row_stride; a.v_rs = v_row_stride; a.o_rs = o_row_stride;
    launch(form_of(d), a.g.items, (hipStream_t)stream, a, attn_fwd<1>, attn_fwd<2>, attn_fwd<4>, attn_fwd<8>);
    return sgp::check_launch("attn_fwd");
}

int sgp_attention_bwd_f32(const float* dO, int64_t do_row_stride, const float* Q, int64_t q_row_stride,
                          const float* K, int64_t k_row_stride, const float* V, int64_t v_row_stride,
                          const float* O, int64_t o_row_stride, const float* lse,
                          float* dQ, int64_t dq_row_stride, float* dK, int64_t dk_row_stride,
                          float* dV, int64_t dv_row_stride, void* work, int64_t work_bytes,
                          int32_t L, int32_t d, int32_t heads, int64_t n_seq,
                          int64_t inner, int64_t outer_rows, int64_t inner_rows, int64_t tok_rows,
                          int32_t causal, int32_t q_first, sgp_stream_t stream) {
    if (const char* e = domain_error(L, d, heads, n_seq, causal, q_first))
        return sgp::fail(SGP_EUNSUP, "sgp_attention_bwd_f32: %s (L %d, d %d, heads %d, n_seq %lld, causal %d, q_first %d)", e,
                         L, d, heads, (long long)n_seq, causal, q_first);
    SGP_REQUIRE(vec_ok(dO, do_row_stride) && vec_ok(Q, q_row_stride) && vec_ok(K, k_row_stride) && vec_ok(V, v_row_stride) &&
                vec_ok(O, o_row_stride) && vec_ok(dQ, dq_row_stride) && vec_ok(dK, dk_row_stride) && vec_ok(dV, dv_row_stride),
                "sgp_attention_bwd_f32: the operands must be non-null, 16-byte aligned, with row strides in whole float4s");
    SGP_REQUIRE(lse && work, "sgp_attention_bwd_f32: null pointer");
    SGP_REQUIRE(work_bytes >= sgp_attention_workspace_bytes(L, heads, n_seq), "sgp_attention_bwd_f32: workspace too small");
    SGP_REQUIRE(inner >= 1 && outer_rows >= 0 && inner_rows >= 0 && tok_rows >= 0, "sgp_attention_bwd_f32: bad token map");
    const int64_t E = (int64_t)heads * d;
    SGP_REQUIRE(do_row_stride >= E && q_row_stride >= E && k_row_stride >= E && v_row_stride >= E && o_row_stride >= E &&
                dq_row_stride >= E && dk_row_stride >= E && dv_row_stride >= E,
                "sgp_attention_bwd_f32: a row stride below heads * d");
    BwdArgs a;
    a.g = make_geo(L, d, heads, n_seq, inner, outer_rows, inner_rows, tok_rows, causal, q_first);
    a.dO = dO; a.Q = Q; a.K = K; a.V = V; a.O = O; a.lse = lse;
    a.dQ = dQ; a.dK = dK; a.dV = dV; a.delta = static_cast<float*>(work);
    a.do_rs = do_row_stride; a.q_rs = q_row_stride; a.k_rs = k_row_stride; a.v_rs = v_row_stride; a.o_rs = o_row_stride;
    a.dq_rs = dq_row_stride; a.dk_rs = dk_row_stride; a.dv_rs = dv_row_stride;
    hipStream_t s = (hipStream_t)stream;
    a.g.items = n_seq * heads * a.g.qtiles;                         // first: it writes the delta the second pass reads
    launch(form_of(d), a.g.items, s, a, attn_bwd_dq<1>, attn_bwd_dq<2>, attn_bwd_dq<4>, attn_bwd_dq<8>);
    if (int rc = sgp::check_launch("attn_bwd_dq")) return rc;
    a.g.items = n_seq * heads * a.g.ktiles;
    launch(form_of(d), a.g.items, s, a, attn_bwd_dkv<1>, attn_bwd_dkv<2>, attn_bwd_dkv<4>, attn_bwd_dkv<8>);
    return sgp::check_launch("attn_bwd_dkv");
}

}  // extern "C"
