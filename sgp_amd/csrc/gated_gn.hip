// The gated graph network layer's per-edge MLP (tsl/nn/layers/graph_convs/gated_gn.py:53-64), forward and backward,
// without any per-edge tensor in the forward pass.  With W1 = [Wa | Wb] split by the caller into the node
// projection PQ = [X Wa^T + b1 | X Wb^T] (sgp_dense_f32), an edge (j -> i) is
//     z1 = P[i] + Q[j],  a1 = act(z1),  z2 = W2 a1 + b2,  m = act(z2),  g = sigmoid(wg . m + bg),  agg[i] += g m.
//
// Work unit: a CHUNK = up to 256 incoming edges of ONE target (edges sorted by target; a target with more edges is
// split into several chunks, a target without edges is one empty chunk so that its row is written).  One wave walks
// its chunk in tiles of 16 edges: lane (q, e) = (lane >> 4, lane & 15) gathers the 16-byte pieces [16 kb + 4 q, + 4)
// of P[i] and Q[src[e]] -- the B operand of v_mfma_f32_16x16x4_f32 in the fragment order of decoder_mlp.hip, whose
// packed weights (sgp_dense_pack_f32) are the A operand -- and gets z2[o = 16 ot + 4 q + r] of ITS edge in register r
// of tile ot.  The gate's dot product is a 2-step cross-lane sum over q; the gated messages are added into per-lane
// accumulators over the tiles and summed over the 16 edge lanes once per chunk, all in a fixed order.  Chunks of a
// split target write partial rows that a second kernel adds in chunk order (fp64).
//
// Backward: the same walk recomputes z1, a1, z2, m, g; dz2 comes out in exactly the lane layout the B operand of
// da1 = W2^T dz2 needs, and da1 in the layout of z1, so nothing moves between lanes.  dz1 is stored once per edge in
// a bounded workspace (batch items in slices) and summed per SOURCE through the inverted index (edges stably sorted
// by source) for dQ; dP is the per-target sum.  dW2 = sum_e dz2[e] a1[e]^T has the edges as contraction index: the 4
// waves of a workgroup put their tiles (64 edges) in LDS and wave w accumulates the output-row tiles ot = w, w + 4, ..
// Workgroups take work items in a fixed strided order and write one partial each, added in workgroup order in fp64:
// no float atomics anywhere, results are bit-identical from run to run.
#include "common.h"
#include "decoder_ops.h"
#include "wg.h"

using sgp::f32x4;
using sgp::sigmoid_f32;

namespace {

constexpr int GG_CHUNK = 256;          // edges per chunk (sgp_gated_gn_chunk_edges)
constexpr int GG_WAVES = 4;
constexpr long long GG_PART_BYTES = 32ll << 20;    // weight-gradient partials: at most this many bytes
constexpr int GG_MAX_WG = 1024;

struct GgArgs {
    const float* pq; long long pq_rs;
    const float* dagg; long long dagg_rs;
    int n, H, Hm, HTa, KTa, act;
    const int* chunks; int n_chunks;                // (target, e0, e1, partial row or -1) per chunk
    const int* src; long long n_edges;
    int n_parts;
    const float* w2p; const float* w2tp;            // packed W2 [H, Hm] and W2^T [Hm, H]
    const float* b2; const float* wg; const float* bg;
    float* out; long long out_rs;                   // forward: agg; backward: dPQ
    float* part;                                    // partial rows of split targets: [batch item][n_parts][width]
    float* ws;                                      // backward: dz1 per (batch item of the slice, edge) [Hm]
    float* wpart; int accum;                        // backward: per-workgroup weight-gradient partials
    int b0, nb;                                     // batch items [b0, b0 + nb) of this launch
    bool vec, ovec, dvec;                           // 16-byte accesses of PQ / out / dAgg rows are legal
};

__device__ __forceinline__ f32x4 load_piece(const float* row, int col, int width, bool vec) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (col < width) {
        if (vec) v = *reinterpret_cast<const f32x4*>(row + col);
        else {
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (col + s < width) v[s] = row[col + s];
        }
    }
    return v;
}

__device__ __forceinline__ void store_piece(float* row, int col, int width, bool vec, f32x4 v) {
    if (col >= width) return;
    if (vec) *reinterpret_cast<f32x4*>(row + col) = v;
    else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (col + s < width) row[col + s] = v[s];
    }
}

__device__ __forceinline__ f32x4 sum16(f32x4 v) {            // over the 16 edge lanes, fixed tree
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += __shfl_xor(v[r], off);
    return v;
}

// z2 (before the bias) of one tile: zt[ot] += W2 tile . a1
template <int HT, int KT>
__device__ __forceinline__ void product(const float* __restrict__ wp, int nt, int nk, int lane,
                                        const f32x4 (&bop)[KT], f32x4 (&acc)[HT]) {
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) {
        acc[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ot >= nt) continue;                                      // wave-uniform
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) {
            if (kb >= nk) continue;
            const f32x4 wf = *reinterpret_cast<const f32x4*>(wp + (((long long)ot * nk + kb) * 64 + lane) * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc[ot] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], bop[kb][s], acc[ot], 0, 0, 0);
        }
    }
}

template <int HT, int KT>
__global__ __launch_bounds__(64 * GG_WAVES) void edge_fwd(GgArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e16 = lane & 15, q = lane >> 4;
    const int c = blockIdx.x * GG_WAVES + wave;
    if (c >= a.n_chunks) return;
    const int bi = a.b0 + blockIdx.y;
    const int tgt = a.chunks[4 * c], e0 = a.chunks[4 * c + 1], e1 = a.chunks[4 * c + 2], prow = a.chunks[4 * c + 3];
    const long long rb = (long long)bi * a.n;
    const float* prow_p = a.pq + (rb + tgt) * a.pq_rs;
    f32x4 p[KT], oacc[HT];
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) p[kb] = load_piece(prow_p, 16 * kb + 4 * q, a.Hm, a.vec);
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) oacc[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float bg = a.bg[0];
    for (int t = e0; t < e1; t += 16) {
        const int e = t + e16;
        const bool valid = e < e1;
        const int j = valid ? a.src[e] : tgt;
        const float* qrow = a.pq + (rb + j) * a.pq_rs + a.Hm;
        f32x4 a1[KT], z[HT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) {
            const f32x4 qv = load_piece(qrow, 16 * kb + 4 * q, a.Hm, a.vec);
#pragma unroll
            for (int s = 0; s < 4; ++s) a1[kb][s] = valid ? activate(p[kb][s] + qv[s], a.act) : 0.f;
        }
        product<HT, KT>(a.w2p, a.HTa, a.KTa, lane, a1, z);
        float dot = 0.f;
#pragma unroll
        for (int ot = 0; ot < HT; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * ot + 4 * q + r;
                const bool in = o < a.H;
                const float m = in ? activate(z[ot][r] + a.b2[o], a.act) : 0.f;
                dot += in ? a.wg[o] * m : 0.f;
                z[ot][r] = m;
            }
        dot += __shfl_xor(dot, 16);
        dot += __shfl_xor(dot, 32);
        const float g = valid ? sigmoid_f32(dot + bg) : 0.f;
#pragma unroll
        for (int ot = 0; ot < HT; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[ot][r] += g * z[ot][r];
    }
    float* orow = prow < 0 ? a.out + (rb + tgt) * a.out_rs
                           : a.part + ((long long)bi * a.n_parts + prow) * a.H;
    const bool ovec = a.H % 4 == 0 && (prow >= 0 || a.ovec);
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) {
        if (ot >= a.HTa) continue;
        const f32x4 v = sum16(oacc[ot]);
        if (e16 == 0) store_piece(orow, 16 * ot + 4 * q, a.H, ovec, v);
    }
}

// rows of split targets: out[b, target] = partial rows p0 .. p0 + cnt - 1 added in chunk order (fp64)
__global__ void fix_rows(const float* __restrict__ part, const int* __restrict__ fix, int n_fix, int n_parts, int width,
                         int n, int b0, int nb, float* __restrict__ out, long long out_rs) {
    const long long total = (long long)nb * n_fix * width;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const int col = (int)(t % width);
        const long long r = t / width;
        const int f = (int)(r % n_fix), bi = b0 + (int)(r / n_fix);
        const int tgt = fix[3 * f], p0 = fix[3 * f + 1], cnt = fix[3 * f + 2];
        double s = 0.0;
        for (int k = 0; k < cnt; ++k) s += (double)part[((long long)bi * n_parts + p0 + k) * width + col];
        out[((long long)bi * n + tgt) * out_rs + col] = (float)s;
    }
}

__device__ __forceinline__ void act_both(float z, int act, float& m, float& d) {
    if (act == 1) { m = fmaxf(z, 0.f); d = z > 0.f ? 1.f : 0.f; }
    else if (act == 2) { const float sg = sigmoid_f32(z); m = z * sg; d = sg * (1.f + z * (1.f - sg)); }
    else { m = z; d = 1.f; }
}

template <int HT, int KT>
__global__ __launch_bounds__(64 * GG_WAVES) void edge_bwd(GgArgs a) {
    constexpr int SH = 16 * HT + 16;                                 // LDS row strides: 16 mod 32 words, so that the
    constexpr int SK = (16 * KT) % 32 == 16 ? 16 * KT : 16 * KT + 16;   // rows q and q + 1 of a read fall on disjoint banks
    constexpr int OQ = HT >= 4 ? HT / 4 : 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* dzl = lds;                                                // [64 edges][SH]
    float* a1l = lds + 64 * SH;                                      // [64 edges][SK]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e16 = lane & 15, q = lane >> 4;
    const int n_groups = (a.n_chunks + GG_WAVES - 1) / GG_WAVES;
    const long long items = (long long)n_groups * a.nb;
    const float bg = a.bg[0];
    f32x4 wacc[OQ][KT], db2[HT], dwg[HT];
    float dbg = 0.f;
#pragma unroll
    for (int j = 0; j < OQ; ++j)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) wacc[j][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) db2[ot] = dwg[ot] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int grp = (int)(it % n_groups), bl = (int)(it / n_groups);
        const int bi = a.b0 + bl;
        const long long rb = (long long)bi * a.n;
        int rounds = 0;
#pragma unroll
        for (int w = 0; w < GG_WAVES; ++w) {
            const int cw = grp * GG_WAVES + w;
            if (cw < a.n_chunks) rounds = max(rounds, (a.chunks[4 * cw + 2] - a.chunks[4 * cw + 1] + 15) / 16);
        }
        const int c = grp * GG_WAVES + wave;
        const bool active = c < a.n_chunks;
        const int tgt = active ? a.chunks[4 * c] : 0, e0 = active ? a.chunks[4 * c + 1] : 0;
        const int e1 = active ? a.chunks[4 * c + 2] : 0, prow = active ? a.chunks[4 * c + 3] : -1;
        const float* prow_p = a.pq + (rb + tgt) * a.pq_rs;
        const float* drow = a.dagg + (rb + tgt) * a.dagg_rs;
        const bool dvec = a.dvec;
        f32x4 p[KT], dpacc[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) {
            p[kb] = load_piece(prow_p, 16 * kb + 4 * q, a.Hm, a.vec);
            dpacc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        for (int rd = 0; rd < rounds; ++rd) {
            const int t = e0 + 16 * rd;
            f32x4 a1[KT], z[HT];
            if (t < e1) {                                            // wave-uniform
                const int e = t + e16;
                const bool valid = e < e1;
                const int j = valid ? a.src[e] : tgt;
                const float* qrow = a.pq + (rb + j) * a.pq_rs + a.Hm;
                f32x4 d1[KT];
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    const f32x4 qv = load_piece(qrow, 16 * kb + 4 * q, a.Hm, a.vec);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float m, d;
                        act_both(p[kb][s] + qv[s], a.act, m, d);
                        a1[kb][s] = valid ? m : 0.f;
                        d1[kb][s] = valid ? d : 0.f;
                    }
                }
                product<HT, KT>(a.w2p, a.HTa, a.KTa, lane, a1, z);
                float dotg = 0.f, dotd = 0.f;
#pragma unroll
                for (int ot = 0; ot < HT; ++ot) {
                    if (ot >= a.HTa) continue;
                    const f32x4 dv = load_piece(drow, 16 * ot + 4 * q, a.H, dvec);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = 16 * ot + 4 * q + r;
                        const bool in = o < a.H;
                        z[ot][r] = in ? z[ot][r] + a.b2[o] : 0.f;
                        const float m = in ? activate(z[ot][r], a.act) : 0.f;
                        dotg += in ? a.wg[o] * m : 0.f;
                        dotd += dv[r] * m;
                    }
                }
                dotg += __shfl_xor(dotg, 16); dotg += __shfl_xor(dotg, 32);
                dotd += __shfl_xor(dotd, 16); dotd += __shfl_xor(dotd, 32);
                const float g = valid ? sigmoid_f32(dotg + bg) : 0.f;
                const float dgp = valid ? dotd * g * (1.f - g) : 0.f;     // gradient at the gate's pre-activation
                if (q == 0) dbg += dgp;
#pragma unroll
                for (int ot = 0; ot < HT; ++ot) {
                    if (ot >= a.HTa) continue;
                    const f32x4 dv = load_piece(drow, 16 * ot + 4 * q, a.H, dvec);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int o = 16 * ot + 4 * q + r;
                        float m, d;
                        act_both(z[ot][r], a.act, m, d);
                        const bool in = o < a.H;
                        const float wgo = in ? a.wg[o] : 0.f;
                        const float dz = in ? (dv[r] * g + dgp * wgo) * d : 0.f;
                        dwg[ot][r] += in ? dgp * m : 0.f;
                        db2[ot][r] += dz;
                        z[ot][r] = dz;                               // dz2
                    }
                }
                // da1 = W2^T dz2: register r of tile ot is the B operand s = r of k block ot
                f32x4 da[KT];
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    da[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (kt >= a.KTa) continue;
#pragma unroll
                    for (int ot = 0; ot < HT; ++ot) {
                        if (ot >= a.HTa) continue;
                        const f32x4 wf = *reinterpret_cast<const f32x4*>(
                            a.w2tp + (((long long)kt * a.HTa + ot) * 64 + lane) * 4);
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            da[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], z[ot][s], da[kt], 0, 0, 0);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) da[kt][r] *= d1[kt][r];   // dz1 (0 on the lanes past the chunk)
                }
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dpacc[kt][r] += da[kt][r];
                    if (valid && kt < a.KTa)
                        store_piece(a.ws + ((long long)bl * a.n_edges + e) * a.Hm, 16 * kt + 4 * q, a.Hm,
                                    a.Hm % 4 == 0, da[kt]);
                }
            } else {
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) a1[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ot = 0; ot < HT; ++ot) z[ot] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            // this wave's tile into LDS: row = 16 wave + edge, 16 bytes per (tile, q)
            {
                float* dr = dzl + (16 * wave + e16) * SH;
                float* ar = a1l + (16 * wave + e16) * SK;
#pragma unroll
                for (int ot = 0; ot < HT; ++ot) *reinterpret_cast<f32x4*>(dr + 16 * ot + 4 * q) = z[ot];
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) *reinterpret_cast<f32x4*>(ar + 16 * kb + 4 * q) = a1[kb];
            }
            __syncthreads();
            // dW2[o, k] += sum over the 64 edges: A lane (edge 4 u + q, o = 16 ot + e16), B lane (edge, k = 16 kt + e16)
#pragma unroll
            for (int jo = 0; jo < OQ; ++jo) {
                const int ot = wave + GG_WAVES * jo;
                if (ot >= a.HTa) continue;                           // wave-uniform
#pragma unroll 4
                for (int u = 0; u < 16; ++u) {
                    const float av = dzl[(4 * u + q) * SH + 16 * ot + e16];
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt) {
                        const float bv = a1l[(4 * u + q) * SK + 16 * kt + e16];
                        wacc[jo][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, wacc[jo][kt], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
        if (active) {
            float* orow = prow < 0 ? a.out + (rb + tgt) * a.out_rs
                                   : a.part + ((long long)bl * a.n_parts + prow) * a.Hm;
            const bool ovec = a.Hm % 4 == 0 && (prow >= 0 || a.ovec);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                if (kt >= a.KTa) continue;
                const f32x4 v = sum16(dpacc[kt]);
                if (e16 == 0) store_piece(orow, 16 * kt + 4 * q, a.Hm, ovec, v);
            }
        }
    }
    // this workgroup's partial: [H * Hm] dW2, then per wave [H] db2, [H] dwg, [1] dbg
    float* rec = a.wpart + (long long)blockIdx.x * ((long long)a.H * a.Hm + GG_WAVES * (2 * a.H + 1));
#pragma unroll
    for (int jo = 0; jo < OQ; ++jo) {
        const int ot = wave + GG_WAVES * jo;
        if (ot >= a.HTa) continue;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * ot + 4 * q + r, k = 16 * kt + e16;
                if (o < a.H && k < a.Hm) {
                    float* d = rec + (long long)o * a.Hm + k;
                    *d = (a.accum ? *d : 0.f) + wacc[jo][kt][r];
                }
            }
    }
    float* wrec = rec + (long long)a.H * a.Hm + wave * (2 * a.H + 1);
#pragma unroll
    for (int ot = 0; ot < HT; ++ot) {
        if (ot >= a.HTa) continue;
        const f32x4 vb = sum16(db2[ot]), vg = sum16(dwg[ot]);
        if (e16 == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 16 * ot + 4 * q + r;
                if (o < a.H) {
                    wrec[o] = (a.accum ? wrec[o] : 0.f) + vb[r];
                    wrec[a.H + o] = (a.accum ? wrec[a.H + o] : 0.f) + vg[r];
                }
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) dbg += __shfl_xor(dbg, off);
    if (lane == 0) wrec[2 * a.H] = (a.accum ? wrec[2 * a.H] : 0.f) + dbg;
}

// dQ[b, j] = the dz1 rows of the edges OUT OF j (positions pos[ptr[j] .. ptr[j + 1]) of the target-sorted list, in the
// order of the caller's edge list), one wave per row: the list is dealt over 64 / QN lane groups, each adds its share
// in order in fp64, the groups meet in a fixed tree.
__global__ __launch_bounds__(256) void src_sum(const float* __restrict__ ws, const int* __restrict__ ptr,
                                               const int* __restrict__ pos, long long n_edges, int n, int Hm, int qn,
                                               int b0, int nb, float* __restrict__ out, long long out_rs) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)nb * n) return;
    const int bl = (int)(row / n), j = (int)(row % n);
    const int quad = lane % qn, grp = lane / qn, ngrp = 64 / qn;
    const bool vec = Hm % 4 == 0;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int k1 = ptr[j + 1];
    for (int k = ptr[j] + grp; k < k1; k += ngrp) {
        const f32x4 v = load_piece(ws + ((long long)bl * n_edges + pos[k]) * Hm, 4 * quad, Hm, vec);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += (double)v[r];
    }
    for (int off = qn; off < 64; off <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += __shfl_xor(s[r], off);
    if (grp == 0) {
        float* orow = out + ((long long)(b0 + bl) * n + j) * out_rs + Hm;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * quad + r < Hm) orow[4 * quad + r] = (float)s[r];
    }
}

// weight-gradient partials added in workgroup order (fp64)
__global__ void wpart_reduce(const float* __restrict__ wpart, int n_wg, int H, int Hm, float* __restrict__ dw2,
                             float* __restrict__ db2, float* __restrict__ dwg, float* __restrict__ dbg) {
    const long long hw = (long long)H * Hm, rec = hw + GG_WAVES * (2 * H + 1), total = hw + 2 * H + 1;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        double s = 0.0;
        if (e < hw) {
            for (int g = 0; g < n_wg; ++g) s += (double)wpart[g * rec + e];
            dw2[e] = (float)s;
        } else {
            const long long v = e - hw;
            for (int g = 0; g < n_wg; ++g)
                for (int w = 0; w < GG_WAVES; ++w) s += (double)wpart[g * rec + hw + w * (2 * H + 1) + v];
            if (v < H) db2[v] = (float)s;
            else if (v < 2 * H) dwg[v - H] = (float)s;
            else dbg[0] = (float)s;
        }
    }
}

bool supported(int H, int act) { return H >= 16 && H <= 256 && H % 2 == 0 && (act == 1 || act == 2); }

int unsupported(const char* fn, int H, int act) {
    return sgp::fail(SGP_EUNSUP, "%s: hidden width %d / activation code %d outside the kernel's domain (even widths "
                     "16..256, relu = 1 or silu = 2)", fn, H, act);
}

long long align256(long long v) { return (v + 255) / 256 * 256; }

struct BwdPlan { long long slice, n_wg, off_ws, off_wpart, bytes; };

// batch items per pass (the dz1 workspace of a pass stays under the byte cap, one item at least), workgroups, offsets
BwdPlan bwd_plan(long long b, long long n_edges, long long n_chunks, int n_parts, int H) {
    const int Hm = H / 2;
    BwdPlan p;
    const long long cap = (long long)sgp::tune("gated_gn_ws_mb", 256) << 20;
    const long long item = (n_edges > 0 ? n_edges : 1) * Hm * 4;
    p.slice = cap / item;
    if (p.slice < 1) p.slice = 1;
    if (p.slice > b) p.slice = b > 0 ? b : 1;
    const long long rec = ((long long)H * Hm + GG_WAVES * (2 * H + 1)) * 4;
    long long g = GG_PART_BYTES / rec;
    if (g > GG_MAX_WG) g = GG_MAX_WG;
    const long long items = (n_chunks + GG_WAVES - 1) / GG_WAVES * p.slice;
    if (g > items) g = items;
    if (g < 1) g = 1;
    p.n_wg = g;
    p.off_ws = align256(p.slice * n_parts * Hm * 4);
    p.off_wpart = p.off_ws + align256(p.slice * item);
    p.bytes = p.off_wpart + align256(g * rec);
    return p;
}

using sgp::grid_for;

template <int HT, int KT>
int launch_bwd(const GgArgs& a, int n_wg, hipStream_t s) {
    constexpr int SH = 16 * HT + 16;
    constexpr int SK = (16 * KT) % 32 == 16 ? 16 * KT : 16 * KT + 16;
    const int bytes = 64 * (SH + SK) * 4;
    if (bytes > 48 * 1024)                                           // an instantiation asks for this one size only
        if (int rc = sgp::raise_lds_limit<edge_bwd<HT, KT>>(bytes, "gated_gn_edge_bwd")) return rc;
    hipLaunchKernelGGL((edge_bwd<HT, KT>), dim3(n_wg), dim3(64 * GG_WAVES), (size_t)bytes, s, a);
    return sgp::check_launch("gated_gn_edge_bwd");
}

int check_common(const char* fn, const float* PQ, int64_t pq_rs, int32_t b, int32_t n, int32_t H, int32_t act,
                 const int32_t* chunks, int32_t n_chunks, const int32_t* src, int64_t n_edges, const int32_t* fix,
                 int32_t n_fix, int32_t n_parts) {
    if (!supported(H, act)) return unsupported(fn, H, act);
    SGP_REQUIRE(PQ && chunks, "%s: null pointer", fn);
    SGP_REQUIRE(b >= 0 && n > 0 && n_chunks >= n && n_edges >= 0 && n_edges < (1ll << 31) && pq_rs >= H / 2 * 2,
                "%s: bad size", fn);
    SGP_REQUIRE(src || n_edges == 0, "%s: null edge list", fn);
    SGP_REQUIRE(n_fix >= 0 && n_parts >= 0 && (fix || n_fix == 0), "%s: bad split-target table", fn);
    return 0;
}

void fill_common(GgArgs& a, const float* PQ, int64_t pq_rs, int32_t n, int32_t H, int32_t act, const int32_t* chunks,
                 int32_t n_chunks, const int32_t* src, int64_t n_edges, int32_t n_parts, const float* w2p,
                 const float* b2, const float* wg, const float* bg) {
    a.pq = PQ; a.pq_rs = pq_rs; a.n = n; a.H = H; a.Hm = H / 2; a.HTa = (H + 15) / 16; a.KTa = (a.Hm + 15) / 16;
    a.act = act; a.chunks = chunks; a.n_chunks = n_chunks; a.src = src; a.n_edges = n_edges; a.n_parts = n_parts;
    a.w2p = w2p; a.b2 = b2; a.wg = wg; a.bg = bg;
    a.vec = a.Hm % 4 == 0 && pq_rs % 4 == 0 && sgp::aligned16(PQ);
    a.ovec = a.dvec = false; a.dagg = nullptr; a.dagg_rs = 0; a.w2tp = nullptr; a.ws = nullptr; a.wpart = nullptr; a.accum = 0;
}

}  // namespace

extern "C" {

int32_t sgp_gated_gn_supported(int32_t H, int32_t act) {
    if (supported(H, act)) return 1;
    unsupported("sgp_gated_gn_supported", H, act);                   // the reason, for sgp_last_error
    return 0;
}

int32_t sgp_gated_gn_chunk_edges(void) { return GG_CHUNK; }

int64_t sgp_gated_gn_workspace_bytes(int32_t backward, int64_t b, int64_t n_edges, int64_t n_chunks, int32_t n_parts,
                                     int32_t H) {
    if (b < 0 || n_edges < 0 || n_chunks < 0 || n_parts < 0 || H < 2) return -1;
    if (!backward) return align256(b * n_parts * H * 4);
    return bwd_plan(b, n_edges, n_chunks, n_parts, H).bytes;
}

int sgp_gated_gn_edge_f32(const float* PQ, int64_t pq_row_stride, int32_t b, int32_t n, int32_t H, int32_t act,
                          const int32_t* chunks, int32_t n_chunks, const int32_t* src, int64_t n_edges,
                          const int32_t* fix, int32_t n_fix, int32_t n_parts,
                          const float* w2_packed, const float* b2, const float* wg, const float* bg,
                          float* agg, int64_t agg_row_stride, void* work, int64_t work_bytes, sgp_stream_t stream) {
    int rc = check_common("sgp_gated_gn_edge_f32", PQ, pq_row_stride, b, n, H, act, chunks, n_chunks, src, n_edges,
                          fix, n_fix, n_parts);
    if (rc) return rc;
    SGP_REQUIRE(w2_packed && b2 && wg && bg && agg, "sgp_gated_gn_edge_f32: null pointer");
    SGP_REQUIRE(agg_row_stride >= H, "sgp_gated_gn_edge_f32: bad output stride");
    SGP_REQUIRE(sgp::aligned16(w2_packed), "sgp_gated_gn_edge_f32: packed weights must be 16-byte aligned");
    SGP_REQUIRE(n_parts == 0 || (work && sgp::aligned16(work) && work_bytes >= (int64_t)b * n_parts * H * 4),
                "sgp_gated_gn_edge_f32: workspace too small");
    if (b == 0) return 0;
    GgArgs a;
    fill_common(a, PQ, pq_row_stride, n, H, act, chunks, n_chunks, src, n_edges, n_parts, w2_packed, b2, wg, bg);
    a.out = agg; a.out_rs = agg_row_stride; a.part = (float*)work;
    a.ovec = agg_row_stride % 4 == 0 && sgp::aligned16(agg);
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)((n_chunks + GG_WAVES - 1) / GG_WAVES);
    for (int b0 = 0; b0 < b; b0 += 65535) {
        a.b0 = b0; a.nb = b - b0 < 65535 ? b - b0 : 65535;
        const dim3 grid(gx, (unsigned)a.nb), block(64 * GG_WAVES);
        if (H <= 32) hipLaunchKernelGGL((edge_fwd<2, 1>), grid, block, 0, s, a);
        else if (H <= 64) hipLaunchKernelGGL((edge_fwd<4, 2>), grid, block, 0, s, a);
        else if (H <= 128) hipLaunchKernelGGL((edge_fwd<8, 4>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((edge_fwd<16, 8>), grid, block, 0, s, a);
        rc = sgp::check_launch("gated_gn_edge");
        if (rc) return rc;
    }
    if (n_fix > 0) {
        hipLaunchKernelGGL(fix_rows, dim3(grid_for((long long)b * n_fix * H, 256, 8192)), dim3(256), 0, s,
                           (const float*)work, fix, n_fix, n_parts, H, n, 0, b, agg, (long long)agg_row_stride);
        rc = sgp::check_launch("gated_gn_fix_rows");
    }
    return rc;
}

int sgp_gated_gn_edge_bwd_f32(const float* PQ, int64_t pq_row_stride, const float* dAgg, int64_t dagg_row_stride,
                              int32_t b, int32_t n, int32_t H, int32_t act,
                              const int32_t* chunks, int32_t n_chunks, const int32_t* src, int64_t n_edges,
                              const int32_t* fix, int32_t n_fix, int32_t n_parts,
                              const int32_t* src_ptr, const int32_t* src_pos,
                              const float* w2_packed, const float* w2t_packed, const float* b2, const float* wg,
                              const float* bg, float* dPQ, int64_t dpq_row_stride, float* dW2, float* db2, float* dwg,
                              float* dbg, void* work, int64_t work_bytes, sgp_stream_t stream) {
    int rc = check_common("sgp_gated_gn_edge_bwd_f32", PQ, pq_row_stride, b, n, H, act, chunks, n_chunks, src,
                          n_edges, fix, n_fix, n_parts);
    if (rc) return rc;
    SGP_REQUIRE(dAgg && src_ptr && w2_packed && w2t_packed && b2 && wg && bg && dPQ && dW2 && db2 && dwg && dbg && work,
                "sgp_gated_gn_edge_bwd_f32: null pointer");
    SGP_REQUIRE(src_pos || n_edges == 0, "sgp_gated_gn_edge_bwd_f32: null inverted index");
    SGP_REQUIRE(dagg_row_stride >= H && dpq_row_stride >= H / 2 * 2, "sgp_gated_gn_edge_bwd_f32: bad stride");
    SGP_REQUIRE(sgp::aligned16(w2_packed) && sgp::aligned16(w2t_packed) && sgp::aligned16(work),
                "sgp_gated_gn_edge_bwd_f32: packed weights and workspace must be 16-byte aligned");
    const BwdPlan p = bwd_plan(b, n_edges, n_chunks, n_parts, H);
    SGP_REQUIRE(work_bytes >= p.bytes, "sgp_gated_gn_edge_bwd_f32: workspace too small");
    GgArgs a;
    fill_common(a, PQ, pq_row_stride, n, H, act, chunks, n_chunks, src, n_edges, n_parts, w2_packed, b2, wg, bg);
    const int Hm = H / 2;
    a.dagg = dAgg; a.dagg_rs = dagg_row_stride; a.w2tp = w2t_packed;
    a.out = dPQ; a.out_rs = dpq_row_stride;
    a.ovec = dpq_row_stride % 4 == 0 && sgp::aligned16(dPQ);
    a.dvec = H % 4 == 0 && dagg_row_stride % 4 == 0 && sgp::aligned16(dAgg);
    a.part = (float*)work; a.ws = (float*)((char*)work + p.off_ws); a.wpart = (float*)((char*)work + p.off_wpart);
    hipStream_t s = (hipStream_t)stream;
    int qn = 1;
    while (4 * qn < Hm) qn *= 2;
    if (b == 0) {                                                    // no rows: zero gradients
        const long long rec = (long long)H * Hm + GG_WAVES * (2 * H + 1);
        hipError_t e = hipMemsetAsync(a.wpart, 0, (size_t)(p.n_wg * rec * 4), s);
        if (e != hipSuccess) return sgp::fail((int)e, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    for (long long b0 = 0; b0 < b; b0 += p.slice) {
        a.b0 = (int)b0; a.nb = (int)(b - b0 < p.slice ? b - b0 : p.slice);
        a.accum = b0 > 0;
        if (H <= 32) rc = launch_bwd<2, 1>(a, (int)p.n_wg, s);
        else if (H <= 64) rc = launch_bwd<4, 2>(a, (int)p.n_wg, s);
        else if (H <= 128) rc = launch_bwd<8, 4>(a, (int)p.n_wg, s);
        else rc = launch_bwd<16, 8>(a, (int)p.n_wg, s);
        if (rc) return rc;
        if (n_fix > 0) {
            hipLaunchKernelGGL(fix_rows, dim3(grid_for((long long)a.nb * n_fix * Hm, 256, 8192)), dim3(256), 0, s,
                               (const float*)a.part, fix, n_fix, n_parts, Hm, n, 0, a.nb,
                               dPQ + b0 * n * dpq_row_stride, (long long)dpq_row_stride);
            rc = sgp::check_launch("gated_gn_fix_rows");
            if (rc) return rc;
        }
        const long long rows = (long long)a.nb * n;
        SGP_REQUIRE((rows + 3) / 4 < (1ll << 31), "sgp_gated_gn_edge_bwd_f32: too many rows in one pass");
        hipLaunchKernelGGL(src_sum, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const float*)a.ws, src_ptr,
                           src_pos, (long long)n_edges, n, Hm, qn, a.b0, a.nb, dPQ, (long long)dpq_row_stride);
        rc = sgp::check_launch("gated_gn_src_sum");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(wpart_reduce, dim3(grid_for((long long)H * Hm + 2 * H + 1, 256, 4096)), dim3(256), 0, s,
                       (const float*)a.wpart, (int)p.n_wg, H, Hm, dW2, db2, dwg, dbg);
    return sgp::check_launch("gated_gn_wpart_reduce");
}

}  // extern "C"
