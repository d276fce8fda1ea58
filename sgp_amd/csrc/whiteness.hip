// AZ-whiteness test of a residual series on a graph (tsl/ops/test.py): the integer core of the statistic.
//
// For one feature the sign of a product is the product of the signs, so a series [T, N, F] collapses into three bit
// planes per (feature, node): negative | non-zero and valid | valid, 64 steps per 64-bit word.  pack_kernel builds the
// planes and, from a one-bit shift of each word, the temporal sums; the edge kernels AND / XOR / popcount two nodes'
// word rows.  direct_kernel is the general form (the sign of an fp64 dot product over the features) and the
// cross-check of the bit-plane path.  Every sum is an integer: atomics on them are order-independent, and nothing here
// adds floating-point numbers except finish_kernel, whose tree has one fixed order (wg.h).
#include "wg.h"
#include <limits.h>

namespace {

using sgp::in_range;
typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int LDS_FEAT = 64;          // per-feature temporal sums go through LDS up to this many features
constexpr int MAX_WORDS = 65535;      // grid.y of the pack launch: 4.19 M steps per chunk
constexpr int REC = 5;                // doubles per test record: Ct_s | W_s | St | Mt | n_nonfinite

__device__ __forceinline__ void add64(long long* p, long long v) {
    if (v != 0) atomicAdd(reinterpret_cast<u64*>(p), (u64)v);
}

// a workgroup's per-feature (St, Mt) contributions: LDS integer atomics, then one 64-bit atomic per feature
__device__ __forceinline__ void add_per_feature(int* sh, int F, bool live, int f, int st, int mt, long long* St, long long* Mt) {
    if (F <= LDS_FEAT) {
        if (live) {
            if (st != 0) atomicAdd(&sh[f], st);
            if (mt != 0) atomicAdd(&sh[F + f], mt);
        }
        __syncthreads();
        if ((int)threadIdx.x < F) {
            add64(St + threadIdx.x, sh[threadIdx.x]);
            add64(Mt + threadIdx.x, sh[F + threadIdx.x]);
        }
    } else if (live) {
        add64(St + f, st);
        add64(Mt + f, mt);
    }
}

__device__ __forceinline__ bool nonfinite_bits(unsigned b) { return (b & 0x7f800000u) == 0x7f800000u; }

// ------------------------------------------------------------------------------------------------------- bit planes
// Lane (n, f) of word w walks the steps 64 w .. 64 w + 63: a step's loads are contiguous across the wave.  planes is
// [3][F][N][W]; carry rows hold the three bits of the step before / the last step of this chunk per (n, f).
__global__ __launch_bounds__(THREADS) void pack_kernel(const float* __restrict__ x, long long xs_t, long long xs_n,
                                                       const uint8_t* __restrict__ mask, long long ms_t, long long ms_n,
                                                       int T, int N, int F, int W, const uint8_t* __restrict__ carry_in,
                                                       uint8_t* __restrict__ carry_out, u64* __restrict__ planes,
                                                       long long* St, long long* Mt, long long* nonfinite) {
    __shared__ int sh[2 * LDS_FEAT];
    if (F <= LDS_FEAT) {
        for (int k = threadIdx.x; k < 2 * F; k += THREADS) sh[k] = 0;
        __syncthreads();
    }
    const long long NF = (long long)N * F;
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int w = blockIdx.y;
    const bool live = in_range(i, NF) && in_range(w, W);
    int f = 0, st = 0, mt = 0, bad = 0;
    if (live) {
        const int n = (int)(i / F);
        f = (int)(i - (long long)n * F);
        const int t0 = w * 64;
        const int cnt = T - t0 < 64 ? T - t0 : 64;
        const float* xp = x + t0 * xs_t + n * xs_n + f;
        const uint8_t* mp = mask ? mask + t0 * ms_t + n * ms_n + f : nullptr;
        u64 neg = 0, nz = 0, val = 0;
#pragma unroll 8
        for (int b = 0; b < cnt; ++b) {
            const bool v = mp ? mp[b * ms_t] != 0 : true;
            const unsigned bits = __float_as_uint(xp[b * xs_t]);
            neg |= (u64)(bits >> 31) << b;
            nz |= (u64)(v && (bits & 0x7fffffffu) != 0) << b;
            val |= (u64)v << b;
            bad += v && nonfinite_bits(bits);
        }
        // the step before this word: the last one of the word below, or the carry row of the chunk before
        unsigned pneg = 0, pnz = 0, pval = 0;
        if (w > 0) {
            const bool v = mp ? *(mp - ms_t) != 0 : true;
            const unsigned bits = __float_as_uint(*(xp - xs_t));
            pneg = bits >> 31; pnz = v && (bits & 0x7fffffffu) != 0; pval = v;
        } else if (carry_in) {
            const unsigned c = carry_in[i];
            pneg = c & 1u; pnz = (c >> 1) & 1u; pval = (c >> 2) & 1u;
        }
        const u64 sneg = (neg << 1) | pneg, snz = (nz << 1) | pnz, sval = (val << 1) | pval;
        const u64 pair = nz & snz;
        st = __popcll(pair) - 2 * __popcll((neg ^ sneg) & pair);
        mt = __popcll(val & sval);
        const long long row = (long long)n * W + w, plane = NF * W;
        planes[(long long)f * N * W + row] = neg;
        planes[plane + (long long)f * N * W + row] = nz;
        planes[2 * plane + (long long)f * N * W + row] = val;
        if (w == W - 1 && carry_out) {
            const int b = cnt - 1;
            carry_out[i] = (uint8_t)(((neg >> b) & 1u) | (((nz >> b) & 1u) << 1) | (((val >> b) & 1u) << 2));
        }
        add64(nonfinite, bad);
    }
    add_per_feature(sh, F, live, f, st, mt, St, Mt);
}

__device__ __forceinline__ void edge_word(const u64* __restrict__ neg, const u64* __restrict__ nz, const u64* __restrict__ val,
                                          long long ru, long long rv, int& s, int& m) {
    const u64 both = nz[ru] & nz[rv];
    s += __popcll(both) - 2 * __popcll((neg[ru] ^ neg[rv]) & both);
    m += __popcll(val[ru] & val[rv]);
}

// "words": one wave per (edge, feature), lanes along the W words of the two rows (long series)
__global__ __launch_bounds__(THREADS) void edge_words_kernel(const u64* __restrict__ planes, const int* __restrict__ eu,
                                                             const int* __restrict__ ev, long long E, int N, int F, int W,
                                                             long long* __restrict__ S, long long* __restrict__ M) {
    const long long g = (long long)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6);
    if (!in_range(g, E * F)) return;
    const long long e = g / F;
    const int f = (int)(g - e * F), lane = threadIdx.x & 63;
    const int u = eu[e], v = ev[e];
    if (!in_range(u, N) || !in_range(v, N)) return;
    const long long plane = (long long)N * F * W;
    const u64* neg = planes + (long long)f * N * W;
    const long long ru = (long long)u * W, rv = (long long)v * W;
    int s = 0, m = 0;
    for (int w = lane; w < W; w += 64) edge_word(neg, neg + plane, neg + 2 * plane, ru + w, rv + w, s, m);
    s = sgp::wave_sum(s);
    m = sgp::wave_sum(m);
    if (lane == 0) { S[g] += s; M[g] += m; }          // the wave owns (e, f); launches of one stream are ordered
}

// "edges": one lane per (feature, edge), each walks its W words (short series); neighbouring lanes take neighbouring
// edges of the sorted list, which share their first node
__global__ __launch_bounds__(THREADS) void edge_lanes_kernel(const u64* __restrict__ planes, const int* __restrict__ eu,
                                                             const int* __restrict__ ev, long long E, int N, int F, int W,
                                                             long long* __restrict__ S, long long* __restrict__ M) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (!in_range(g, E * F)) return;
    const int f = (int)(g / E);
    const long long e = g - (long long)f * E;
    const int u = eu[e], v = ev[e];
    if (!in_range(u, N) || !in_range(v, N)) return;
    const long long plane = (long long)N * F * W;
    const u64* neg = planes + (long long)f * N * W;
    const long long ru = (long long)u * W, rv = (long long)v * W;
    int s = 0, m = 0;
    for (int w = 0; w < W; ++w) edge_word(neg, neg + plane, neg + 2 * plane, ru + w, rv + w, s, m);
    S[e * F + f] += s;
    M[e * F + f] += m;
}

// ----------------------------------------------------------------------------------------------------- general form
// Workgroups 0 .. edge_blocks - 1: a lane owns an edge (MULTI) or an (edge, feature) over the time slab blockIdx.y,
// gathers the two rows, forms the fp64 dot product (f ascending; the products of fp32 values are exact) and counts its
// sign.  The workgroups behind them are node tiles: the same over (t - 1, t) for the temporal sums.  prev_x / prev_m:
// the last step of the chunk before ([N, F] contiguous), or NULL.
struct Series {
    const float* x; long long xs_t, xs_n;
    const uint8_t* mask; long long ms_t, ms_n;
    __device__ __forceinline__ bool valid(int t, int n, int f) const { return mask ? mask[t * ms_t + n * ms_n + f] != 0 : true; }
    __device__ __forceinline__ float at(int t, int n, int f) const { return x[t * xs_t + n * xs_n + f]; }
};

template <bool MULTI>
__global__ __launch_bounds__(THREADS) void direct_kernel(Series X, const float* __restrict__ prev_x, const uint8_t* __restrict__ prev_m,
                                                         int T, int N, int F, const int* __restrict__ eu, const int* __restrict__ ev,
                                                         long long E, unsigned edge_blocks, int slab, long long* __restrict__ S,
                                                         long long* __restrict__ M, long long* St, long long* Mt, long long* nonfinite) {
    __shared__ int sh[2 * LDS_FEAT];
    const int t0 = blockIdx.y * slab;
    const int t1 = T - t0 < slab ? T : t0 + slab;
    if (blockIdx.x < edge_blocks) {
        const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
        if (!in_range(g, MULTI ? E : E * F)) return;
        const long long e = MULTI ? g : g / F;
        const int f0 = MULTI ? 0 : (int)(g - e * F), nf = MULTI ? F : 1;
        const int u = eu[e], v = ev[e];
        if (!in_range(u, N) || !in_range(v, N)) return;
        int s = 0, m = 0;
        for (int t = t0; t < t1; ++t) {
            double dot = 0.0;
            bool vu = false, vv = false;
            for (int k = 0; k < nf; ++k) {
                const bool mu = X.valid(t, u, f0 + k), mv = X.valid(t, v, f0 + k);
                const double a = mu ? (double)X.at(t, u, f0 + k) : 0.0, b = mv ? (double)X.at(t, v, f0 + k) : 0.0;
                dot += a * b;
                vu |= mu; vv |= mv;
            }
            s += (dot > 0.0) - (dot < 0.0);
            m += vu && vv;
        }
        add64(S + g, s);
        add64(M + g, m);
        return;
    }
    if (!MULTI && F <= LDS_FEAT) {
        for (int k = threadIdx.x; k < 2 * F; k += THREADS) sh[k] = 0;
        __syncthreads();
    }
    const long long g = (long long)(blockIdx.x - edge_blocks) * THREADS + threadIdx.x;
    const bool live = in_range(g, MULTI ? (long long)N : (long long)N * F);
    int f0 = 0, st = 0, mt = 0, bad = 0;
    if (live) {
        const int n = MULTI ? (int)g : (int)(g / F);
        f0 = MULTI ? 0 : (int)(g - (long long)n * F);
        const int nf = MULTI ? F : 1;
        for (int t = t0; t < t1; ++t) {
            const bool has_prev = t > 0 || prev_x != nullptr;
            double dot = 0.0;
            for (int k = 0; k < nf; ++k) {
                const int f = f0 + k;
                const bool mc = X.valid(t, n, f);
                const float c = X.at(t, n, f);
                bad += mc && nonfinite_bits(__float_as_uint(c));
                if (!has_prev) continue;
                const bool mp = t > 0 ? X.valid(t - 1, n, f) : (prev_m ? prev_m[(long long)n * F + f] != 0 : true);
                const float p = t > 0 ? X.at(t - 1, n, f) : prev_x[(long long)n * F + f];
                dot += (mc ? (double)c : 0.0) * (mp ? (double)p : 0.0);
                mt += mc && mp;
            }
            st += (dot > 0.0) - (dot < 0.0);
        }
        add64(nonfinite, bad);
    }
    if (MULTI) {
        st = sgp::wave_sum(st);
        mt = sgp::wave_sum(mt);
        if ((threadIdx.x & 63) == 0) { add64(St, st); add64(Mt, mt); }
    } else {
        add_per_feature(sh, F, live, f0, st, mt, St, Mt);
    }
}

// ----------------------------------------------------------------------------------------------------------- finish
// One workgroup per test: thread k adds the edges k, k + THREADS, .. in order, then the halving tree of wg.h.
__global__ __launch_bounds__(THREADS) void finish_kernel(const long long* __restrict__ S, const long long* __restrict__ M,
                                                         const double* __restrict__ w, long long E, int n_tests,
                                                         const long long* __restrict__ St, const long long* __restrict__ Mt,
                                                         const long long* __restrict__ nonfinite, double* __restrict__ rec) {
    __shared__ double sh[2][THREADS];
    const int k = blockIdx.x;
    double c = 0.0, ws = 0.0;
    for (long long e = threadIdx.x; e < E; e += THREADS) {
        const double we = w[e];
        c += we * (double)S[e * n_tests + k];
        ws += we * we * (double)M[e * n_tests + k];
    }
    sh[0][threadIdx.x] = c;
    sh[1][threadIdx.x] = ws;
    sgp::wg_reduce<THREADS>([&](int a, int b) { sh[0][a] += sh[0][b]; sh[1][a] += sh[1][b]; });
    if (threadIdx.x == 0) {
        double* r = rec + (long long)k * REC;
        r[0] = sh[0][0]; r[1] = sh[1][0]; r[2] = (double)St[k]; r[3] = (double)Mt[k]; r[4] = (double)nonfinite[0];
    }
}

int check_series(const char* what, int64_t xs_t, int64_t xs_n, const void* mask, int64_t ms_t, int64_t ms_n, int64_t steps,
                 int64_t nodes, int32_t feat) {
    SGP_REQUIRE(steps > 0 && nodes > 0 && feat > 0, "%s: sizes must be positive (steps=%lld, nodes=%lld, feat=%d)", what,
                (long long)steps, (long long)nodes, (int)feat);
    SGP_REQUIRE(steps <= 64ll * MAX_WORDS && nodes * feat <= INT_MAX, "%s: steps=%lld or nodes x feat=%lld is out of range",
                what, (long long)steps, (long long)(nodes * feat));
    SGP_REQUIRE(xs_n >= feat && xs_t >= 0 && (!mask || (ms_n >= feat && ms_t >= 0)), "%s: bad strides", what);
    return 0;
}

}  // namespace

extern "C" {

int sgp_az_pack_f32(const float* x, int64_t x_step_stride, int64_t x_node_stride, const uint8_t* mask,
                    int64_t mask_step_stride, int64_t mask_node_stride, int64_t steps, int64_t nodes, int32_t feat,
                    const uint8_t* carry_in, uint8_t* carry_out, uint64_t* planes, int64_t* st, int64_t* mt,
                    int64_t* nonfinite, sgp_stream_t stream) {
    SGP_REQUIRE(x && planes && st && mt && nonfinite, "sgp_az_pack_f32: null pointer");
    if (int rc = check_series("sgp_az_pack_f32", x_step_stride, x_node_stride, mask, mask_step_stride, mask_node_stride,
                              steps, nodes, feat)) return rc;
    const int W = (int)((steps + 63) / 64);
    SGP_REQUIRE(nodes * feat <= LLONG_MAX / 24 / W, "sgp_az_pack_f32: the planes are out of range");
    const dim3 grid((unsigned)((nodes * feat + THREADS - 1) / THREADS), (unsigned)W);
    hipLaunchKernelGGL(pack_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, x, (long long)x_step_stride,
                       (long long)x_node_stride, mask, (long long)mask_step_stride, (long long)mask_node_stride, (int)steps,
                       (int)nodes, (int)feat, W, carry_in, carry_out, (u64*)planes, (long long*)st, (long long*)mt,
                       (long long*)nonfinite);
    return sgp::check_launch("sgp_az_pack_f32");
}

int sgp_az_edge_counts(const uint64_t* planes, const int32_t* edge_u, const int32_t* edge_v, int64_t n_edges, int64_t nodes,
                       int32_t feat, int64_t words, int32_t regime, int64_t* s, int64_t* m, sgp_stream_t stream) {
    SGP_REQUIRE(planes && edge_u && edge_v && s && m, "sgp_az_edge_counts: null pointer");
    SGP_REQUIRE(n_edges >= 0 && nodes > 0 && feat > 0 && words > 0 && words <= MAX_WORDS && nodes * feat <= INT_MAX,
                "sgp_az_edge_counts: bad sizes (edges=%lld, nodes=%lld, feat=%d, words=%lld)", (long long)n_edges,
                (long long)nodes, (int)feat, (long long)words);
    SGP_REQUIRE(regime == 0 || regime == 1, "sgp_az_edge_counts: regime must be 0 (words) or 1 (edges)");
    SGP_REQUIRE(n_edges <= INT_MAX / feat, "sgp_az_edge_counts: %lld edges x %d features are out of range",
                (long long)n_edges, (int)feat);
    if (n_edges == 0) return 0;
    const long long items = (long long)n_edges * feat, per = regime == 0 ? THREADS / 64 : THREADS;
    const dim3 grid((unsigned)((items + per - 1) / per));
    if (regime == 0)
        hipLaunchKernelGGL(edge_words_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, (const u64*)planes, edge_u, edge_v,
                           (long long)n_edges, (int)nodes, (int)feat, (int)words, (long long*)s, (long long*)m);
    else
        hipLaunchKernelGGL(edge_lanes_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream, (const u64*)planes, edge_u, edge_v,
                           (long long)n_edges, (int)nodes, (int)feat, (int)words, (long long*)s, (long long*)m);
    return sgp::check_launch("sgp_az_edge_counts");
}

int sgp_az_direct_f32(const float* x, int64_t x_step_stride, int64_t x_node_stride, const uint8_t* mask,
                      int64_t mask_step_stride, int64_t mask_node_stride, const float* prev_x, const uint8_t* prev_mask,
                      int64_t steps, int64_t nodes, int32_t feat, int32_t multivariate, const int32_t* edge_u,
                      const int32_t* edge_v, int64_t n_edges, int32_t slab, int64_t* s, int64_t* m, int64_t* st, int64_t* mt,
                      int64_t* nonfinite, sgp_stream_t stream) {
    SGP_REQUIRE(x && edge_u && edge_v && s && m && st && mt && nonfinite, "sgp_az_direct_f32: null pointer");
    if (int rc = check_series("sgp_az_direct_f32", x_step_stride, x_node_stride, mask, mask_step_stride, mask_node_stride,
                              steps, nodes, feat)) return rc;
    SGP_REQUIRE(n_edges >= 0 && n_edges <= INT_MAX / feat, "sgp_az_direct_f32: %lld edges x %d features are out of range",
                (long long)n_edges, (int)feat);
    SGP_REQUIRE(slab >= 1 && (steps + slab - 1) / slab <= MAX_WORDS, "sgp_az_direct_f32: bad time slab %d for %lld steps",
                (int)slab, (long long)steps);
    SGP_REQUIRE(!prev_x || !mask || prev_mask, "sgp_az_direct_f32: a masked series needs the mask of the step before");
    const bool multi = multivariate != 0;
    const long long e_items = multi ? n_edges : n_edges * feat, n_items = multi ? nodes : nodes * feat;
    const unsigned eb = (unsigned)((e_items + THREADS - 1) / THREADS), nb = (unsigned)((n_items + THREADS - 1) / THREADS);
    const dim3 grid(eb + nb, (unsigned)((steps + slab - 1) / slab));
    const Series X{x, (long long)x_step_stride, (long long)x_node_stride, mask, (long long)mask_step_stride,
                   (long long)mask_node_stride};
    if (multi)
        hipLaunchKernelGGL(direct_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream, X, prev_x, prev_mask, (int)steps,
                           (int)nodes, (int)feat, edge_u, edge_v, (long long)n_edges, eb, (int)slab, (long long*)s,
                           (long long*)m, (long long*)st, (long long*)mt, (long long*)nonfinite);
    else
        hipLaunchKernelGGL(direct_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream, X, prev_x, prev_mask, (int)steps,
                           (int)nodes, (int)feat, edge_u, edge_v, (long long)n_edges, eb, (int)slab, (long long*)s,
                           (long long*)m, (long long*)st, (long long*)mt, (long long*)nonfinite);
    return sgp::check_launch("sgp_az_direct_f32");
}

int sgp_az_finish(const int64_t* s, const int64_t* m, const double* weight, int64_t n_edges, int32_t n_tests,
                  const int64_t* st, const int64_t* mt, const int64_t* nonfinite, double* rec, sgp_stream_t stream) {
    SGP_REQUIRE(s && m && weight && st && mt && nonfinite && rec, "sgp_az_finish: null pointer");
    SGP_REQUIRE(n_edges >= 0 && n_tests > 0 && n_tests <= 65535 && n_edges <= LLONG_MAX / n_tests,
                "sgp_az_finish: bad sizes (edges=%lld, tests=%d)", (long long)n_edges, (int)n_tests);
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)n_tests), dim3(THREADS), 0, (hipStream_t)stream, (const long long*)s,
                       (const long long*)m, weight, (long long)n_edges, (int)n_tests, (const long long*)st,
                       (const long long*)mt, (const long long*)nonfinite, rec);
    return sgp::check_launch("sgp_az_finish");
}

}  // extern "C"
