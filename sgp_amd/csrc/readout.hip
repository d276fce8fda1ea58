// Closed-form ridge readout (experiments/run_closed_form.py:169-247 of the reference): the Gram matrix of a VIRTUAL
// design matrix, its column means, and one predict + masked-metric pass.  Nothing is materialised: row r = (s, n) of
// the matrix is node n at step steps[s], and its columns come from up to 8 segments, each an fp32 tensor slice
//   value(s, n, q * width + c) = base[(steps[s] + off + q) * step_stride + n * node_stride + c],  c < width, q < reps
// laid side by side (q > 0: the targets of lags 2 .. H as one segment) (include/sgp_amd.h, "Ridge readout").  Every reduction is fp64 in a fixed order: no atomics,
// results are bit-identical run to run.
#include "common.h"

namespace {

constexpr int kMaxSegs = 8;
constexpr int NXCD = 8;

// Gram: 128 x 128 output tiles, 4 waves as 2 x 2 of 64 x 64 (2 x 2 v_mfma_f32_32x32x2_f32 tiles each), 32 rows per
// LDS stage, the fp32 partial of at most 256 rows added into the fp64 slab of the workgroup's (slice, tile).
constexpr int GT = 128;
constexpr int GKB = 32;
constexpr int GFLUSH = 256;         // rows per fp32 partial (each partial then goes into fp64)
constexpr int GLD = GT + 32;        // LDS row stride: the two half-waves of an A/B read land on disjoint banks
constexpr int GTILE = GT * GT;
constexpr int GWG_TARGET = 2048;    // slices are chosen so that tiles x slices is about this many workgroups

// colmeans: one thread per column, rows split into at most 1024 slices
constexpr int CM_MAX_SLICES = 1024;

// predict: 64 rows per block iteration (16 per wave), k panels of 32 columns, W resident in LDS
constexpr int PRB = 64;
constexpr int PKB = 32;
constexpr int PLD = PKB + 1;
constexpr int PGRID = 512;

struct Seg {
    const float* base;
    int64_t ss, ns;
    int32_t width, off, col0, span;     // span = width * reps columns
};
struct Segs {
    Seg s[kMaxSegs];
    int32_t n, ncols;
};

// where column c of the virtual matrix comes from: kind 0 = a segment, 1 = the ones column, 2 = zero padding
struct ColSrc {
    const float* p;
    int64_t ss, ns;
    int32_t off, kind;
};

__device__ inline ColSrc resolve(const Segs& S, int c, int ones) {
    ColSrc r{nullptr, 0, 0, 0, 2};
    if (c < S.ncols) {
#pragma unroll
        for (int k = 0; k < kMaxSegs; ++k)      // unrolled: no dynamic index into the kernel-argument table
            if (k < S.n && c >= S.s[k].col0 && c < S.s[k].col0 + S.s[k].span) {
                const int q = (c - S.s[k].col0) / S.s[k].width, cc = c - S.s[k].col0 - q * S.s[k].width;
                r.p = S.s[k].base + (int64_t)q * S.s[k].ss + cc;
                r.ss = S.s[k].ss;
                r.ns = S.s[k].ns;
                r.off = S.s[k].off;
                r.kind = 0;
            }
    } else if (ones && c == S.ncols) {
        r.kind = 1;
    }
    return r;
}

__device__ inline float fetch(const ColSrc& c, int step, int node, float shift) {
    if (step < 0 || c.kind == 2) return 0.f;                 // row past the end, or padding column
    if (c.kind == 1) return 1.f;
    return c.p[(int64_t)(step + c.off) * c.ss + (int64_t)node * c.ns] - shift;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ column means
__global__ __launch_bounds__(256) void ridge_colsum_kernel(Segs S, const int32_t* __restrict__ steps, int64_t n_nodes,
                                                         int64_t n_rows, int64_t rows_per_slice,
                                                         double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= S.ncols) return;
    const ColSrc src = resolve(S, c, 0);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t r1 = r0 + rows_per_slice < n_rows ? r0 + rows_per_slice : n_rows;
    double acc = 0.0;
    if (r0 < r1) {
        int64_t s = r0 / n_nodes, n = r0 - s * n_nodes;
        const float* p = src.p + (int64_t)(steps[s] + src.off) * src.ss;
        for (int64_t r = r0; r < r1; ++r) {
            acc += (double)p[n * src.ns];
            if (++n == n_nodes && r + 1 < r1) {
                n = 0;
                ++s;
                p = src.p + (int64_t)(steps[s] + src.off) * src.ss;
            }
        }
    }
    part[(int64_t)blockIdx.y * S.ncols + c] = acc;
}

__global__ void ridge_colmean_final_kernel(const double* __restrict__ part, int n_slices, int ncols, int64_t n_rows,
                                           double* __restrict__ means) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    double s = 0.0;
    for (int k = 0; k < n_slices; ++k) s += part[(int64_t)k * ncols + c];
    means[c] = s / (double)n_rows;
}

// ------------------------------------------------------------------ Gram
__device__ inline void upper_tile(int tile, int nt1, int& ti, int& tj) {
    int t = 0, rem = tile;
    while (rem >= nt1 - t) {
        rem -= nt1 - t;
        ++t;
    }
    ti = t;
    tj = t + rem;
}

__global__ __launch_bounds__(256) void ridge_gram_kernel(Segs S, const int32_t* __restrict__ steps, int64_t n_nodes,
                                                       int64_t n_rows, const float* __restrict__ shift, int ones,
                                                       int nt1, int n_tiles, int64_t rows_per_slice,
                                                       double* __restrict__ part) {
    __shared__ float sA[GKB * GLD], sB[GKB * GLD];
    __shared__ int rstep[2][GKB], rnode[2][GKB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // workgroups of one row slice share an XCD (blockIdx % 8 labels the XCD the dispatcher deals a block to): the
    // slice's column panels are read from HBM once and then served from that XCD's L2 to all its tiles
    const int bid = blockIdx.x, local = bid / NXCD;
    const int slice = (local / n_tiles) * NXCD + bid % NXCD, tile = local % n_tiles;
    int ti, tj;
    upper_tile(tile, nt1, ti, tj);

    const int ldcol = tid & (GT - 1), ldrow = tid >> 7;       // staging: one column, rows ldrow + 2q
    const ColSrc ca = resolve(S, ti * GT + ldcol, ones), cb = resolve(S, tj * GT + ldcol, ones);
    const float sha = (shift && ca.kind == 0) ? shift[ti * GT + ldcol] : 0.f;
    const float shb = (shift && cb.kind == 0) ? shift[tj * GT + ldcol] : 0.f;

    const int64_t r0 = (int64_t)slice * rows_per_slice;
    const int64_t r1 = r0 + rows_per_slice < n_rows ? r0 + rows_per_slice : n_rows;
    const int64_t nblk = r1 > r0 ? (r1 - r0 + GKB - 1) / GKB : 0;

    auto rowinfo = [&](int64_t kb, int buf) {
        if (tid < GKB) {
            const int64_t r = r0 + kb * GKB + tid;
            int st = -1, nd = 0;
            if (r < r1) {
                const int64_t s = r / n_nodes;
                nd = (int)(r - s * n_nodes);
                st = steps[s];
            }
            rstep[buf][tid] = st;
            rnode[buf][tid] = nd;
        }
    };
    float va[GKB / 2], vb[GKB / 2];
    auto load = [&](int buf) {
#pragma unroll
        for (int q = 0; q < GKB / 2; ++q) {
            const int row = ldrow + 2 * q;                  // wave-uniform: the row's step and node go to SGPRs
            const int st = __builtin_amdgcn_readfirstlane(rstep[buf][row]);
            const int nd = __builtin_amdgcn_readfirstlane(rnode[buf][row]);
            va[q] = fetch(ca, st, nd, sha);
            vb[q] = fetch(cb, st, nd, shb);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16){};
    double* slab = part + ((int64_t)slice * n_tiles + tile) * GTILE;
    // the lane's 64 results stay in their register order in the slab ([wave][a][b][reg][lane]); the reduce decodes it
    auto flush = [&](bool first) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    double* d = slab + ((((w * 2 + a) * 2 + b) * 16 + r) * 64 + lane);
                    const double v = (double)acc[a][b][r];
                    *d = first ? v : *d + v;
                    acc[a][b][r] = 0.f;
                    if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // 4 slab loads in flight, not 64
                }
    };

    const int wi = w >> 1, wj = w & 1, kl = lane >> 5, il = lane & 31;
    if (nblk > 0) {
        rowinfo(0, 0);
        __syncthreads();
        load(0);
    }
    bool first = true;
    int since = 0;
    for (int64_t kb = 0; kb < nblk; ++kb) {
        const int buf = (int)(kb & 1);
#pragma unroll
        for (int q = 0; q < GKB / 2; ++q) {
            sA[(ldrow + 2 * q) * GLD + ldcol] = va[q];
            sB[(ldrow + 2 * q) * GLD + ldcol] = vb[q];
        }
        if (kb + 1 < nblk) rowinfo(kb + 1, buf ^ 1);
        __syncthreads();
        if (kb + 1 < nblk) load(buf ^ 1);                  // next stage's loads in flight under this stage's MFMAs
#pragma unroll
        for (int kk = 0; kk < GKB / 2; ++kk) {
            const float* ra = sA + (2 * kk + kl) * GLD + wi * 64 + il;
            const float* rb = sB + (2 * kk + kl) * GLD + wj * 64 + il;
            const float a0 = ra[0], a1 = ra[32], b0 = rb[0], b1 = rb[32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
        if (++since == GFLUSH / GKB || kb + 1 == nblk) {
            flush(first);
            first = false;
            since = 0;
        }
    }
    if (first) flush(true);                                  // empty slice: a zero slab
}

// G[i][j] = G[j][i] = sum over slices (in slice order) of the slab entries of (i, j), i <= j
__global__ void ridge_gram_reduce_kernel(const double* __restrict__ part, int n_slices, int n_tiles, int nt1, int mp,
                                         double* __restrict__ G, int64_t ldg) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n_tiles * GTILE) return;
    const int tile = (int)(idx / GTILE), e = (int)(idx % GTILE);
    int ti, tj;
    upper_tile(tile, nt1, ti, tj);
    const int lane = e & 63, reg = (e >> 6) & 15, b = (e >> 10) & 1, a = (e >> 11) & 1, w = e >> 12;
    // 32x32 C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int i = ti * GT + (w >> 1) * 64 + a * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    const int j = tj * GT + (w & 1) * 64 + b * 32 + (lane & 31);
    if (i >= mp || j >= mp || i > j) return;
    double s = 0.0;
    for (int k = 0; k < n_slices; ++k) s += part[((int64_t)k * n_tiles + tile) * GTILE + e];
    G[(int64_t)i * ldg + j] = s;
    G[(int64_t)j * ldg + i] = s;
}

// Node-invariant columns (a segment of node stride 0, the ones column) hold one value for the n_nodes rows of a step.
// The MFMA partial adds such a pair's product n_nodes times in a row, and every one of those additions rounds the same
// way: the error grows with the run instead of averaging out (8.6e-7 Sum|a b| measured with 22 such columns over 29
// nodes).  Their products are therefore redone here as n_nodes x the fp64 sum over the steps, in a fixed order:
// one workgroup per pair (i <= j) of the `nb` invariant columns, thread t takes steps t, t + 256, ...
__device__ inline int invariant_col(const Segs& S, int ones, int b) {
    int col = -1;
#pragma unroll
    for (int k = 0; k < kMaxSegs; ++k)
        if (k < S.n && S.s[k].ns == 0) {
            if (col < 0 && b >= 0 && b < S.s[k].span) col = S.s[k].col0 + b;
            b -= S.s[k].span;
        }
    if (col < 0 && ones && b == 0) col = S.ncols;
    return col;
}

__global__ __launch_bounds__(256) void ridge_gram_invariant_kernel(Segs S, const int32_t* __restrict__ steps,
                                                                 int64_t n_steps, int64_t n_nodes,
                                                                 const float* __restrict__ shift, int ones, int nb,
                                                                 double* __restrict__ G, int64_t ldg) {
    __shared__ double red[256];
    const int bi = blockIdx.x / nb, bj = blockIdx.x % nb;
    if (bi > bj) return;                                     // the whole workgroup
    const int i = invariant_col(S, ones, bi), j = invariant_col(S, ones, bj);
    const ColSrc ca = resolve(S, i, ones), cb = resolve(S, j, ones);
    const float sha = (shift && ca.kind == 0) ? shift[i] : 0.f;
    const float shb = (shift && cb.kind == 0) ? shift[j] : 0.f;
    double acc = 0.0;
    for (int64_t s = threadIdx.x; s < n_steps; s += 256) {
        const int st = steps[s];
        acc += (double)fetch(ca, st, 0, sha) * (double)fetch(cb, st, 0, shb);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t += red[k];
        t *= (double)n_nodes;
        G[(int64_t)i * ldg + j] = t;
        G[(int64_t)j * ldg + i] = t;
    }
}

// ------------------------------------------------------------------ predict + score
struct Score {
    const float* scale;  // inverse scaler, element (n, c) at n * sc_ns + c; nullptr = no inverse transform
    const float* bias;
    int64_t sc_ns;
    const float* y;      // raw target (t, n, c) at t * y_ss + n * y_ns + c; nullptr = no scoring
    int64_t y_ss, y_ns;
    const uint8_t* mask; // (t, n, c) at t * m_ss + n * m_ns + c * m_cs; nullptr = every target counts
    int64_t m_ss, m_ns, m_cs;
    float* yhat;         // [S, H, N, C] or nullptr
};

template <int NT>
__global__ __launch_bounds__(256) void ridge_predict_kernel(Segs S, const int32_t* __restrict__ steps, int64_t n_nodes,
                                                          int64_t n_rows, const float* __restrict__ W,
                                                          const double* __restrict__ bvec, int H, int C, int dpad,
                                                          Score sc, double* __restrict__ part) {
    constexpr int HCP = 16 * NT;
    extern __shared__ float lds[];
    float* Wl = lds;                                 // [dpad][HCP]
    float* X = Wl + (int64_t)dpad * HCP;             // [PRB][PLD]
    double* red = reinterpret_cast<double*>(X + PRB * PLD);  // [16][HCP][4]; both sizes above are even
    __shared__ int rstep[PRB], rnode[PRB], rsidx[PRB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int HC = H * C, D = S.ncols;

    for (int e = tid; e < dpad * HCP; e += 256) {
        const int k = e / HCP, j = e % HCP;
        Wl[e] = (k < D && j < HC) ? W[(int64_t)k * HC + j] : 0.f;
    }
    double sums[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t) sums[t][0] = sums[t][1] = sums[t][2] = sums[t][3] = 0.0;

    const int ldcol = tid & (PKB - 1), ldrow = tid >> 5;     // staging: one column, rows ldrow + 8q
    const int npan = dpad / PKB;
    const int64_t nrb = (n_rows + PRB - 1) / PRB;
    float v[PRB / 8];
    auto load = [&](int kp) {
        const ColSrc c = resolve(S, kp * PKB + ldcol, 0);
#pragma unroll
        for (int q = 0; q < PRB / 8; ++q) {
            const int row = ldrow + 8 * q;
            v[q] = fetch(c, rstep[row], rnode[row], 0.f);
        }
    };

    for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        __syncthreads();                                     // W staged / previous block's epilogue done with rowinfo
        if (tid < PRB) {
            const int64_t r = rb * PRB + tid;
            int st = -1, nd = 0, si = 0;
            if (r < n_rows) {
                const int64_t s = r / n_nodes;
                nd = (int)(r - s * n_nodes);
                si = (int)s;
                st = steps[s];
            }
            rstep[tid] = st;
            rnode[tid] = nd;
            rsidx[tid] = si;
        }
        __syncthreads();
        sgp::f32x4 acc[NT];
        double accd[NT][4];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[t] = (sgp::f32x4){0.f, 0.f, 0.f, 0.f};
            accd[t][0] = accd[t][1] = accd[t][2] = accd[t][3] = 0.0;
        }
        load(0);
        for (int kp = 0; kp < npan; ++kp) {
#pragma unroll
            for (int q = 0; q < PRB / 8; ++q) X[(ldrow + 8 * q) * PLD + ldcol] = v[q];
            __syncthreads();
            if (kp + 1 < npan) load(kp + 1);
            // 16x16x4: A[i = lane & 15][k = lane >> 4] = X[row][k], B[k][j = lane & 15] = W[k][j]
#pragma unroll
            for (int ks = 0; ks < PKB / 4; ++ks) {
                const int k = ks * 4 + (lane >> 4);
                const float a = X[(w * 16 + (lane & 15)) * PLD + k];
                const float* wr = Wl + (int64_t)(kp * PKB + k) * HCP + (lane & 15);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[16 * t], acc[t], 0, 0, 0);
            }
            __syncthreads();
            if ((kp & 1) || kp + 1 == npan) {                // fp32 partial over at most 64 columns, then fp64
#pragma unroll
                for (int t = 0; t < NT; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) accd[t][r] += (double)acc[t][r];
                    acc[t] = (sgp::f32x4){0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        // epilogue: lane holds output column j = 16 t + (lane & 15) of rows 4 (lane >> 4) + r of the wave's 16
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = 16 * t + (lane & 15);
            if (j >= HC) continue;
            const int l = j / C, c = j - l * C;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = w * 16 + (lane >> 4) * 4 + r;
                const int st = rstep[row];
                if (st < 0) continue;
                const int64_t n = rnode[row];
                double yh = accd[t][r] + bvec[j];
                if (sc.scale) {
                    // tsl inverse_transform: x * (scale + epsilon) + bias, the sum rounded to the scaler's fp32
                    const float s1 = sc.scale[n * sc.sc_ns + c] + 5e-8f;
                    yh = yh * (double)s1 + (double)sc.bias[n * sc.sc_ns + c];
                }
                if (sc.yhat)
                    sc.yhat[(((int64_t)rsidx[row] * H + l) * n_nodes + n) * C + c] = (float)yh;
                if (sc.y) {
                    const int64_t ts = (int64_t)st + l + 1;
                    const bool m = sc.mask ? sc.mask[ts * sc.m_ss + n * sc.m_ns + c * sc.m_cs] != 0 : true;
                    if (m) {
                        const float yt = sc.y[ts * sc.y_ss + n * sc.y_ns + c];
                        const double e = yh - (double)yt;
                        sums[t][0] += fabs(e);
                        sums[t][1] += e * e;
                        sums[t][2] += fabs(e / (double)(yt + 5e-8f));   // tsl masked_mape: y + epsilon in fp32
                        sums[t][3] += 1.0;
                    }
                }
            }
        }
    }
    // fixed-order reduction of the lanes' sums: [wave][lane >> 4] in order, then one slab per workgroup
    const int grp = w * 4 + (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[((int64_t)grp * HCP + 16 * t + (lane & 15)) * 4 + q] = sums[t][q];
    __syncthreads();
    for (int e = tid; e < HCP * 4; e += 256) {
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += red[(int64_t)g * HCP * 4 + e];
        part[(int64_t)blockIdx.x * HCP * 4 + e] = s;
    }
}

// sums[l][q] = sum over workgroups, then channels, in order
__global__ void ridge_score_final_kernel(const double* __restrict__ part, int n_blocks, int hcp, int H, int C,
                                         double* __restrict__ sums) {
    const int e = threadIdx.x;
    if (e >= H * 4) return;
    const int l = e >> 2, q = e & 3;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b)
        for (int c = 0; c < C; ++c) s += part[((int64_t)b * hcp + l * C + c) * 4 + q];
    sums[e] = s;
}

// ------------------------------------------------------------------ predict + score, alpha path
// The same product for G alphas at once: W is [D][G * H * C], far too wide to keep in LDS, so its 32-row panels are
// streamed through LDS beside the X stage.  The output columns are walked in passes of TP 16-column tiles (12 VGPRs a
// tile: 4 fp32 accumulators and their 4 fp64 spills; at 8 tiles the kernel still fits the 256 registers of the two
// waves per SIMD its launch bound asks for, without scratch); a row block with
// more than one pass stages its X panels again (from L2).  The arithmetic of one output column is that of
// ridge_predict_kernel instruction for instruction: the same k per lane, the same panel order, fp32 partials over 64
// columns added in fp64, the same epilogue.  The masked sums of a (row block, pass) are reduced in a fixed order (row
// groups of a wave by shuffle, the four waves through LDS) and added into the workgroup's own slab.
constexpr int QT_MAX = 8;           // 16-column tiles per pass
constexpr int QG_MAX = 64;          // alphas
constexpr int QHC_MAX = 256;        // horizon x channels
constexpr int QJ_MAX = 4096;        // alphas x horizon x channels

// LDS row stride of a W stage: the rows k and k + 1 that the two halves of a 32-lane group read land on other banks
__host__ __device__ constexpr int path_wld(int pw) { return pw % 32 == 0 ? pw + 16 : pw; }

template <int TP>
__global__ __launch_bounds__(256, 2) void ridge_path_kernel(Segs S, const int32_t* __restrict__ steps, int64_t n_nodes,
                                                       int64_t n_steps, int64_t n_rows, const float* __restrict__ W,
                                                       const double* __restrict__ bvec, int G, int H, int C,
                                                       int npass, int npan, Score sc, double* __restrict__ part) {
    constexpr int PW = 16 * TP, WLD = path_wld(PW), WQ = PW / 8;      // WQ: W stage elements per thread
    extern __shared__ float lds[];
    float* X = lds;                                  // [PRB][PLD]
    float* Wl = X + PRB * PLD;                       // [PKB][WLD]
    double* red = reinterpret_cast<double*>(Wl + PKB * WLD);  // [4][PW][4]; both sizes above are even
    __shared__ int rstep[PRB], rnode[PRB], rsidx[PRB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int HC = H * C, J = G * HC, D = S.ncols, JP = npass * PW;

    const int ldcol = tid & (PKB - 1), ldrow = tid >> 5;     // X staging: one column, rows ldrow + 8q
    const int64_t nrb = (n_rows + PRB - 1) / PRB;
    float v[PRB / 8], wv[WQ];
    auto load = [&](int kp, int j0) {
        const ColSrc c = resolve(S, kp * PKB + ldcol, 0);
#pragma unroll
        for (int q = 0; q < PRB / 8; ++q) {
            const int row = ldrow + 8 * q;
            v[q] = fetch(c, rstep[row], rnode[row], 0.f);
        }
#pragma unroll
        for (int q = 0; q < WQ; ++q) {                       // W stage: element tid + 256 q of [PKB][PW]
            const int e = tid + 256 * q, k = kp * PKB + e / PW, j = j0 + e % PW;
            wv[q] = (k < D && j < J) ? W[(int64_t)k * J + j] : 0.f;
        }
    };

    for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        __syncthreads();                                     // previous block's epilogue done with rowinfo
        if (tid < PRB) {
            const int64_t r = rb * PRB + tid;
            int st = -1, nd = 0, si = 0;
            if (r < n_rows) {
                const int64_t s = r / n_nodes;
                nd = (int)(r - s * n_nodes);
                si = (int)s;
                st = steps[s];
            }
            rstep[tid] = st;
            rnode[tid] = nd;
            rsidx[tid] = si;
        }
        __syncthreads();
        for (int p = 0; p < npass; ++p) {
            const int j0 = p * PW;
            sgp::f32x4 acc[TP];
            double accd[TP][4];
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                acc[t] = (sgp::f32x4){0.f, 0.f, 0.f, 0.f};
                accd[t][0] = accd[t][1] = accd[t][2] = accd[t][3] = 0.0;
            }
            load(0, j0);
            for (int kp = 0; kp < npan; ++kp) {
#pragma unroll
                for (int q = 0; q < PRB / 8; ++q) X[(ldrow + 8 * q) * PLD + ldcol] = v[q];
#pragma unroll
                for (int q = 0; q < WQ; ++q) {
                    const int e = tid + 256 * q;
                    Wl[(e / PW) * WLD + e % PW] = wv[q];
                }
                __syncthreads();
                if (kp + 1 < npan) load(kp + 1, j0);
                // 16x16x4: A[i = lane & 15][k = lane >> 4] = X[row][k], B[k][j = lane & 15] = W[k][j]
#pragma unroll
                for (int ks = 0; ks < PKB / 4; ++ks) {
                    const int k = ks * 4 + (lane >> 4);
                    const float a = X[(w * 16 + (lane & 15)) * PLD + k];
                    const float* wr = Wl + k * WLD + (lane & 15);
#pragma unroll
                    for (int t = 0; t < TP; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wr[16 * t], acc[t], 0, 0, 0);
                }
                __syncthreads();
                if ((kp & 1) || kp + 1 == npan) {            // fp32 partial over at most 64 columns, then fp64
#pragma unroll
                    for (int t = 0; t < TP; ++t) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) accd[t][r] += (double)acc[t][r];
                        acc[t] = (sgp::f32x4){0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
            // epilogue: lane holds output column j = j0 + 16 t + (lane & 15) = (g H + l) C + c of rows
            // 4 (lane >> 4) + r of the wave's 16; a tile may straddle two alphas
#pragma unroll
            for (int t = 0; t < TP; ++t) {
                const int j = j0 + 16 * t + (lane & 15);
                double sums[4] = {0.0, 0.0, 0.0, 0.0};
                if (j < J) {
                    const int g = j / HC, jr = j - g * HC, l = jr / C, c = jr - l * C;
                    const double bj = bvec[j];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = w * 16 + (lane >> 4) * 4 + r;
                        const int st = rstep[row];
                        if (st < 0) continue;
                        const int64_t n = rnode[row];
                        double yh = accd[t][r] + bj;
                        if (sc.scale) {
                            // tsl inverse_transform: x * (scale + epsilon) + bias, the sum rounded to the scaler's fp32
                            const float s1 = sc.scale[n * sc.sc_ns + c] + 5e-8f;
                            yh = yh * (double)s1 + (double)sc.bias[n * sc.sc_ns + c];
                        }
                        if (sc.yhat)
                            sc.yhat[((((int64_t)g * n_steps + rsidx[row]) * H + l) * n_nodes + n) * C + c] = (float)yh;
                        if (sc.y) {
                            const int64_t ts = (int64_t)st + l + 1;
                            const bool m = sc.mask ? sc.mask[ts * sc.m_ss + n * sc.m_ns + c * sc.m_cs] != 0 : true;
                            if (m) {
                                const float yt = sc.y[ts * sc.y_ss + n * sc.y_ns + c];
                                const double e = yh - (double)yt;
                                sums[0] += fabs(e);
                                sums[1] += e * e;
                                sums[2] += fabs(e / (double)(yt + 5e-8f));   // tsl masked_mape: y + epsilon in fp32
                                sums[3] += 1.0;
                            }
                        }
                    }
                }
                if (sc.y) {                                  // the wave's four row groups, then one slot per wave
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        sums[q] += __shfl_xor(sums[q], 16);
                        sums[q] += __shfl_xor(sums[q], 32);
                        if (lane < 16) red[((w * PW) + 16 * t + lane) * 4 + q] = sums[q];
                    }
                }
            }
            if (sc.y) {
                __syncthreads();
                const bool first = rb == (int64_t)blockIdx.x;    // the workgroup's first row block stores its slab
                for (int e = tid; e < PW * 4; e += 256) {
                    const double s = ((red[e] + red[PW * 4 + e]) + red[2 * PW * 4 + e]) + red[3 * PW * 4 + e];
                    double* d = part + ((int64_t)blockIdx.x * JP + j0) * 4 + e;
                    *d = first ? s : *d + s;
                }
            }
        }
    }
}

// sums[g][l][q] += sum over workgroups, then channels, in order (the caller's sums accumulate over calls)
__global__ void ridge_path_final_kernel(const double* __restrict__ part, int n_blocks, int jp, int GH, int C,
                                        double* __restrict__ sums) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= GH * 4) return;
    const int gl = e >> 2, q = e & 3;
    double s = 0.0;
    for (int b = 0; b < n_blocks; ++b)
        for (int c = 0; c < C; ++c) s += part[((int64_t)b * jp + gl * C + c) * 4 + q];
    sums[e] += s;
}


// ------------------------------------------------------------------ host side
int parse_segs(const int64_t* segs, int32_t n_segs, Segs& S, const char* what) {
    SGP_REQUIRE(segs, "%s: null pointer (segment table)", what);
    SGP_REQUIRE(n_segs >= 1 && n_segs <= kMaxSegs, "%s: %d segments (1 .. %d)", what, (int)n_segs, kMaxSegs);
    S = Segs{};
    int64_t col = 0;
    for (int k = 0; k < n_segs; ++k) {
        const int64_t* d = segs + 6 * k;
        SGP_REQUIRE(d[0] != 0, "%s: null pointer (segment %d)", what, k);
        SGP_REQUIRE(d[1] >= 0 && d[2] >= 0 && d[3] >= 1 && d[3] <= 16384 && d[4] >= 0 && d[4] < (1 << 30) &&
                    d[5] >= 1 && d[5] <= 1024 && d[3] * d[5] <= 16384,
                    "%s: bad segment %d (strides %lld %lld, width %lld, step offset %lld, reps %lld)", what, k,
                    (long long)d[1], (long long)d[2], (long long)d[3], (long long)d[4], (long long)d[5]);
        S.s[k] = Seg{reinterpret_cast<const float*>(d[0]), d[1], d[2], (int32_t)d[3], (int32_t)d[4], (int32_t)col,
                     (int32_t)(d[3] * d[5])};
        col += d[3] * d[5];
    }
    SGP_REQUIRE(col <= 16384, "%s: %lld columns (at most 16384)", what, (long long)col);
    S.n = n_segs;
    S.ncols = (int32_t)col;
    return 0;
}

int check_rows(const int32_t* steps, int64_t n_steps, int64_t n_nodes, const char* what) {
    SGP_REQUIRE(steps, "%s: null pointer (steps)", what);
    SGP_REQUIRE(n_steps >= 1 && n_nodes >= 1 && n_nodes < (int64_t(1) << 31) && n_steps < (int64_t(1) << 31),
                "%s: bad size (%lld steps, %lld nodes)", what, (long long)n_steps, (long long)n_nodes);
    return 0;
}

int cm_slices(int64_t n_rows, int64_t& rows_per_slice) {
    int64_t p = (n_rows + 1023) / 1024;
    if (p > CM_MAX_SLICES) p = CM_MAX_SLICES;
    if (p < 1) p = 1;
    rows_per_slice = (n_rows + p - 1) / p;
    return (int)p;
}

int gram_tiles(int mp, int& nt1) {
    nt1 = (mp + GT - 1) / GT;
    return nt1 * (nt1 + 1) / 2;
}

int gram_slices(int64_t n_rows, int n_tiles, int64_t& rows_per_slice) {
    int64_t p = (GWG_TARGET + n_tiles - 1) / n_tiles;
    const int64_t chunks = (n_rows + GFLUSH - 1) / GFLUSH;
    if (p > chunks) p = chunks;
    if (p < 1) p = 1;
    p = (p + NXCD - 1) / NXCD * NXCD;                         // the XCD grouping needs a multiple of 8 slices
    rows_per_slice = ((n_rows + p - 1) / p + GKB - 1) / GKB * GKB;
    return (int)p;
}

// fp32 partials a slice of `rows` rows adds into its slab: one per GFLUSH rows, the last one short (an empty slice
// writes one zero slab)
int64_t gram_flushes(int64_t rows) {
    const int64_t nblk = (rows + GKB - 1) / GKB, per = GFLUSH / GKB;
    return nblk > 0 ? (nblk + per - 1) / per : 1;
}

// columns ridge_gram_invariant_kernel redoes: those of node stride 0 and the ones column, when rows of one step
// differ at all (n_nodes > 1) and a segment is among them (the ones column alone sums exactly)
int gram_invariant_cols(const Segs& S, int ones, int64_t n_nodes) {
    int nb = 0;
    for (int k = 0; k < S.n; ++k)
        if (S.s[k].ns == 0) nb += S.s[k].span;
    return (n_nodes > 1 && nb > 0) ? nb + ones : 0;
}

int predict_nt(int hc) { return (hc + 15) / 16; }

int predict_dpad(int ncols) { return (ncols + PKB - 1) / PKB * PKB; }

int64_t predict_lds(int dpad, int nt) {
    const int hcp = 16 * nt;
    return (int64_t)dpad * hcp * 4 + PRB * PLD * 4 + (int64_t)16 * hcp * 4 * 8;
}

// the kernel's static __shared__ (rstep, rnode, rsidx) counts against the same 160 KiB as the dynamic part
constexpr int64_t PSTATIC = 3 * PRB * 4;
bool predict_fits(int64_t lds) { return lds + PSTATIC <= 160 * 1024; }

int64_t predict_blocks(int64_t n_rows) { return (n_rows + PRB - 1) / PRB; }

int64_t predict_grid(int64_t n_rows) {
    const int64_t nrb = predict_blocks(n_rows);
    return nrb < PGRID ? nrb : PGRID;
}

// alpha path: 16-column tiles of all G x H x C columns, dealt evenly to the fewest passes of at most QT_MAX tiles
struct PathForm {
    int tiles, tp, passes, panels;
    int64_t grid, trips, lds;
};

int path_form(int64_t n_rows, int n_cols, int n_out, int n_alphas, PathForm& f, const char* what) {
    SGP_REQUIRE(n_rows >= 1 && n_cols >= 1 && n_cols <= 16384, "%s: bad size (%lld rows, %d columns)", what,
                (long long)n_rows, (int)n_cols);
    SGP_REQUIRE(n_alphas >= 1 && n_alphas <= QG_MAX, "%s: %d alphas (1 .. %d)", what, (int)n_alphas, QG_MAX);
    SGP_REQUIRE(n_out >= 1 && n_out <= QHC_MAX, "%s: horizon x channels must be 1 .. %d", what, QHC_MAX);
    SGP_REQUIRE((int64_t)n_alphas * n_out <= QJ_MAX, "%s: %d alphas x %d outputs (at most %d columns of W)", what,
                (int)n_alphas, (int)n_out, QJ_MAX);
    f.tiles = (n_alphas * n_out + 15) / 16;
    f.passes = (f.tiles + QT_MAX - 1) / QT_MAX;
    f.tp = (f.tiles + f.passes - 1) / f.passes;
    f.panels = predict_dpad(n_cols) / PKB;
    f.grid = predict_grid(n_rows);
    f.trips = (predict_blocks(n_rows) + f.grid - 1) / f.grid;
    const int pw = 16 * f.tp;
    f.lds = (int64_t)PRB * PLD * 4 + (int64_t)PKB * path_wld(pw) * 4 + (int64_t)4 * pw * 4 * 8;
    return 0;
}

int64_t path_work_bytes(const PathForm& f) { return f.grid * f.passes * f.tp * 16 * 4 * 8; }

}  // namespace

extern "C" {

int64_t sgp_ridge_workspace_bytes(int32_t which, int64_t n_rows, int32_t n_cols, int32_t n_out) {
    if (n_rows < 1 || n_cols < 1 || n_cols > 16385) return -1;
    int64_t rps;
    if (which == 0) return (int64_t)cm_slices(n_rows, rps) * n_cols * 8;
    if (which == 1) {
        int nt1;
        const int nt = gram_tiles(n_cols, nt1);
        return (int64_t)gram_slices(n_rows, nt, rps) * nt * GTILE * 8;
    }
    if (which == 2 && n_out >= 1 && n_out <= 64) return predict_grid(n_rows) * 16 * predict_nt(n_out) * 4 * 8;
    return -1;
}

int sgp_ridge_form(int32_t which, int64_t n_rows, int32_t n_cols, int32_t n_out, int64_t* out) {
    const char* what = "sgp_ridge_form";
    SGP_REQUIRE(out, "%s: null pointer", what);
    SGP_REQUIRE(which >= 0 && which <= 2, "%s: which must be 0, 1 or 2", what);
    // the entries' own limits: 16384 segment columns (the Gram's count includes its ones column), 2^31 steps x nodes
    SGP_REQUIRE(n_rows >= 1 && n_cols >= 1 && n_cols <= 16384 + (which == 1), "%s: bad size (%lld rows, %d columns)",
                what, (long long)n_rows, (int)n_cols);
    int64_t rps;
    if (which == 0) {
        out[0] = cm_slices(n_rows, rps);
        out[1] = rps;
        return 0;
    }
    if (which == 1) {
        int nt1;
        const int nt = gram_tiles(n_cols, nt1);
        out[2] = gram_slices(n_rows, nt, rps);
        out[0] = nt1;
        out[1] = nt;
        out[3] = rps;
        out[4] = gram_flushes(rps < n_rows ? rps : n_rows);          // slice 0 is never shorter than another
        return 0;
    }
    SGP_REQUIRE(n_out >= 1 && n_out <= 64, "%s: horizon x channels must be 1 .. 64", what);
    const int nt = predict_nt(n_out), dpad = predict_dpad(n_cols);
    const int64_t lds = predict_lds(dpad, nt), grid = predict_grid(n_rows);
    out[0] = nt;
    out[1] = grid;
    out[2] = (predict_blocks(n_rows) + grid - 1) / grid;
    out[3] = dpad / PKB;
    out[4] = lds;
    if (!predict_fits(lds))
        return sgp::fail(SGP_EUNSUP, "%s: %d features x %d outputs need %lld bytes of LDS (at most 160 KiB)", what,
                         (int)n_cols, (int)n_out, (long long)lds);
    return 0;
}

int sgp_ridge_colmeans_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps,
                           int64_t n_nodes, double* means, void* work, int64_t work_bytes, sgp_stream_t stream) {
    const char* what = "sgp_ridge_colmeans_f32";
    Segs S;
    if (int rc = parse_segs(segs, n_segs, S, what)) return rc;
    if (int rc = check_rows(steps, n_steps, n_nodes, what)) return rc;
    SGP_REQUIRE(means && work, "%s: null pointer", what);
    const int64_t n_rows = n_steps * n_nodes;
    int64_t rps;
    const int p = cm_slices(n_rows, rps);
    SGP_REQUIRE(work_bytes >= (int64_t)p * S.ncols * 8, "%s: workspace of %lld bytes is too small", what,
                (long long)work_bytes);
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(work);
    hipLaunchKernelGGL(ridge_colsum_kernel, dim3((S.ncols + 255) / 256, p), dim3(256), 0, st, S, steps, n_nodes,
                       n_rows, rps, part);
    if (int rc = sgp::check_launch(what)) return rc;
    hipLaunchKernelGGL(ridge_colmean_final_kernel, dim3((S.ncols + 255) / 256), dim3(256), 0, st, part, p, S.ncols,
                       n_rows, means);
    return sgp::check_launch(what);
}

int sgp_ridge_gram_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps, int64_t n_nodes,
                       const float* shift, int32_t ones, double* gram, int64_t ldg, void* work, int64_t work_bytes,
                       sgp_stream_t stream) {
    const char* what = "sgp_ridge_gram_f32";
    Segs S;
    if (int rc = parse_segs(segs, n_segs, S, what)) return rc;
    if (int rc = check_rows(steps, n_steps, n_nodes, what)) return rc;
    SGP_REQUIRE(gram && work, "%s: null pointer", what);
    SGP_REQUIRE(ones == 0 || ones == 1, "%s: ones must be 0 or 1", what);
    const int mp = S.ncols + ones;
    SGP_REQUIRE(ldg >= mp, "%s: ldg %lld < %d columns", what, (long long)ldg, mp);
    const int64_t n_rows = n_steps * n_nodes;
    int nt1;
    const int nt = gram_tiles(mp, nt1);
    int64_t rps;
    const int p = gram_slices(n_rows, nt, rps);
    SGP_REQUIRE(work_bytes >= (int64_t)p * nt * GTILE * 8, "%s: workspace of %lld bytes is too small", what,
                (long long)work_bytes);
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(work);
    hipLaunchKernelGGL(ridge_gram_kernel, dim3(p * nt), dim3(256), 0, st, S, steps, n_nodes, n_rows, shift, ones, nt1,
                       nt, rps, part);
    if (int rc = sgp::check_launch(what)) return rc;
    const int64_t n_el = (int64_t)nt * GTILE;
    hipLaunchKernelGGL(ridge_gram_reduce_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, st, part, p, nt,
                       nt1, mp, gram, ldg);
    if (int rc = sgp::check_launch(what)) return rc;
    const int nb = gram_invariant_cols(S, ones, n_nodes);
    if (nb == 0) return 0;
    hipLaunchKernelGGL(ridge_gram_invariant_kernel, dim3((unsigned)((int64_t)nb * nb)), dim3(256), 0, st, S, steps,
                       n_steps, n_nodes, shift, ones, nb, gram, ldg);
    return sgp::check_launch(what);
}

int sgp_ridge_predict_score_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps,
                                int64_t n_nodes, const float* W, const double* b, int32_t horizon, int32_t channels,
                                const float* scale, const float* bias, int64_t sc_node_stride,
                                const float* y, int64_t y_ss, int64_t y_ns,
                                const uint8_t* mask, int64_t m_ss, int64_t m_ns, int64_t m_cs,
                                float* yhat, double* sums, void* work, int64_t work_bytes, sgp_stream_t stream) {
    const char* what = "sgp_ridge_predict_score_f32";
    Segs S;
    if (int rc = parse_segs(segs, n_segs, S, what)) return rc;
    if (int rc = check_rows(steps, n_steps, n_nodes, what)) return rc;
    SGP_REQUIRE(W && b && work, "%s: null pointer", what);
    SGP_REQUIRE((scale == nullptr) == (bias == nullptr), "%s: scale and bias go together", what);
    SGP_REQUIRE((y == nullptr) == (sums == nullptr), "%s: y and sums go together", what);
    SGP_REQUIRE(y || yhat, "%s: nothing to compute (no y and no yhat)", what);
    SGP_REQUIRE(horizon >= 1 && channels >= 1 && (int64_t)horizon * channels <= 64,
                "%s: horizon x channels must be 1 .. 64", what);
    SGP_REQUIRE(sc_node_stride >= 0 && y_ss >= 0 && y_ns >= 0 && m_ss >= 0 && m_ns >= 0 && m_cs >= 0,
                "%s: negative stride", what);
    const int hc = horizon * channels, nt = predict_nt(hc);
    const int dpad = predict_dpad(S.ncols);
    const int64_t lds = predict_lds(dpad, nt);
    if (!predict_fits(lds))
        return sgp::fail(SGP_EUNSUP, "%s: %d features x %d outputs need %lld bytes of LDS (at most 160 KiB)", what,
                         S.ncols, hc, (long long)lds);
    const int64_t n_rows = n_steps * n_nodes;
    const int64_t grid = predict_grid(n_rows);
    SGP_REQUIRE(work_bytes >= grid * 16 * nt * 4 * 8, "%s: workspace of %lld bytes is too small", what,
                (long long)work_bytes);
    Score sc{scale, bias, sc_node_stride, y, y_ss, y_ns, mask, m_ss, m_ns, m_cs, yhat};
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(work);
    const void* kern = nt == 1 ? (const void*)ridge_predict_kernel<1> : nt == 2 ? (const void*)ridge_predict_kernel<2>
                     : nt == 3 ? (const void*)ridge_predict_kernel<3> : (const void*)ridge_predict_kernel<4>;
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return sgp::fail((int)e, "%s: %s", what, hipGetErrorString(e));
#define SGP_RIDGE_LAUNCH(NT)                                                                                           \
    hipLaunchKernelGGL(ridge_predict_kernel<NT>, dim3((unsigned)grid), dim3(256), (size_t)lds, st, S, steps, n_nodes, \
                       n_rows, W, b, (int)horizon, (int)channels, dpad, sc, part)
    if (nt == 1) SGP_RIDGE_LAUNCH(1);
    else if (nt == 2) SGP_RIDGE_LAUNCH(2);
    else if (nt == 3) SGP_RIDGE_LAUNCH(3);
    else SGP_RIDGE_LAUNCH(4);
#undef SGP_RIDGE_LAUNCH
    if (int rc = sgp::check_launch(what)) return rc;
    if (!sums) return 0;
    hipLaunchKernelGGL(ridge_score_final_kernel, dim3(1), dim3(256), 0, st, part, (int)grid, 16 * nt, (int)horizon,
                       (int)channels, sums);
    return sgp::check_launch(what);
}

int64_t sgp_ridge_path_workspace_bytes(int64_t n_rows, int32_t n_cols, int32_t n_out, int32_t n_alphas) {
    PathForm f;
    if (path_form(n_rows, n_cols, n_out, n_alphas, f, "sgp_ridge_path_workspace_bytes")) return -1;
    return path_work_bytes(f);
}

int sgp_ridge_path_form(int64_t n_rows, int32_t n_cols, int32_t n_out, int32_t n_alphas, int64_t* out) {
    const char* what = "sgp_ridge_path_form";
    SGP_REQUIRE(out, "%s: null pointer", what);
    PathForm f;
    if (int rc = path_form(n_rows, n_cols, n_out, n_alphas, f, what)) return rc;
    out[0] = f.tiles;
    out[1] = f.tp;
    out[2] = f.passes;
    out[3] = f.grid;
    out[4] = f.trips;
    out[5] = f.panels;
    out[6] = f.lds;
    return 0;
}

int sgp_ridge_predict_score_path_f32(const int64_t* segs, int32_t n_segs, const int32_t* steps, int64_t n_steps,
                                     int64_t n_nodes, const float* W, const double* b, int32_t n_alphas,
                                     int32_t horizon, int32_t channels,
                                     const float* scale, const float* bias, int64_t sc_node_stride,
                                     const float* y, int64_t y_ss, int64_t y_ns,
                                     const uint8_t* mask, int64_t m_ss, int64_t m_ns, int64_t m_cs,
                                     float* yhat, double* sums, void* work, int64_t work_bytes, sgp_stream_t stream) {
    const char* what = "sgp_ridge_predict_score_path_f32";
    Segs S;
    if (int rc = parse_segs(segs, n_segs, S, what)) return rc;
    if (int rc = check_rows(steps, n_steps, n_nodes, what)) return rc;
    SGP_REQUIRE(W && b && work, "%s: null pointer", what);
    SGP_REQUIRE((scale == nullptr) == (bias == nullptr), "%s: scale and bias go together", what);
    SGP_REQUIRE((y == nullptr) == (sums == nullptr), "%s: y and sums go together", what);
    SGP_REQUIRE(y || yhat, "%s: nothing to compute (no y and no yhat)", what);
    SGP_REQUIRE(horizon >= 1 && channels >= 1 && (int64_t)horizon * channels <= QHC_MAX,
                "%s: horizon x channels must be 1 .. %d", what, QHC_MAX);
    SGP_REQUIRE(sc_node_stride >= 0 && y_ss >= 0 && y_ns >= 0 && m_ss >= 0 && m_ns >= 0 && m_cs >= 0,
                "%s: negative stride", what);
    const int64_t n_rows = n_steps * n_nodes;
    PathForm f;
    if (int rc = path_form(n_rows, S.ncols, horizon * channels, n_alphas, f, what)) return rc;
    SGP_REQUIRE(work_bytes >= path_work_bytes(f), "%s: workspace of %lld bytes is too small", what,
                (long long)work_bytes);
    Score sc{scale, bias, sc_node_stride, y, y_ss, y_ns, mask, m_ss, m_ns, m_cs, yhat};
    hipStream_t st = (hipStream_t)stream;
    double* part = static_cast<double*>(work);
#define SGP_RIDGE_PATH_LAUNCH(TP)                                                                                      \
    case TP:                                                                                                           \
        hipLaunchKernelGGL(ridge_path_kernel<TP>, dim3((unsigned)f.grid), dim3(256), (size_t)f.lds, st, S, steps,     \
                           n_nodes, n_steps, n_rows, W, b, (int)n_alphas, (int)horizon, (int)channels, f.passes,      \
                           f.panels, sc, part);                                                                        \
        break
    switch (f.tp) {
        SGP_RIDGE_PATH_LAUNCH(1);
        SGP_RIDGE_PATH_LAUNCH(2);
        SGP_RIDGE_PATH_LAUNCH(3);
        SGP_RIDGE_PATH_LAUNCH(4);
        SGP_RIDGE_PATH_LAUNCH(5);
        SGP_RIDGE_PATH_LAUNCH(6);
        SGP_RIDGE_PATH_LAUNCH(7);
        default: SGP_RIDGE_PATH_LAUNCH(8);
    }
#undef SGP_RIDGE_PATH_LAUNCH
    if (int rc = sgp::check_launch(what)) return rc;
    if (!sums) return 0;
    const int gh = n_alphas * horizon;
    hipLaunchKernelGGL(ridge_path_final_kernel, dim3((unsigned)((gh * 4 + 255) / 256)), dim3(256), 0, st, part,
                       (int)f.grid, f.passes * f.tp * 16, gh, (int)channels, sums);
    return sgp::check_launch(what);
}

}  // extern "C"
