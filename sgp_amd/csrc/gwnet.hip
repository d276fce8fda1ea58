// Graph WaveNet baseline (`--model-name gwnet`, tsl/nn/models/stgn/graph_wavenet_model.py, lib/nn/models/gwnet_model.py):
// what the model needs beyond the DiffConv hop of dcrnn.hip and the dense kernels of decoder_mlp.hip.  Activations are
// time-major [S, M, H] with M = b n, so tap j of the temporal convolution is the row offset j d M and the residual
// res[:, -S:] a contiguous suffix.
//
//   sgp_gwnet_tconv_f32       gated dilated temporal convolution: [a | g] = sum_j W_j x[r + j d M] + bias, y = tanh(a) *
//                             sigmoid(g).  The stage loop of dense_tile.h with the taps as extra k chunks; column c of a
//                             and of g sit in the same lane and register, so the gate is lane-local.
//   sgp_gwnet_tconv_bwd_f32   dz = [dy s (1 - t^2) | dy t s (1 - s)] over the saved [tanh a | sigmoid g]; the products of
//                             the backward pass are sgp_dense_f32 / sgp_dense_wgrad_f32 per tap.
//   sgp_adj_apply_f32         Y[i] (+)= A X[i] (or A^T X[i]) for a dense shared [n, n] operator: a workgroup owns 64 or
//                             128 destination rows x 128 (item, feature) columns; the X tile of a k stage goes through
//                             LDS once and serves all waves, a wave's A piece stays in registers for all columns.
//   sgp_adj_grad_f32          dA (+)= sum_i dY[i] X[i]^T: one wave per 64 x 64 tile, the items in order; for a small
//                             operator the items are split into slices with one partial each, added in order in fp64.
//   sgp_row_softmax_f32 / _bwd_f32   rows of softmax(L) with the max subtracted; dL = A (dA - <dA, A>) [L > 0].
//   sgp_gwnet_norm_f32 / _bwd_f32    z = dropout(y) + res, then batch / layer normalisation (or none); column sums in
//                             fp64 over row slices added in slice order.
//
// Exact fp32 products (v_mfma_f32_16x16x4_f32), no float atomics, every sum has one fixed order.
#include "common.h"
#include "decoder_ops.h"
#include "dense_tile.h"
#include "wg.h"

namespace {
using sgp::f32x4;
using sgp::grid_for;
using sgp::sigmoid_f32;
using namespace sgp_dense;

const char* domain_error(int H, int Kt) {
    if (H < 16 || H > 128 || H % 16 != 0) return "hidden size must be a multiple of 16 in 16 .. 128";
    if (Kt < 1 || Kt > 4) return "temporal kernel size must lie in 1 .. 4";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------- temporal conv
struct TcArgs {
    const float* x; long long xrs, tap_rows;      // tap j reads row r + j * tap_rows (tap_rows = d M)
    const float* wp; const float* bias;           // sgp_dense_pack_f32 of [2 H, Kt H] (tap-major), bias [2 H]
    float* y; long long yrs;
    float* act; long long ars;                    // [tanh a | sigmoid g], or null
    long long n_rows; int H, Kt;
};

// 64 rows x 32 columns of y per workgroup: LDS tiles 0, 1 are the a half's column tiles ct0, ct0 + 1, tiles 2, 3 the g
// half's, so acc[0][c] and acc[0][c + 2] hold the same (row, column) of a and g.
__global__ __launch_bounds__(256) void tconv_kernel(TcArgs a) {
    __shared__ f32x4 wl[DT_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & 15, q = lane >> 4;
    const int HT = a.H / 16, KB = a.Kt * HT;
    const int ct0 = blockIdx.y * 2;
    const long long row = (long long)blockIdx.x * 64 + wave * 16 + b;
    const bool ok = row < a.n_rows;
    const float* xp = a.x + (ok ? row : 0) * a.xrs;
    f32x4 acc[1][DT_TILES];
    dense_tile_loop<1>(
        wl, a.wp, KB,
        [xp, ok, q, HT, KB, tap_rows = a.tap_rows, xrs = a.xrs](int, int kb) {
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok && kb < KB) {
                const int tap = kb / HT, col = 16 * (kb % HT) + 4 * q;
                v = *reinterpret_cast<const f32x4*>(xp + (long long)tap * tap_rows * xrs + col);
            }
            return v;
        },
        [ct0, HT](int c) {
            const int ct = ct0 + (c & 1);
            return ct < HT ? (c >> 1) * HT + ct : -1;
        },
        acc);
    if (!ok) return;
    // D[col, row]: lane (q, b), register r -> column 16 ct + 4 q + r of row b
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int ct = ct0 + c;
        if (ct >= HT) continue;
        const int col0 = 16 * ct + 4 * q;
        f32x4 tv, sv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            tv[r] = sgp_res::tanh_f32(acc[0][c][r] + a.bias[col0 + r]);
            sv[r] = sigmoid_f32(acc[0][c + 2][r] + a.bias[a.H + col0 + r]);
        }
        *reinterpret_cast<f32x4*>(a.y + row * a.yrs + col0) = tv * sv;
        if (a.act) {
            *reinterpret_cast<f32x4*>(a.act + row * a.ars + col0) = tv;
            *reinterpret_cast<f32x4*>(a.act + row * a.ars + a.H + col0) = sv;
        }
    }
}

__global__ void tconv_bwd_kernel(const float* __restrict__ dy, long long dyrs, float* act, long long ars,
                                 long long total, int H) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / H;
    const int col = (int)(i % H);
    float* p = act + row * ars;
    const float d = dy[row * dyrs + col], t = p[col], s = p[H + col];
    p[col] = d * s * (1.f - t * t);
    p[H + col] = d * t * s * (1.f - s);
}

// ---------------------------------------------------------------------------------------------------- dense operator
struct AdjArgs {
    const float* A; long long ars; int transpose;
    const float* x; long long xrs, xbs;           // the column offsets are folded into the pointers
    float* y; long long yrs, ybs;
    int n, batch, F, accumulate;
    bool avec;                                    // A rows may be read 16 bytes at a time
};

constexpr int AJ_CT = 8;                          // 16-column chunks of (item, feature) per workgroup
constexpr int AJ_KC = 32;                         // source rows v per LDS stage
constexpr int AJ_LS = AJ_CT * 16 + 4;             // LDS row stride in floats: rows 4 q apart fall into different banks

template <int WT>                                 // 16-row tiles of destination rows per wave
__global__ __launch_bounds__(256) void adj_apply_kernel(AdjArgs a) {
    __shared__ float xl[AJ_KC * AJ_LS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & 15, q = lane >> 4;
    const int FT = a.F / 16;
    const long long chunks = (long long)a.batch * FT;
    const long long cc0 = (long long)blockIdx.y * AJ_CT;
    const int w_base = blockIdx.x * (64 * WT) + wave * (16 * WT);
    // loader role: thread -> one 16-byte piece of the 128 columns, rows lv, lv + 8, ..
    const int lc4 = threadIdx.x & 31, lv = threadIdx.x >> 5;
    const long long lchunk = cc0 + (lc4 >> 2);
    const bool lok = lchunk < chunks;
    const float* lx = lok ? a.x + (lchunk / FT) * a.xbs + 16 * (lchunk % FT) + 4 * (lc4 & 3) : a.x;
    f32x4 xr[4], ar[WT][2], cur[WT][2];
    f32x4 acc[WT][AJ_CT];
#pragma unroll
    for (int t = 0; t < WT; ++t)
#pragma unroll
        for (int c = 0; c < AJ_CT; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int v = k0 + lv + 8 * i;
            xr[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (lok && v < a.n) xr[i] = *reinterpret_cast<const f32x4*>(lx + (long long)v * a.xrs);
        }
#pragma unroll
        for (int t = 0; t < WT; ++t) {
            const int w = w_base + 16 * t + b;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int vv = k0 + 16 * ks + 4 * q;
                f32x4 v4 = f32x4{0.f, 0.f, 0.f, 0.f};
                if (w < a.n) {
                    if (!a.transpose) {
                        const float* p = a.A + (long long)w * a.ars + vv;
                        if (a.avec && vv + 3 < a.n) v4 = *reinterpret_cast<const f32x4*>(p);
                        else {
#pragma unroll
                            for (int s = 0; s < 4; ++s)
                                if (vv + s < a.n) v4[s] = p[s];
                        }
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            if (vv + s < a.n) v4[s] = a.A[(long long)(vv + s) * a.ars + w];
                    }
                }
                ar[t][ks] = v4;
            }
        }
    };

    load(0);
    for (int k0 = 0; k0 < a.n; k0 += AJ_KC) {
        __syncthreads();                                             // previous stage fully consumed
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(&xl[(lv + 8 * i) * AJ_LS + 4 * lc4]) = xr[i];
#pragma unroll
        for (int t = 0; t < WT; ++t) { cur[t][0] = ar[t][0]; cur[t][1] = ar[t][1]; }
        __syncthreads();
        if (k0 + AJ_KC < a.n) load(k0 + AJ_KC);                      // in flight while this stage computes
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* xrow = &xl[(16 * ks + 4 * q + s) * AJ_LS + b];
#pragma unroll
                for (int c = 0; c < AJ_CT; ++c) {
                    const float xa = xrow[16 * c];
#pragma unroll
                    for (int t = 0; t < WT; ++t)
                        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, cur[t][ks][s], acc[t][c], 0, 0, 0);
                }
            }
    }
    // D[feature, row]: lane (q, b), register r -> feature 4 q + r of the chunk, destination row 16 t + b
#pragma unroll
    for (int t = 0; t < WT; ++t) {
        const int w = w_base + 16 * t + b;
        if (w >= a.n) continue;
#pragma unroll
        for (int c = 0; c < AJ_CT; ++c) {
            const long long chunk = cc0 + c;
            if (chunk >= chunks) continue;
            float* p = a.y + (chunk / FT) * a.ybs + (long long)w * a.yrs + 16 * (chunk % FT) + 4 * q;
            f32x4 v = acc[t][c];
            if (a.accumulate) v += *reinterpret_cast<const f32x4*>(p);
            *reinterpret_cast<f32x4*>(p) = v;
        }
    }
}

struct AgArgs {
    const float* dy; long long dyrs, dybs;
    const float* x; long long xrs, xbs;
    float* out; long long ors, slice_stride;      // dA itself (one slice) or the partials [slices, n, n]
    int n, batch, F, items_per_slice, accumulate;
};

// one wave = 64 destination rows w x 64 source rows v; the contraction runs over (item, feature) in order
__global__ __launch_bounds__(256) void adj_grad_kernel(AgArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int wt = blockIdx.x * 2 + (wave >> 1), vt = blockIdx.y * 2 + (wave & 1);
    if (64 * wt >= a.n || 64 * vt >= a.n) return;                     // wave-uniform; the kernel has no barrier
    const int slice = blockIdx.z;
    const int i0 = slice * a.items_per_slice, i1 = min(a.batch, i0 + a.items_per_slice);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
        const float* dyi = a.dy + (long long)i * a.dybs + 4 * q;
        const float* xi = a.x + (long long)i * a.xbs + 4 * q;
        for (int f0 = 0; f0 < a.F; f0 += 16) {
            f32x4 av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int w = 64 * wt + 16 * t + c, v = 64 * vt + 16 * t + c;
                av[t] = bv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (w < a.n) av[t] = *reinterpret_cast<const f32x4*>(dyi + (long long)w * a.dyrs + f0);
                if (v < a.n) bv[t] = *reinterpret_cast<const f32x4*>(xi + (long long)v * a.xrs + f0);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int to = 0; to < 4; ++to)
#pragma unroll
                    for (int ti = 0; ti < 4; ++ti)
                        acc[to][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[to][s], bv[ti][s], acc[to][ti], 0, 0, 0);
        }
    }
    // D: lane (q, c), register r -> w = 64 wt + 16 to + 4 q + r, v = 64 vt + 16 ti + c
    float* o = a.out + (long long)slice * a.slice_stride;
#pragma unroll
    for (int to = 0; to < 4; ++to)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int w = 64 * wt + 16 * to + 4 * q + r;
            if (w >= a.n) continue;
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
                const int v = 64 * vt + 16 * ti + c;
                if (v >= a.n) continue;
                float* p = o + (long long)w * a.ors + v;
                float val = acc[to][ti][r];
                if (a.accumulate) val += *p;
                *p = val;
            }
        }
}

__global__ void adj_grad_reduce(const float* __restrict__ part, int slices, int n, float* dA, long long ars, int accumulate) {
    const long long total = (long long)n * n;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        double sum = 0.0;
        for (int s = 0; s < slices; ++s) sum += (double)part[s * total + e];
        float* p = dA + (e / n) * ars + (e % n);
        *p = accumulate ? (float)((double)*p + sum) : (float)sum;
    }
}

// slices of the items: enough 64 x 64 waves to fill the chip
void adj_grad_slices(int n, int batch, int& ips, int& slices) {
    const long long t = (n + 63) / 64, tiles = t * t;
    long long want = 1024 / tiles;
    if (want < 1) want = 1;
    if (want > batch) want = batch;
    ips = (int)((batch + want - 1) / want);
    slices = (batch + ips - 1) / ips;
}

// ---------------------------------------------------------------------------------------------------- softmax
constexpr int SM_T = 256;

__device__ __forceinline__ double block_sum(double v, double* sh) {
    return sgp::wg_reduce<SM_T>(v, sh, [](double a, double b) { return a + b; });
}

__global__ __launch_bounds__(SM_T) void row_softmax_kernel(const float* __restrict__ L, long long lrs, float* A,
                                                           long long ars, int n) {
    __shared__ double sh[SM_T];
    __shared__ float mx[SM_T];
    const float* l = L + (long long)blockIdx.x * lrs;
    float* o = A + (long long)blockIdx.x * ars;
    float m = -INFINITY;
    for (int j = threadIdx.x; j < n; j += SM_T) m = fmaxf(m, l[j]);
    m = sgp::wg_reduce<SM_T>(m, mx, [](float a, float b) { return fmaxf(a, b); });
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += SM_T) s += (double)expf(l[j] - m);
    const float tot = (float)block_sum(s, sh);
    for (int j = threadIdx.x; j < n; j += SM_T) o[j] = expf(l[j] - m) / tot;
}

__global__ __launch_bounds__(SM_T) void row_softmax_bwd_kernel(const float* __restrict__ A, long long ars,
                                                               const float* dA, long long drs,
                                                               const float* __restrict__ L, long long lrs,
                                                               float* dL, long long ors, int n) {
    __shared__ double sh[SM_T];
    const float* p = A + (long long)blockIdx.x * ars;
    const float* g = dA + (long long)blockIdx.x * drs;
    const float* l = L + (long long)blockIdx.x * lrs;
    float* o = dL + (long long)blockIdx.x * ors;
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += SM_T) s += (double)g[j] * (double)p[j];
    const float dot = (float)block_sum(s, sh);
    for (int j = threadIdx.x; j < n; j += SM_T) o[j] = l[j] > 0.f ? p[j] * (g[j] - dot) : 0.f;
}

// ---------------------------------------------------------------------------------------------------- norm
struct NmArgs {
    const float* y; long long yrs;                // fwd: the block's spatial output; bwd: d out
    const float* res; long long rrs;              // fwd: residual tail or null
    const float* z; const float* stats;           // bwd: saved z [R, H]; batch: mean | rstd | mean_lo [3 H]; layer: (mean, inv) [R, 2]
    const float* w; const float* bias;
    float* zs;                                    // fwd: z [R, H] to save, or null
    float* out; long long ors;                    // fwd: the normalised rows; bwd: d y
    float* out2; long long o2rs;                  // bwd: d res, or null
    double* part; const double* cm;               // column partials [slices, 2, H]; bwd: column means [2 H]
    float* st_out;                                // fwd: stats to write
    long long R; int H, kind, rows_per_slice, layer_stats, train;
    unsigned thresh, k0, k1; float scale;
};

__device__ __forceinline__ float nm_z(const NmArgs& a, long long row, int col) {
    float v = a.y[row * a.yrs + col] *
              keep_factor((unsigned long long)(row * a.H + col), a.thresh, a.k0, a.k1, a.scale);
    if (a.res) v += a.res[row * a.rrs + col];
    return v;
}

// per-slice column sums in fp64: FWD (z, z^2), BWD (d out, d out * xhat); thread (row lane rs, column col)
template <int BWD>
__global__ __launch_bounds__(256) void norm_colsum_kernel(NmArgs a) {
    __shared__ double sh[2][256];
    const int rl = 256 / a.H;
    const int col = threadIdx.x % a.H, rs = threadIdx.x / a.H;
    const long long r0 = (long long)blockIdx.x * a.rows_per_slice;
    const long long r1 = min(a.R, r0 + a.rows_per_slice);
    double s1 = 0.0, s2 = 0.0;
    if (rs < rl) {
        for (long long row = r0 + rs; row < r1; row += rl) {
            if (!BWD) {
                const double z = (double)nm_z(a, row, col);
                s1 += z; s2 += z * z;
            } else {
                const float d = a.y[row * a.yrs + col], z = a.z[row * a.H + col];
                const float xh = a.layer_stats ? (z - a.stats[2 * row]) * a.stats[2 * row + 1]
                                               : ((z - a.stats[col]) - a.stats[2 * a.H + col]) * a.stats[a.H + col];
                s1 += (double)d; s2 += (double)d * (double)xh;
            }
        }
    }
    sh[0][threadIdx.x] = s1; sh[1][threadIdx.x] = s2;
    __syncthreads();
    if ((int)threadIdx.x < a.H) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < rl; ++k) { t1 += sh[0][k * a.H + col]; t2 += sh[1][k * a.H + col]; }
        a.part[((long long)blockIdx.x * 2) * a.H + col] = t1;
        a.part[((long long)blockIdx.x * 2 + 1) * a.H + col] = t2;
    }
}

// slices added in slice order.  FWD: mean, rstd of the biased variance, and the running buffers (unbiased variance).
__global__ void norm_finalize_fwd(const double* part, int slices, long long R, int H, double eps, double momentum,
                                  float* st, float* rmean, float* rvar) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= H) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < slices; ++s) { s1 += part[((long long)s * 2) * H + col]; s2 += part[((long long)s * 2 + 1) * H + col]; }
    const double mean = s1 / (double)R;
    double var = s2 / (double)R - mean * mean;
    if (var < 0.0) var = 0.0;
    st[col] = (float)mean;                                            // mean = hi + lo: z - hi is exact near the mean
    st[2 * H + col] = (float)(mean - (double)(float)mean);
    st[H + col] = (float)(1.0 / sqrt(var + eps));
    if (rmean) rmean[col] = (float)((1.0 - momentum) * (double)rmean[col] + momentum * mean);
    if (rvar) rvar[col] = (float)((1.0 - momentum) * (double)rvar[col] + momentum * var * ((double)R / (double)(R - 1)));
}

__global__ void norm_stats_eval(const float* rmean, const float* rvar, int H, double eps, float* st) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= H) return;
    st[col] = rmean[col];
    st[2 * H + col] = 0.f;
    st[H + col] = (float)(1.0 / sqrt((double)rvar[col] + eps));
}

__global__ void norm_finalize_bwd(const double* part, int slices, long long R, int H, double* cm, float* dw, float* db) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= H) return;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < slices; ++s) { s1 += part[((long long)s * 2) * H + col]; s2 += part[((long long)s * 2 + 1) * H + col]; }
    cm[col] = s1 / (double)R;
    cm[H + col] = s2 / (double)R;
    if (db) db[col] = (float)s1;
    if (dw) dw[col] = (float)s2;
}

// kind 0 (none) and 1 (batch), one thread per element
__global__ void norm_apply_fwd(NmArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R * a.H) return;
    const long long row = i / a.H;
    const int col = (int)(i % a.H);
    const float z = nm_z(a, row, col);
    if (a.zs) a.zs[i] = z;
    float v = z;
    if (a.kind == 1) v = ((z - a.stats[col]) - a.stats[2 * a.H + col]) * a.stats[a.H + col] * a.w[col] + a.bias[col];
    a.out[row * a.ors + col] = v;
}

__global__ void norm_apply_bwd(NmArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R * a.H) return;
    const long long row = i / a.H;
    const int col = (int)(i % a.H);
    float dz = a.y[row * a.yrs + col];
    if (a.kind == 1) {
        const float rstd = a.stats[a.H + col];
        if (a.train) {
            const float xh = ((a.z[i] - a.stats[col]) - a.stats[2 * a.H + col]) * rstd;
            dz = rstd * a.w[col] * (dz - (float)a.cm[col] - xh * (float)a.cm[a.H + col]);
        } else {
            dz = dz * a.w[col] * rstd;
        }
    }
    a.out[row * a.ors + col] = dz * keep_factor((unsigned long long)i, a.thresh, a.k0, a.k1, a.scale);
    if (a.out2) a.out2[row * a.o2rs + col] = dz;
}

// butterfly: every lane gets the sum (the rows below need it in all of them)
__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// kind 2 (layer): one wave per row, H <= 256; (x - mean) / (std + eps) with the population std
template <int BWD>
__global__ __launch_bounds__(256) void norm_layer_kernel(NmArgs a, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.R) return;                                           // wave-uniform
    float v[4], g[4];
    if (!BWD) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = lane + 64 * k;
            v[k] = col < a.H ? nm_z(a, row, col) : 0.f;
            s += v[k];
        }
        const float mean = wave_sum_all(s) / (float)a.H;
        float ss = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = lane + 64 * k;
            if (col < a.H) { const float u = v[k] - mean; ss += u * u; }
        }
        const float inv = 1.f / (sqrtf(wave_sum_all(ss) / (float)a.H) + eps);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = lane + 64 * k;
            if (col >= a.H) continue;
            if (a.zs) a.zs[row * a.H + col] = v[k];
            a.out[row * a.ors + col] = (v[k] - mean) * inv * a.w[col] + a.bias[col];
        }
        if (a.st_out && lane == 0) { a.st_out[2 * row] = mean; a.st_out[2 * row + 1] = inv; }
    } else {
        const float mean = a.stats[2 * row], inv = a.stats[2 * row + 1];
        float sg = 0.f, sgu = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = lane + 64 * k;
            v[k] = g[k] = 0.f;
            if (col < a.H) {
                v[k] = a.z[row * a.H + col] - mean;
                g[k] = a.y[row * a.yrs + col] * a.w[col];
            }
            sg += g[k]; sgu += g[k] * v[k];
        }
        sg = wave_sum_all(sg) / (float)a.H;
        sgu = wave_sum_all(sgu);
        const float sd = 1.f / inv - eps;
        const float k2 = sd > 0.f ? inv * inv * sgu / ((float)a.H * sd) : 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int col = lane + 64 * k;
            if (col >= a.H) continue;
            const float dz = inv * (g[k] - sg) - k2 * v[k];
            a.out[row * a.ors + col] = dz * keep_factor((unsigned long long)(row * a.H + col), a.thresh, a.k0, a.k1, a.scale);
            if (a.out2) a.out2[row * a.o2rs + col] = dz;
        }
    }
}

void norm_slices(long long R, int& rps, int& slices) {
    long long r = (R + 1023) / 1024;
    if (r < 128) r = 128;
    rps = (int)r;
    slices = (int)((R + r - 1) / r);
    if (slices < 1) slices = 1;
}

void set_drop(NmArgs& a, double p, uint64_t seed) {
    if (p >= 1.0) { a.thresh = 1u; a.k0 = a.k1 = 0u; a.scale = 0.f; }    // nn.Dropout(p=1): every factor 0
    else set_dropout(a.thresh, a.k0, a.k1, a.scale, p, seed);
}

}  // namespace

extern "C" {

int32_t sgp_gwnet_supported(int32_t H, int32_t Kt) {
    if (const char* e = domain_error(H, Kt)) {
        sgp::fail(SGP_EUNSUP, "sgp_gwnet_supported: %s (H %d, Kt %d)", e, H, Kt);
        return 0;
    }
    return 1;
}

int sgp_gwnet_tconv_f32(const float* X, int64_t x_row_stride, int64_t x_rows, int64_t tap_rows,
                        const float* w_packed, const float* bias, float* Y, int64_t y_row_stride,
                        float* act, int64_t act_row_stride, int64_t n_rows, int32_t H, int32_t Kt,
                        sgp_stream_t stream) {
    SGP_REQUIRE(X && w_packed && bias && Y, "sgp_gwnet_tconv_f32: null pointer");
    SGP_REQUIRE(n_rows > 0 && x_rows > 0 && tap_rows > 0 && H > 0 && Kt > 0, "sgp_gwnet_tconv_f32: bad size");
    if (const char* e = domain_error(H, Kt)) return sgp::fail(SGP_EUNSUP, "sgp_gwnet_tconv_f32: %s (H %d, Kt %d)", e, H, Kt);
    SGP_REQUIRE(n_rows + (int64_t)(Kt - 1) * tap_rows <= x_rows, "sgp_gwnet_tconv_f32: the last tap reads past x");
    SGP_REQUIRE(x_row_stride >= H && y_row_stride >= H && x_row_stride % 4 == 0 && y_row_stride % 4 == 0 &&
                (!act || (act_row_stride >= 2 * H && act_row_stride % 4 == 0)),
                "sgp_gwnet_tconv_f32: a row stride is too small or not a multiple of 4 floats");
    SGP_REQUIRE(sgp::aligned16(X) && sgp::aligned16(w_packed) && sgp::aligned16(Y) && sgp::aligned16(act),
                "sgp_gwnet_tconv_f32: buffers must be 16-byte aligned");
    const int64_t gx = (n_rows + 63) / 64;
    SGP_REQUIRE(gx <= 0x7fffffffll, "sgp_gwnet_tconv_f32: too many rows for one launch");
    TcArgs a;
    a.x = X; a.xrs = x_row_stride; a.tap_rows = tap_rows; a.wp = w_packed; a.bias = bias;
    a.y = Y; a.yrs = y_row_stride; a.act = act; a.ars = act_row_stride;
    a.n_rows = n_rows; a.H = H; a.Kt = Kt;
    hipLaunchKernelGGL(tconv_kernel, dim3((unsigned)gx, (unsigned)((H / 16 + 1) / 2)), dim3(256), 0, (hipStream_t)stream, a);
    return sgp::check_launch("gwnet_tconv");
}

int sgp_gwnet_tconv_bwd_f32(const float* dY, int64_t dy_row_stride, float* act, int64_t act_row_stride,
                            int64_t n_rows, int32_t H, sgp_stream_t stream) {
    SGP_REQUIRE(dY && act, "sgp_gwnet_tconv_bwd_f32: null pointer");
    SGP_REQUIRE(n_rows > 0 && H > 0 && dy_row_stride >= H && act_row_stride >= 2 * H, "sgp_gwnet_tconv_bwd_f32: bad size");
    const long long total = (long long)n_rows * H, blocks = (total + 255) / 256;
    SGP_REQUIRE(blocks <= 0x7fffffffll, "sgp_gwnet_tconv_bwd_f32: too many rows for one launch");
    hipLaunchKernelGGL(tconv_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       dY, (long long)dy_row_stride, act, (long long)act_row_stride, total, (int)H);
    return sgp::check_launch("gwnet_tconv_bwd");
}

int sgp_adj_apply_f32(const float* A, int64_t a_row_stride, int32_t transpose,
                      const float* X, int64_t xcol, int64_t x_row_stride, int64_t x_batch_stride,
                      float* Y, int64_t ycol, int64_t y_row_stride, int64_t y_batch_stride,
                      int32_t n, int32_t batch, int32_t feat, int32_t accumulate, sgp_stream_t stream) {
    SGP_REQUIRE(A && X && Y, "sgp_adj_apply_f32: null pointer");
    SGP_REQUIRE(n > 0 && batch > 0 && feat > 0 && a_row_stride >= n, "sgp_adj_apply_f32: bad size");
    if (feat % 16 != 0) return sgp::fail(SGP_EUNSUP, "sgp_adj_apply_f32: the feature width must be a multiple of 16 (%d)", feat);
    SGP_REQUIRE(xcol >= 0 && ycol >= 0 && x_row_stride >= xcol + feat && y_row_stride >= ycol + feat &&
                x_batch_stride >= 0 && y_batch_stride >= 0, "sgp_adj_apply_f32: bad column range or stride");
    SGP_REQUIRE(xcol % 4 == 0 && ycol % 4 == 0 && x_row_stride % 4 == 0 && y_row_stride % 4 == 0 &&
                x_batch_stride % 4 == 0 && y_batch_stride % 4 == 0 && sgp::aligned16(X) && sgp::aligned16(Y),
                "sgp_adj_apply_f32: X and Y must be 16-byte aligned with strides that are multiples of 4 floats");
    AdjArgs a;
    a.A = A; a.ars = a_row_stride; a.transpose = transpose ? 1 : 0;
    a.x = X + xcol; a.xrs = x_row_stride; a.xbs = x_batch_stride;
    a.y = Y + ycol; a.yrs = y_row_stride; a.ybs = y_batch_stride;
    a.n = n; a.batch = batch; a.F = feat; a.accumulate = accumulate ? 1 : 0;
    a.avec = a_row_stride % 4 == 0 && sgp::aligned16(A);
    const long long gy = ((long long)batch * (feat / 16) + AJ_CT - 1) / AJ_CT;
    SGP_REQUIRE(gy <= 65535, "sgp_adj_apply_f32: too many (item, feature) columns for one launch");
    hipStream_t s = (hipStream_t)stream;
    // 128 destination rows per workgroup when that still gives every CU two workgroups, 64 otherwise
    if ((long long)((n + 127) / 128) * gy >= 512)
        hipLaunchKernelGGL(adj_apply_kernel<2>, dim3((unsigned)((n + 127) / 128), (unsigned)gy), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(adj_apply_kernel<1>, dim3((unsigned)((n + 63) / 64), (unsigned)gy), dim3(256), 0, s, a);
    return sgp::check_launch("adj_apply");
}

int64_t sgp_adj_grad_workspace_floats(int32_t n, int32_t batch) {
    if (n <= 0 || batch <= 0) return -1;
    int ips, slices;
    adj_grad_slices(n, batch, ips, slices);
    return slices > 1 ? (int64_t)slices * n * n : 0;
}

int sgp_adj_grad_f32(const float* dY, int64_t dycol, int64_t dy_row_stride, int64_t dy_batch_stride,
                     const float* X, int64_t xcol, int64_t x_row_stride, int64_t x_batch_stride,
                     float* dA, int64_t da_row_stride, int32_t n, int32_t batch, int32_t feat, int32_t accumulate,
                     float* work, int64_t work_floats, sgp_stream_t stream) {
    SGP_REQUIRE(dY && X && dA, "sgp_adj_grad_f32: null pointer");
    SGP_REQUIRE(n > 0 && batch > 0 && feat > 0 && da_row_stride >= n, "sgp_adj_grad_f32: bad size");
    if (feat % 16 != 0) return sgp::fail(SGP_EUNSUP, "sgp_adj_grad_f32: the feature width must be a multiple of 16 (%d)", feat);
    SGP_REQUIRE(xcol >= 0 && dycol >= 0 && x_row_stride >= xcol + feat && dy_row_stride >= dycol + feat &&
                x_batch_stride >= 0 && dy_batch_stride >= 0, "sgp_adj_grad_f32: bad column range or stride");
    SGP_REQUIRE(xcol % 4 == 0 && dycol % 4 == 0 && x_row_stride % 4 == 0 && dy_row_stride % 4 == 0 &&
                x_batch_stride % 4 == 0 && dy_batch_stride % 4 == 0 && sgp::aligned16(X) && sgp::aligned16(dY),
                "sgp_adj_grad_f32: X and dY must be 16-byte aligned with strides that are multiples of 4 floats");
    int ips, slices;
    adj_grad_slices(n, batch, ips, slices);
    SGP_REQUIRE(slices == 1 || (work && work_floats >= (int64_t)slices * n * n), "sgp_adj_grad_f32: workspace too small");
    AgArgs a;
    a.dy = dY + dycol; a.dyrs = dy_row_stride; a.dybs = dy_batch_stride;
    a.x = X + xcol; a.xrs = x_row_stride; a.xbs = x_batch_stride;
    a.n = n; a.batch = batch; a.F = feat; a.items_per_slice = ips;
    if (slices == 1) { a.out = dA; a.ors = da_row_stride; a.slice_stride = 0; a.accumulate = accumulate ? 1 : 0; }
    else { a.out = work; a.ors = n; a.slice_stride = (long long)n * n; a.accumulate = 0; }
    const unsigned g = (unsigned)(((n + 63) / 64 + 1) / 2);
    SGP_REQUIRE(g <= 65535 && slices <= 65535, "sgp_adj_grad_f32: operator too large for one launch");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adj_grad_kernel, dim3(g, g, (unsigned)slices), dim3(256), 0, s, a);
    int rc = sgp::check_launch("adj_grad");
    if (rc || slices == 1) return rc;
    hipLaunchKernelGGL(adj_grad_reduce, dim3(grid_for((long long)n * n, 256, 8192)), dim3(256), 0, s,
                       work, slices, (int)n, dA, (long long)da_row_stride, accumulate ? 1 : 0);
    return sgp::check_launch("adj_grad_reduce");
}

int sgp_row_softmax_f32(const float* L, int64_t l_row_stride, float* A, int64_t a_row_stride, int32_t n_rows, int32_t n,
                        sgp_stream_t stream) {
    SGP_REQUIRE(L && A, "sgp_row_softmax_f32: null pointer");
    SGP_REQUIRE(n_rows > 0 && n > 0 && l_row_stride >= n && a_row_stride >= n, "sgp_row_softmax_f32: bad size");
    hipLaunchKernelGGL(row_softmax_kernel, dim3((unsigned)n_rows), dim3(SM_T), 0, (hipStream_t)stream,
                       L, (long long)l_row_stride, A, (long long)a_row_stride, (int)n);
    return sgp::check_launch("row_softmax");
}

int sgp_row_softmax_bwd_f32(const float* A, int64_t a_row_stride, const float* dA, int64_t da_row_stride,
                            const float* L, int64_t l_row_stride, float* dL, int64_t dl_row_stride,
                            int32_t n_rows, int32_t n, sgp_stream_t stream) {
    SGP_REQUIRE(A && dA && L && dL, "sgp_row_softmax_bwd_f32: null pointer");
    SGP_REQUIRE(n_rows > 0 && n > 0 && a_row_stride >= n && da_row_stride >= n && l_row_stride >= n && dl_row_stride >= n,
                "sgp_row_softmax_bwd_f32: bad size");
    hipLaunchKernelGGL(row_softmax_bwd_kernel, dim3((unsigned)n_rows), dim3(SM_T), 0, (hipStream_t)stream,
                       A, (long long)a_row_stride, dA, (long long)da_row_stride, L, (long long)l_row_stride,
                       dL, (long long)dl_row_stride, (int)n);
    return sgp::check_launch("row_softmax_bwd");
}

int64_t sgp_gwnet_norm_workspace_doubles(int64_t R, int32_t H) {
    if (R <= 0 || H <= 0) return -1;
    int rps, slices;
    norm_slices(R, rps, slices);
    return (int64_t)(slices + 1) * 2 * H;
}

int sgp_gwnet_norm_f32(int32_t kind, int32_t training, const float* Y, int64_t y_row_stride,
                       const float* res, int64_t res_row_stride, double dropout_p, uint64_t seed,
                       const float* weight, const float* bias, float* running_mean, float* running_var,
                       double momentum, double eps, float* z_save, float* stats,
                       float* out, int64_t out_row_stride, int64_t R, int32_t H,
                       double* work, int64_t work_doubles, sgp_stream_t stream) {
    SGP_REQUIRE(Y && out, "sgp_gwnet_norm_f32: null pointer");
    SGP_REQUIRE(kind >= 0 && kind <= 2, "sgp_gwnet_norm_f32: kind must be 0 (none), 1 (batch) or 2 (layer)");
    SGP_REQUIRE(R > 0 && H > 0 && H <= 256 && y_row_stride >= H && out_row_stride >= H && (!res || res_row_stride >= H),
                "sgp_gwnet_norm_f32: bad size");
    SGP_REQUIRE(R * (int64_t)H / 256 < 0x7fffffffll, "sgp_gwnet_norm_f32: too many rows for one launch");
    SGP_REQUIRE(dropout_p >= 0.0 && dropout_p <= 1.0, "sgp_gwnet_norm_f32: dropout_p must lie in [0, 1]");
    SGP_REQUIRE(kind == 0 || (weight && bias), "sgp_gwnet_norm_f32: the affine parameters are missing");
    SGP_REQUIRE(kind != 1 || stats, "sgp_gwnet_norm_f32: batch statistics need the stats buffer [3 H]");
    SGP_REQUIRE(kind != 1 || training || (running_mean && running_var), "sgp_gwnet_norm_f32: eval mode needs the running buffers");
    SGP_REQUIRE(kind != 1 || !training || R > 1, "sgp_gwnet_norm_f32: batch statistics need more than one row");
    hipStream_t s = (hipStream_t)stream;
    NmArgs a{};
    a.y = Y; a.yrs = y_row_stride; a.res = res; a.rrs = res_row_stride; a.w = weight; a.bias = bias;
    a.zs = z_save; a.out = out; a.ors = out_row_stride; a.R = R; a.H = H; a.kind = kind; a.train = training ? 1 : 0;
    a.stats = stats; a.st_out = stats;
    set_drop(a, dropout_p, seed);
    const unsigned eblocks = (unsigned)((R * (int64_t)H + 255) / 256);
    if (kind == 2) {
        hipLaunchKernelGGL(norm_layer_kernel<0>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, a, (float)eps);
        return sgp::check_launch("gwnet_norm_layer");
    }
    if (kind == 1 && training) {
        int rps, slices;
        norm_slices(R, rps, slices);
        SGP_REQUIRE(work && work_doubles >= (int64_t)slices * 2 * H, "sgp_gwnet_norm_f32: workspace too small");
        a.part = work; a.rows_per_slice = rps;
        hipLaunchKernelGGL(norm_colsum_kernel<0>, dim3((unsigned)slices), dim3(256), 0, s, a);
        if (int rc = sgp::check_launch("gwnet_norm_colsum")) return rc;
        hipLaunchKernelGGL(norm_finalize_fwd, dim3(1), dim3(256), 0, s, (const double*)work, slices, (long long)R, (int)H,
                           eps, momentum, stats, running_mean, running_var);
        if (int rc = sgp::check_launch("gwnet_norm_finalize")) return rc;
    } else if (kind == 1) {
        hipLaunchKernelGGL(norm_stats_eval, dim3(1), dim3(256), 0, s, (const float*)running_mean,
                           (const float*)running_var, (int)H, eps, stats);
        if (int rc = sgp::check_launch("gwnet_norm_stats")) return rc;
    }
    hipLaunchKernelGGL(norm_apply_fwd, dim3(eblocks), dim3(256), 0, s, a);
    return sgp::check_launch("gwnet_norm_apply");
}

int sgp_gwnet_norm_bwd_f32(int32_t kind, int32_t training, const float* dOut, int64_t dout_row_stride,
                           const float* z, const float* stats, const float* weight, double dropout_p, uint64_t seed,
                           double eps, float* dY, int64_t dy_row_stride, float* dRes, int64_t dres_row_stride,
                           float* dweight, float* dbias, int64_t R, int32_t H,
                           double* work, int64_t work_doubles, sgp_stream_t stream) {
    SGP_REQUIRE(dOut && dY, "sgp_gwnet_norm_bwd_f32: null pointer");
    SGP_REQUIRE(kind >= 0 && kind <= 2, "sgp_gwnet_norm_bwd_f32: kind must be 0 (none), 1 (batch) or 2 (layer)");
    SGP_REQUIRE(R > 0 && H > 0 && H <= 256 && dout_row_stride >= H && dy_row_stride >= H && (!dRes || dres_row_stride >= H),
                "sgp_gwnet_norm_bwd_f32: bad size");
    SGP_REQUIRE(R * (int64_t)H / 256 < 0x7fffffffll, "sgp_gwnet_norm_bwd_f32: too many rows for one launch");
    SGP_REQUIRE(dropout_p >= 0.0 && dropout_p <= 1.0, "sgp_gwnet_norm_bwd_f32: dropout_p must lie in [0, 1]");
    SGP_REQUIRE(kind == 0 || (z && stats && weight && dweight && dbias), "sgp_gwnet_norm_bwd_f32: saved state is missing");
    hipStream_t s = (hipStream_t)stream;
    NmArgs a{};
    a.y = dOut; a.yrs = dout_row_stride; a.z = z; a.stats = stats; a.w = weight;
    a.out = dY; a.ors = dy_row_stride; a.out2 = dRes; a.o2rs = dres_row_stride;
    a.R = R; a.H = H; a.kind = kind; a.train = training ? 1 : 0; a.layer_stats = kind == 2 ? 1 : 0;
    set_drop(a, dropout_p, seed);
    if (kind != 0) {
        int rps, slices;
        norm_slices(R, rps, slices);
        SGP_REQUIRE(work && work_doubles >= (int64_t)(slices + 1) * 2 * H, "sgp_gwnet_norm_bwd_f32: workspace too small");
        a.part = work; a.rows_per_slice = rps;
        double* cm = work + (int64_t)slices * 2 * H;
        a.cm = cm;
        hipLaunchKernelGGL(norm_colsum_kernel<1>, dim3((unsigned)slices), dim3(256), 0, s, a);
        if (int rc = sgp::check_launch("gwnet_norm_bwd_colsum")) return rc;
        hipLaunchKernelGGL(norm_finalize_bwd, dim3(1), dim3(256), 0, s, (const double*)work, slices, (long long)R, (int)H,
                           cm, dweight, dbias);
        if (int rc = sgp::check_launch("gwnet_norm_bwd_finalize")) return rc;
    }
    if (kind == 2) {
        hipLaunchKernelGGL(norm_layer_kernel<1>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, a, (float)eps);
        return sgp::check_launch("gwnet_norm_layer_bwd");
    }
    hipLaunchKernelGGL(norm_apply_bwd, dim3((unsigned)((R * (int64_t)H + 255) / 256)), dim3(256), 0, s, a);
    return sgp::check_launch("gwnet_norm_apply_bwd");
}

}  // extern "C"
