// The rest of the SGP decoder (lib/nn/models/sgp_model.py:54-103): the dense layers of tsl's MLP /
// ResidualMLP (tsl/nn/blocks/encoders/mlp.py, tsl/nn/base/dense.py), the positional encoding's
// lin_emb (sgp_model.py:76,97) and the LinearReadout (tsl/nn/blocks/decoders/linear_readout.py), forward
// and backward.  (The MaskedMAE loss the experiments train with is train.hip's sgp_masked_loss_f32.)
//
//   sgp_dense_f32         Y = epilogue(X . M^T): one kernel for every forward layer and every dX of the backward
//                         pass.  The stage loop of dense_tile.h over a workgroup's 64 or 128 rows (gathered, with a
//                         scalar tail where a row cannot be read 16 bytes at a time) x 64 output columns.
//   sgp_dense_wgrad_f32   dM = dZ^T X (+ db = column sums of dZ through a virtual ones column of X): the rows are the
//                         contraction index; every row slice writes its own partial, a second kernel adds the
//                         slices in slice order in fp64 -- no float atomics, the gradients are bit-identical run to run.
//   sgp_row_segsum_f32    node_emb gradient: rows of G summed per node in a fixed order (strided over the batch, or
//                         along a stably sorted index vector).
#include "common.h"
#include "decoder_ops.h"
#include "dense_tile.h"
#include "frag.h"
#include "wg.h"

using sgp::f32x4;

namespace {
using namespace sgp_dense;

// source row of output row r: gidx[r % row_mod] when an index vector is given, r % row_mod without one
// (row_mod = 0: r itself)
__device__ __forceinline__ long long source_row(const int* gidx, long long row_mod, long long r) {
    const long long q = row_mod > 0 ? r % row_mod : r;
    return gidx ? (long long)gidx[q] : q;
}

struct DenseArgs {
    const float* x; long long xrs; const int* gidx; long long row_mod;
    const float* wp; const float* bias;
    int n_rows, k, n_out;
    int act, n_act;                   // forward: act (+ dropout) on the columns < n_act, the others stay linear
    int dmode;                        // 1: backward epilogue, v *= act'(dpre[r, c]) * keep(r, c) on the columns < n_act
    const float* dpre; long long dpre_rs;
    float* pre; long long pre_rs;     // forward: z of the columns < n_act (for the backward pass), or null
    unsigned thresh, k0, k1; float scale; long long drop_w;    // keep(r, c) = Philox(seed, r * drop_w + c)
    const float* add; long long add_rs;                         // + add[r, c] last (residual / positional add)
    float* out; long long o_rdiv, o_r0, o_r1, o_cdiv, o_c0, o_c1;   // out[(r/rdiv) r0 + (r%rdiv) r1 + (c/cdiv) c0 + (c%cdiv) c1]
    bool xvec;
};

template <int RT>
__global__ __launch_bounds__(256) void dense_kernel(DenseArgs a) {
    __shared__ f32x4 wl[DT_LDS];                                    // 16 KB: 64 columns x 64 k of M
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & 15, q = lane >> 4;
    const int JT = (a.n_out + 15) / 16, KB = (a.k + 15) / 16;
    const int jt0 = blockIdx.y * DT_TILES;
    const long long row_base = (long long)blockIdx.x * (64 * RT) + wave * (16 * RT);
    const float* xp[RT];
    bool ok[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const long long row = row_base + 16 * t + b;
        ok[t] = row < a.n_rows;
        xp[t] = ok[t] ? a.x + source_row(a.gidx, a.row_mod, row) * a.xrs : a.x;
    }
    f32x4 acc[RT][DT_TILES];
    dense_tile_loop<RT>(
        wl, a.wp, KB,
        [xp, ok, q, k = a.k, xvec = a.xvec](int t, int kb) {
            const int kk = 16 * kb + 4 * q;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok[t] && kk < k) {
                if (xvec) v = *reinterpret_cast<const f32x4*>(xp[t] + kk);
                else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (kk + s < k) v[s] = xp[t][kk + s];
                }
            }
            return v;
        },
        [jt0, JT](int c) { return jt0 + c < JT ? jt0 + c : -1; }, acc);
    // D[col, row]: lane (q, b), register r -> column 16 (jt0 + c) + 4 q + r, row 16 t + b
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        if (!ok[t]) continue;
        const long long row = row_base + 16 * t + b;
        const long long orow = (row / a.o_rdiv) * a.o_r0 + (row % a.o_rdiv) * a.o_r1;
#pragma unroll
        for (int c = 0; c < DT_TILES; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int col = 16 * (jt0 + c) + 4 * q + r;
                if (col >= a.n_out) continue;
                float v = acc[t][c][r];
                if (a.bias) v += a.bias[col];
                if (col < a.n_act) {
                    const float kf = keep_factor((unsigned long long)(row * a.drop_w + col), a.thresh, a.k0, a.k1, a.scale);
                    if (a.dmode) {
                        v *= dactivate(a.dpre[row * a.dpre_rs + col], a.act) * kf;
                    } else {
                        if (a.pre) a.pre[row * a.pre_rs + col] = v;
                        v = activate(v, a.act) * kf;
                    }
                }
                if (a.add) v += a.add[row * a.add_rs + col];
                a.out[orow + (col / a.o_cdiv) * a.o_c0 + (col % a.o_cdiv) * a.o_c1] = v;
            }
        }
    }
}

// dM[o, i] = sum_rows dZ[row, o] X[row, i] (i = k: the virtual ones column, db).  One wave = 64 o x 64 i over one row
// slice; MFMA with the rows as contraction index: A lane (k, o) = dZ[row0 + k][o], B lane (k, i) = X[row0 + k][i].
struct WgArgs {
    const float* dz; long long dz_rs;
    const float* x; long long xrs; const int* gidx; long long row_mod;
    float* part;                      // [slices, n_out, kp] with kp = k + with_bias
    int n_rows, n_out, k, kp, rows_per_slice, iblocks;
};

__global__ __launch_bounds__(64) void dense_wgrad_kernel(WgArgs a) {
    const int lane = threadIdx.x & 63;
    const int c = lane & 15, kq = lane >> 4;
    const int ob = blockIdx.x / a.iblocks, ib = blockIdx.x % a.iblocks;
    const int s = blockIdx.y;
    const int r0 = s * a.rows_per_slice, r1 = min(a.n_rows, r0 + a.rows_per_slice);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = r0; r < r1; r += 16) {
        float av[4][4], bv[4][4];                                    // [row group u][tile]
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = r + 4 * u + kq;
            const bool ok = row < r1;
            const float* xr = ok ? a.x + source_row(a.gidx, a.row_mod, row) * a.xrs : a.x;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int o = 64 * ob + 16 * t + c, i = 64 * ib + 16 * t + c;
                av[u][t] = (ok && o < a.n_out) ? a.dz[(long long)row * a.dz_rs + o] : 0.f;
                bv[u][t] = (ok && i < a.kp) ? (i < a.k ? xr[i] : 1.f) : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int to = 0; to < 4; ++to)
#pragma unroll
                for (int ti = 0; ti < 4; ++ti)
                    acc[to][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][to], bv[u][ti], acc[to][ti], 0, 0, 0);
    }
    // D: lane (q = kq, j = c), register r -> o = 64 ob + 16 to + 4 q + r, i = 64 ib + 16 ti + c
    float* p = a.part + (long long)s * a.n_out * a.kp;
#pragma unroll
    for (int to = 0; to < 4; ++to)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 64 * ob + 16 * to + 4 * kq + r;
            if (o >= a.n_out) continue;
#pragma unroll
            for (int ti = 0; ti < 4; ++ti) {
                const int i = 64 * ib + 16 * ti + c;
                if (i < a.kp) p[(long long)o * a.kp + i] = acc[to][ti][r];
            }
        }
}

// slices added in slice order in fp64: dw[o * dw_rs + i] (i < k), db[o] (i == k)
__global__ void dense_wgrad_reduce(const float* __restrict__ part, int slices, int n_out, int k, int kp,
                                   float* __restrict__ dw, long long dw_rs, float* __restrict__ db) {
    const long long total = (long long)n_out * kp, stride = total;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
         e += (long long)gridDim.x * blockDim.x) {
        double sum = 0.0;
        for (int s = 0; s < slices; ++s) sum += (double)part[s * stride + e];
        const int o = (int)(e / kp), i = (int)(e % kp);
        if (i < k) dw[(long long)o * dw_rs + i] = (float)sum;
        else db[o] = (float)sum;
    }
}

// out[n, e] = sum of g[row, e] over the rows of node n, in a fixed order:
//   perm == null: row = b * n_seg + n for b = 0, 1, ... (the traffic layout: every batch element holds all nodes)
//   otherwise:    keys[] = the rows' node ids stably sorted, perm[] the rows in that order; thread (p, e) with p the
//                 first position of a run of equal keys adds the run in order (nodes without rows stay zero)
__global__ void row_segsum_kernel(const float* __restrict__ g, long long g_rs, long long n_rows, int width,
                                  const int* __restrict__ perm, const int* __restrict__ keys, int n_seg,
                                  float* __restrict__ out) {
    const long long total = (perm ? n_rows : (long long)n_seg) * width;
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < total;
         t += (long long)gridDim.x * blockDim.x) {
        const long long p = t / width;
        const int e = (int)(t % width);
        double sum = 0.0;
        if (!perm) {
            for (long long row = p; row < n_rows; row += n_seg) sum += (double)g[row * g_rs + e];
            out[p * width + e] = (float)sum;
        } else {
            const int key = keys[p];
            if ((p > 0 && keys[p - 1] == key) || key < 0 || key >= n_seg) continue;
            for (long long qq = p; qq < n_rows && keys[qq] == key; ++qq) sum += (double)g[(long long)perm[qq] * g_rs + e];
            out[(long long)key * width + e] = (float)sum;
        }
    }
}

using sgp::grid_for;

// row slices of the wgrad pass: enough (o, i, slice) waves to fill the chip, each slice >= 64 rows (a multiple of 16)
void wgrad_slices(long long n_rows, int n_out, int kp, int& rps, int& slices) {
    const long long blocks = (long long)((n_out + 63) / 64) * ((kp + 63) / 64);
    long long want = 2048 / (blocks < 1 ? 1 : blocks);
    if (want < 1) want = 1;
    long long r = (n_rows + want - 1) / want;
    if (r < 64) r = 64;
    r = (r + 15) / 16 * 16;
    rps = (int)r;
    slices = (int)((n_rows + r - 1) / r);
    if (slices < 1) slices = 1;
}

}  // namespace

extern "C" {

int64_t sgp_dense_packed_floats(int32_t n_out, int32_t k) {
    if (n_out <= 0 || k <= 0) return -1;
    return sgp::frag_floats(n_out, k);
}

int sgp_dense_pack_f32(const float* w, int64_t w_row_stride, int32_t transpose, int32_t n_out, int32_t k,
                       float* packed, sgp_stream_t stream) {
    SGP_REQUIRE(w && packed, "sgp_dense_pack_f32: null pointer");
    SGP_REQUIRE(n_out > 0 && k > 0 && w_row_stride > 0, "sgp_dense_pack_f32: bad size");
    // M [n_out, k] is w itself, or the transpose of w [k, n_out]
    if (transpose) sgp::frag_pack_to(packed, w, w_row_stride, k, n_out, 1, (hipStream_t)stream);
    else sgp::frag_pack_to(packed, w, w_row_stride, n_out, k, 0, (hipStream_t)stream);
    return sgp::check_launch("dense_pack");
}

int sgp_dense_f32(const float* X, int64_t x_row_stride, const int32_t* gather, int64_t row_mod,
                  const float* w_packed, const float* bias, int32_t n_rows, int32_t k, int32_t n_out,
                  int32_t act, int32_t n_act, int32_t dmode, const float* dpre, int64_t dpre_row_stride,
                  float* pre, int64_t pre_row_stride, double dropout_p, uint64_t seed, int64_t drop_width,
                  const float* add, int64_t add_row_stride,
                  float* out, const int64_t* out_map, sgp_stream_t stream) {
    SGP_REQUIRE(X && w_packed && out && out_map, "sgp_dense_f32: null pointer");
    SGP_REQUIRE(n_rows >= 0 && k > 0 && n_out > 0 && x_row_stride >= k && row_mod >= 0, "sgp_dense_f32: bad size");
    SGP_REQUIRE(act >= 0 && act <= 3 && n_act >= 0 && n_act <= n_out, "sgp_dense_f32: bad activation");
    SGP_REQUIRE(dropout_p >= 0.0 && dropout_p <= 1.0, "sgp_dense_f32: dropout_p must lie in [0, 1]");
    SGP_REQUIRE(!dmode || (dpre && dpre_row_stride >= n_act), "sgp_dense_f32: the backward epilogue needs dpre");
    SGP_REQUIRE(!dmode || !pre, "sgp_dense_f32: pre is a forward output");
    SGP_REQUIRE(dropout_p == 0.0 || drop_width >= n_act, "sgp_dense_f32: drop_width below n_act");
    SGP_REQUIRE(out_map[0] > 0 && out_map[3] > 0, "sgp_dense_f32: out_map divisors must be positive");
    SGP_REQUIRE(sgp::aligned16(w_packed), "sgp_dense_f32: packed weights must be 16-byte aligned");
    SGP_REQUIRE(sgp::frag_floats(n_out, k) / 256 <= 0x7fffffffll, "sgp_dense_f32: packed weights too large");
    if (n_rows == 0) return 0;
    DenseArgs a;
    a.x = X; a.xrs = x_row_stride; a.gidx = gather; a.row_mod = row_mod;
    a.wp = w_packed; a.bias = bias;
    a.n_rows = n_rows; a.k = k; a.n_out = n_out; a.act = act; a.n_act = n_act; a.dmode = dmode;
    a.dpre = dpre; a.dpre_rs = dpre_row_stride; a.pre = pre; a.pre_rs = pre_row_stride;
    if (dropout_p >= 1.0) { a.thresh = 1u; a.k0 = a.k1 = 0u; a.scale = 0.f; }    // nn.Dropout(p=1): every factor 0
    else set_dropout(a.thresh, a.k0, a.k1, a.scale, dropout_p, seed);
    a.drop_w = drop_width;
    a.add = add; a.add_rs = add_row_stride; a.out = out;
    a.o_rdiv = out_map[0]; a.o_r0 = out_map[1]; a.o_r1 = out_map[2];
    a.o_cdiv = out_map[3]; a.o_c0 = out_map[4]; a.o_c1 = out_map[5];
    int32_t rows_per_wg, xvec;
    sgp_dense_form(n_rows, n_out, k, x_row_stride, sgp::aligned16(X) ? 1 : 0, &rows_per_wg, &xvec);   // sizes checked above
    a.xvec = xvec != 0;
    const int gy = (n_out + 16 * DT_TILES - 1) / (16 * DT_TILES);
    SGP_REQUIRE(gy <= 65535, "sgp_dense_f32: too many output columns");
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)(((long long)n_rows + rows_per_wg - 1) / rows_per_wg);
    if (rows_per_wg == 128) hipLaunchKernelGGL(dense_kernel<2>, dim3(gx, gy), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dense_kernel<1>, dim3(gx, gy), dim3(256), 0, s, a);
    return sgp::check_launch("dense");
}

int sgp_dense_form(int32_t n_rows, int32_t n_out, int32_t k, int64_t x_row_stride, int32_t x_aligned16,
                   int32_t* rows_per_wg, int32_t* xvec) {
    SGP_REQUIRE(n_rows >= 0 && k > 0 && n_out > 0 && x_row_stride >= k, "sgp_dense_form: bad size");
    // 128 rows per workgroup when that still gives the chip two workgroups per CU, 64 otherwise
    const long long g128 = ((long long)n_rows + 127) / 128, gy = (n_out + 16 * DT_TILES - 1) / (16 * DT_TILES);
    if (rows_per_wg) *rows_per_wg = g128 * gy >= 512 ? 128 : 64;
    if (xvec) *xvec = (k % 4 == 0 && x_row_stride % 4 == 0 && x_aligned16) ? 1 : 0;
    return 0;
}

int64_t sgp_dense_wgrad_workspace_floats(int64_t n_rows, int32_t n_out, int32_t k, int32_t with_bias) {
    if (n_rows < 0 || n_out <= 0 || k <= 0) return -1;
    int rps, slices;
    const int kp = k + (with_bias ? 1 : 0);
    wgrad_slices(n_rows, n_out, kp, rps, slices);
    return (int64_t)slices * n_out * kp;
}

int sgp_dense_wgrad_f32(const float* dZ, int64_t dz_row_stride, const float* X, int64_t x_row_stride,
                        const int32_t* gather, int64_t row_mod, int32_t n_rows, int32_t n_out, int32_t k,
                        float* dw, int64_t dw_row_stride, float* db, float* work, int64_t work_floats,
                        sgp_stream_t stream) {
    SGP_REQUIRE(dZ && X && dw && work, "sgp_dense_wgrad_f32: null pointer");
    SGP_REQUIRE(n_rows >= 0 && n_out > 0 && k > 0 && dz_row_stride >= n_out && x_row_stride >= k &&
                dw_row_stride >= k && row_mod >= 0, "sgp_dense_wgrad_f32: bad size");
    const int kp = k + (db ? 1 : 0);
    int rps, slices;
    wgrad_slices(n_rows, n_out, kp, rps, slices);
    SGP_REQUIRE(work_floats >= (int64_t)slices * n_out * kp, "sgp_dense_wgrad_f32: workspace too small");
    SGP_REQUIRE(slices <= 65535, "sgp_dense_wgrad_f32: too many row slices");
    hipStream_t s = (hipStream_t)stream;
    if (n_rows == 0) {
        // no rows: zero gradients (the reduction below over one all-zero slice)
        hipError_t e = hipMemsetAsync(work, 0, (size_t)n_out * kp * sizeof(float), s);
        if (e != hipSuccess) return sgp::fail((int)e, "hipMemsetAsync: %s", hipGetErrorString(e));
        slices = 1;
    } else {
        WgArgs a;
        a.dz = dZ; a.dz_rs = dz_row_stride; a.x = X; a.xrs = x_row_stride; a.gidx = gather; a.row_mod = row_mod;
        a.part = work; a.n_rows = n_rows; a.n_out = n_out; a.k = k; a.kp = kp; a.rows_per_slice = rps;
        a.iblocks = (kp + 63) / 64;
        const long long blocks = (long long)((n_out + 63) / 64) * a.iblocks;
        SGP_REQUIRE(blocks < (1ll << 31), "sgp_dense_wgrad_f32: too many tiles");
        hipLaunchKernelGGL(dense_wgrad_kernel, dim3((unsigned)blocks, (unsigned)slices), dim3(64), 0, s, a);
        int rc = sgp::check_launch("dense_wgrad");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(dense_wgrad_reduce, dim3(grid_for((long long)n_out * kp, 256, 4096)), dim3(256), 0, s,
                       work, slices, n_out, k, kp, dw, (long long)dw_row_stride, db);
    return sgp::check_launch("dense_wgrad_reduce");
}

int sgp_row_segsum_f32(const float* g, int64_t g_row_stride, int64_t n_rows, int32_t width,
                       const int32_t* perm, const int32_t* keys, int32_t n_seg, float* out, sgp_stream_t stream) {
    SGP_REQUIRE(g && out, "sgp_row_segsum_f32: null pointer");
    SGP_REQUIRE((perm == nullptr) == (keys == nullptr), "sgp_row_segsum_f32: perm and keys go together");
    SGP_REQUIRE(n_rows >= 0 && width > 0 && n_seg > 0 && g_row_stride >= width, "sgp_row_segsum_f32: bad size");
    SGP_REQUIRE(perm || n_rows % n_seg == 0, "sgp_row_segsum_f32: strided rows must be a multiple of n_seg");
    hipStream_t s = (hipStream_t)stream;
    if (perm) {                                                      // nodes without rows stay zero
        hipError_t e = hipMemsetAsync(out, 0, (size_t)n_seg * width * sizeof(float), s);
        if (e != hipSuccess) return sgp::fail((int)e, "hipMemsetAsync: %s", hipGetErrorString(e));
        if (n_rows == 0) return 0;
    }
    const long long total = (perm ? n_rows : (long long)n_seg) * width;
    hipLaunchKernelGGL(row_segsum_kernel, dim3(grid_for(total, 256, 8192)), dim3(256), 0, s,
                       g, (long long)g_row_stride, (long long)n_rows, width, perm, keys, n_seg, out);
    return sgp::check_launch("row_segsum");
}

}  // extern "C"
