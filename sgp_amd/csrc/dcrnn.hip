// DCRNN baseline (`--model-name dcrnn`): the diffusion convolution (tsl/nn/layers/graph_convs/diff_conv.py) and the
// GRU cell around it (tsl/nn/blocks/encoders/gcrnn.py:6-19, dcrnn.py), cut so that nothing needs a device-wide barrier.
//
// The diffusion acts on the node axis, the filters on the channel axis, so filters(cat[x | h], A cat[x | h], ..)
// splits exactly into an x side (all S steps at once: hops of x, then ONE sgp_dense_f32 launch into G [S R, 3 H], the
// role of the input projection in rnn_window.hip) and an h side that is sequential in time.  This file is the h side
// and the hop:
//
//   sgp_diffuse_f32        one hop ORDER of up to two supports in one launch: Y[b, i, ycol_s ..] (= | +=) A_s X[b, :,
//                          xcol_s ..].  One wave owns a destination row of one batch item and walks its supports in
//                          order, each row's edges in CSR order with plain FMAs: no atomics, a row's sum has one
//                          fixed order.  X and Y may be the same concat buffer (the column ranges differ).  A hop that
//                          needs its neighbours' previous hop is the next launch in stream order.
//   sgp_dcrnn_gates_f32    [r | u] = sigmoid(Dh Wh_ru^T + G[:, 0 : 2 H]); stores r, u and r * h (slot 0 of Drh).
//   sgp_dcrnn_update_f32   c = tanh(Drh Wh_c^T + G[:, 2 H : 3 H]), h' = u h + (1 - u) c.
//                          Both are the stage loop of dense_tile.h over plain rows of the concat buffer, with the
//                          cell's elementwise step as the epilogue in the accumulator layout.
//   sgp_dcrnn_bwd_f32      the elementwise half of one reversed step, two phases.
//
// Everything else of a step (d concat = dz W, the weight gradients) is sgp_dense_f32 / sgp_dense_wgrad_f32.
#include "common.h"
#include "dense_tile.h"
#include "device_math.h"

namespace {
using sgp::f32x4;
using sgp::sigmoid_f32;
using namespace sgp_dense;

const char* domain_error(int H, int k) {
    if (H < 16 || H > 128 || H % 16 != 0) return "hidden size must be a multiple of 16 in 16 .. 128";
    if (k < 1) return "kernel size k must be at least 1";
    if ((long long)(2 * k + 1) * H > (1 << 24)) return "kernel size k too large";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------- hop
struct Support { const int* rowptr; const int* col; const float* val; long long xcol, ycol; };

struct DiffArgs {
    Support sup[2];
    int n_sup;
    const float* x; long long xrs, xbs;
    float* y; long long yrs, ybs;
    int n, batch, feat, accumulate;
};

__global__ __launch_bounds__(256) void diffuse_kernel(DiffArgs a) {
    const int lane = threadIdx.x & 63;
    const long long w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + 4ll * blockIdx.x;
    if (w >= (long long)a.n * a.batch) return;                       // wave-uniform
    const int i = (int)(w % a.n);
    const long long b = w / a.n;
    const float* xb = a.x + b * a.xbs;
    float* yr = a.y + b * a.ybs + (long long)i * a.yrs;
    for (int s = 0; s < a.n_sup; ++s) {
        const Support& sp = a.sup[s];
        const int e0 = sp.rowptr[i], e1 = sp.rowptr[i + 1];
        for (int f = lane; f < a.feat; f += 64) {
            float acc = a.accumulate ? yr[sp.ycol + f] : 0.f;
            const float* xc = xb + sp.xcol + f;
            int e = e0;
            for (; e + 4 <= e1; e += 4) {                            // four gathers in flight, the sum in edge order
                const float x0 = xc[(long long)sp.col[e] * a.xrs], x1 = xc[(long long)sp.col[e + 1] * a.xrs];
                const float x2 = xc[(long long)sp.col[e + 2] * a.xrs], x3 = xc[(long long)sp.col[e + 3] * a.xrs];
                acc = fmaf(sp.val[e], x0, acc);
                acc = fmaf(sp.val[e + 1], x1, acc);
                acc = fmaf(sp.val[e + 2], x2, acc);
                acc = fmaf(sp.val[e + 3], x3, acc);
            }
            for (; e < e1; ++e) acc = fmaf(sp.val[e], xc[(long long)sp.col[e] * a.xrs], acc);
            yr[sp.ycol + f] = acc;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- cell steps
struct CellArgs {
    const float* d; long long drs;        // concat buffer [R, K], K = (2 k + 1) H, slot 0 in the leading H columns
    const float* wp;                      // sgp_dense_pack_f32 of the weight [n_out, K]
    const float* g; long long grs;        // x side G [R, 3 H] of this step (biases folded in)
    float* ruc; long long rrs;            // [R, 3 H]: r | u | c
    const float* h; long long hrs;        // h_{t-1} [R, H] (slot 0 of Dh)
    float* o0; long long o0rs;            // gates: slot 0 of Drh (r * h); update: h_seq[t] or null
    float* o1; long long o1rs;            // update: slot 0 of the next step's Dh, or null
    float* o2;                            // update: h_last [R, H], or null
    int n_rows, H, K;
};

// MODE 0: gates (n_out = 2 H), MODE 1: update (n_out = H).  64 rows x 64 output columns per workgroup.
template <int MODE>
__global__ __launch_bounds__(256) void cell_kernel(CellArgs a) {
    __shared__ f32x4 wl[DT_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane & 15, q = lane >> 4;
    const int n_out = MODE == 0 ? 2 * a.H : a.H;
    const int JT = n_out / 16, KB = a.K / 16;
    const int jt0 = blockIdx.y * DT_TILES;
    const long long row = (long long)blockIdx.x * 64 + wave * 16 + b;
    const bool ok = row < a.n_rows;
    const float* xp = a.d + (ok ? row : 0) * a.drs;
    f32x4 acc[1][DT_TILES];
    dense_tile_loop<1>(
        wl, a.wp, KB,
        [xp, ok, q, K = a.K](int, int kb) {
            const int kk = 16 * kb + 4 * q;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok && kk < K) v = *reinterpret_cast<const f32x4*>(xp + kk);
            return v;
        },
        [jt0, JT](int c) { return jt0 + c < JT ? jt0 + c : -1; }, acc);
    if (!ok) return;
    // D[col, row]: lane (q, b), register r -> column 16 (jt0 + c) + 4 q + r of row 16 wave + b
#pragma unroll
    for (int c = 0; c < DT_TILES; ++c) {
        const int col0 = 16 * (jt0 + c) + 4 * q;
        if (col0 >= n_out) continue;
        if (MODE == 0) {
            const f32x4 gx = *reinterpret_cast<const f32x4*>(a.g + row * a.grs + col0);
            f32x4 z;
#pragma unroll
            for (int r = 0; r < 4; ++r) z[r] = sigmoid_f32(acc[0][c][r] + gx[r]);
            *reinterpret_cast<f32x4*>(a.ruc + row * a.rrs + col0) = z;
            if (col0 < a.H) {                                         // the r half: r * h into slot 0 of Drh
                const f32x4 hv = *reinterpret_cast<const f32x4*>(a.h + row * a.hrs + col0);
                *reinterpret_cast<f32x4*>(a.o0 + row * a.o0rs + col0) = z * hv;
            }
        } else {
            const f32x4 gx = *reinterpret_cast<const f32x4*>(a.g + row * a.grs + 2 * a.H + col0);
            const f32x4 uv = *reinterpret_cast<const f32x4*>(a.ruc + row * a.rrs + a.H + col0);
            const f32x4 hv = *reinterpret_cast<const f32x4*>(a.h + row * a.hrs + col0);
            f32x4 cv, hn;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cv[r] = sgp_res::tanh_f32(acc[0][c][r] + gx[r]);
                hn[r] = uv[r] * hv[r] + (1.f - uv[r]) * cv[r];
            }
            *reinterpret_cast<f32x4*>(a.ruc + row * a.rrs + 2 * a.H + col0) = cv;
            if (a.o0) *reinterpret_cast<f32x4*>(a.o0 + row * a.o0rs + col0) = hn;
            if (a.o1) *reinterpret_cast<f32x4*>(a.o1 + row * a.o1rs + col0) = hn;
            if (a.o2) *reinterpret_cast<f32x4*>(a.o2 + row * (long long)a.H + col0) = hn;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- backward
struct BwdArgs {
    float* dh;                            // carry [R, H], in place
    const float* ruc; long long rrs;      // [R, 3 H]
    const float* h; long long hrs;        // h_{t-1}
    const float* drh; long long drs;      // phase 2: slot 0 of d Drh
    float* dz; long long zrs;             // [R, 3 H]: dzr | dzu | dzc
    long long total; int H;
};

template <int PHASE>
__global__ __launch_bounds__(256) void bwd_kernel(BwdArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.total) return;
    const long long row = i / a.H;
    const int col = (int)(i % a.H);
    const float hp = a.h[row * a.hrs + col];
    const float* g = a.ruc + row * a.rrs;                            // may alias dz: loads before stores, per thread
    float* dz = a.dz + row * a.zrs;
    if (PHASE == 1) {
        const float dh = a.dh[i], u = g[a.H + col], c = g[2 * a.H + col];
        dz[2 * a.H + col] = dh * (1.f - u) * (1.f - c * c);
        dz[a.H + col] = dh * (hp - c) * u * (1.f - u);
        a.dh[i] = dh * u;
    } else {
        const float d = a.drh[row * a.drs + col], r = g[col];
        dz[col] = d * hp * r * (1.f - r);
        a.dh[i] += d * r;
    }
}

}  // namespace

extern "C" {

int32_t sgp_dcrnn_supported(int32_t H, int32_t k) {
    if (const char* e = domain_error(H, k)) {
        sgp::fail(SGP_EUNSUP, "sgp_dcrnn_supported: %s (H %d, k %d)", e, H, k);
        return 0;
    }
    return 1;
}

int sgp_diffuse_f32(const int32_t* rowptr0, const int32_t* col0, const float* val0, int64_t xcol0, int64_t ycol0,
                    const int32_t* rowptr1, const int32_t* col1, const float* val1, int64_t xcol1, int64_t ycol1,
                    const float* X, int64_t x_row_stride, int64_t x_batch_stride,
                    float* Y, int64_t y_row_stride, int64_t y_batch_stride,
                    int32_t n, int32_t batch, int32_t feat, int32_t accumulate, sgp_stream_t stream) {
    SGP_REQUIRE(rowptr0 && col0 && val0 && X && Y, "sgp_diffuse_f32: null pointer");
    SGP_REQUIRE(!rowptr1 || (col1 && val1), "sgp_diffuse_f32: null pointer");
    SGP_REQUIRE(n >= 0 && batch >= 0 && feat > 0, "sgp_diffuse_f32: bad size");
    SGP_REQUIRE(xcol0 >= 0 && ycol0 >= 0 && xcol1 >= 0 && ycol1 >= 0, "sgp_diffuse_f32: negative column offset");
    SGP_REQUIRE(x_row_stride >= 0 && x_batch_stride >= 0 && y_row_stride >= 0 && y_batch_stride >= 0,
                "sgp_diffuse_f32: negative stride");
    if (n == 0 || batch == 0) return 0;
    DiffArgs a;
    a.sup[0] = Support{rowptr0, col0, val0, xcol0, ycol0};
    a.sup[1] = Support{rowptr1, col1, val1, xcol1, ycol1};
    a.n_sup = rowptr1 ? 2 : 1;
    a.x = X; a.xrs = x_row_stride; a.xbs = x_batch_stride;
    a.y = Y; a.yrs = y_row_stride; a.ybs = y_batch_stride;
    a.n = n; a.batch = batch; a.feat = feat; a.accumulate = accumulate ? 1 : 0;
    const long long blocks = ((long long)n * batch + 3) / 4;
    SGP_REQUIRE(blocks <= 0x7fffffffll, "sgp_diffuse_f32: too many rows for one launch");
    hipLaunchKernelGGL(diffuse_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return sgp::check_launch("diffuse");
}

static int cell_checks(const char* what, const void* D, int64_t drs, const void* W, const void* G, int64_t grs,
                       const void* ruc, int64_t rrs, const void* h, int64_t hrs, int64_t R, int32_t H, int32_t k) {
    if (!(D && W && G && ruc && h)) return sgp::fail(SGP_EINVAL, "%s: null pointer", what);
    if (const char* e = domain_error(H, k)) return sgp::fail(SGP_EUNSUP, "%s: %s (H %d, k %d)", what, e, H, k);
    const long long K = (long long)(2 * k + 1) * H;
    if (R < 0 || R > 0x7fffffffll) return sgp::fail(SGP_EINVAL, "%s: bad row count", what);
    if (drs < K || grs < 3 * H || rrs < 3 * H || hrs < H || drs % 4 || grs % 4 || rrs % 4 || hrs % 4)
        return sgp::fail(SGP_EINVAL, "%s: a row stride is too small or not a multiple of 4 floats", what);
    if (!(sgp::aligned16(D) && sgp::aligned16(W) && sgp::aligned16(G) && sgp::aligned16(ruc) && sgp::aligned16(h)))
        return sgp::fail(SGP_EINVAL, "%s: buffers must be 16-byte aligned", what);
    return 0;
}

int sgp_dcrnn_gates_f32(const float* Dh, int64_t d_row_stride, const float* w_ru_packed,
                        const float* G, int64_t g_row_stride, float* ruc, int64_t ruc_row_stride,
                        float* Drh, int64_t drh_row_stride, int64_t R, int32_t H, int32_t k, sgp_stream_t stream) {
    if (int rc = cell_checks("sgp_dcrnn_gates_f32", Dh, d_row_stride, w_ru_packed, G, g_row_stride, ruc, ruc_row_stride,
                             Dh, d_row_stride, R, H, k)) return rc;
    SGP_REQUIRE(Drh && sgp::aligned16(Drh) && drh_row_stride >= H && drh_row_stride % 4 == 0,
                "sgp_dcrnn_gates_f32: bad Drh");
    if (R == 0) return 0;
    CellArgs a{};
    a.d = Dh; a.drs = d_row_stride; a.wp = w_ru_packed; a.g = G; a.grs = g_row_stride;
    a.ruc = ruc; a.rrs = ruc_row_stride; a.h = Dh; a.hrs = d_row_stride;
    a.o0 = Drh; a.o0rs = drh_row_stride;
    a.n_rows = (int)R; a.H = H; a.K = (2 * k + 1) * H;
    const dim3 grid((unsigned)((R + 63) / 64), (unsigned)((2 * H + 63) / 64));
    hipLaunchKernelGGL(cell_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return sgp::check_launch("dcrnn_gates");
}

int sgp_dcrnn_update_f32(const float* Drh, int64_t d_row_stride, const float* w_c_packed,
                         const float* G, int64_t g_row_stride, float* ruc, int64_t ruc_row_stride,
                         const float* h_prev, int64_t h_row_stride, float* h_seq_t, float* dh_next,
                         int64_t dh_next_row_stride, float* h_last, int64_t R, int32_t H, int32_t k,
                         sgp_stream_t stream) {
    if (int rc = cell_checks("sgp_dcrnn_update_f32", Drh, d_row_stride, w_c_packed, G, g_row_stride, ruc,
                             ruc_row_stride, h_prev, h_row_stride, R, H, k)) return rc;
    SGP_REQUIRE(sgp::aligned16(h_seq_t) && sgp::aligned16(dh_next) && sgp::aligned16(h_last) &&
                (!dh_next || (dh_next_row_stride >= H && dh_next_row_stride % 4 == 0)),
                "sgp_dcrnn_update_f32: bad output buffer");
    if (R == 0) return 0;
    CellArgs a{};
    a.d = Drh; a.drs = d_row_stride; a.wp = w_c_packed; a.g = G; a.grs = g_row_stride;
    a.ruc = ruc; a.rrs = ruc_row_stride; a.h = h_prev; a.hrs = h_row_stride;
    a.o0 = h_seq_t; a.o0rs = H; a.o1 = dh_next; a.o1rs = dh_next_row_stride; a.o2 = h_last;
    a.n_rows = (int)R; a.H = H; a.K = (2 * k + 1) * H;
    const dim3 grid((unsigned)((R + 63) / 64), (unsigned)((H + 63) / 64));
    hipLaunchKernelGGL(cell_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return sgp::check_launch("dcrnn_update");
}

int sgp_dcrnn_bwd_f32(int32_t phase, float* dh, const float* ruc, int64_t ruc_row_stride,
                      const float* h_prev, int64_t h_row_stride, const float* dDrh, int64_t ddrh_row_stride,
                      float* dz, int64_t dz_row_stride, int64_t R, int32_t H, sgp_stream_t stream) {
    SGP_REQUIRE(dh && ruc && h_prev && dz, "sgp_dcrnn_bwd_f32: null pointer");
    SGP_REQUIRE(phase == 1 || phase == 2, "sgp_dcrnn_bwd_f32: phase must be 1 or 2");
    SGP_REQUIRE(phase == 1 || dDrh, "sgp_dcrnn_bwd_f32: phase 2 needs dDrh");
    SGP_REQUIRE(R >= 0 && H > 0 && ruc_row_stride >= 3 * H && dz_row_stride >= 3 * H && h_row_stride >= H &&
                (phase == 1 || ddrh_row_stride >= H), "sgp_dcrnn_bwd_f32: bad size");
    if (R == 0) return 0;
    BwdArgs a;
    a.dh = dh; a.ruc = ruc; a.rrs = ruc_row_stride; a.h = h_prev; a.hrs = h_row_stride;
    a.drh = dDrh; a.drs = ddrh_row_stride; a.dz = dz; a.zrs = dz_row_stride;
    a.total = (long long)R * H; a.H = H;
    const long long blocks = (a.total + 255) / 256;
    SGP_REQUIRE(blocks <= 0x7fffffffll, "sgp_dcrnn_bwd_f32: too many rows for one launch");
    if (phase == 1) hipLaunchKernelGGL(bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(bwd_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return sgp::check_launch("dcrnn_bwd");
}

}  // extern "C"
