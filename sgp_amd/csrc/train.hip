// The training step outside the model (gfx950): the optimizer, the gradient norm, the losses and the logged metrics.
//   sgp_multi_sqnorm_f32       L2 norm of a LIST of gradient tensors: one workgroup per chunk of the chunk table writes
//                              its fp64 partial, a single workgroup adds the partials in a fixed order.
//   sgp_adam_step_f32          torch.optim.Adam / AdamW over the same chunk table in one launch, with clip_grad_norm_'s
//                              coefficient formed from the device norm inside the update.
//   sgp_masked_metrics_f32     one pass over y_hat, y, mask for the sums behind mae / mse / mape / mre of every horizon
//                              step, added into a persistent [H, 6] fp64 state.
//   sgp_masked_loss_f32 / _bwd MaskedMAE / MSE / MAPE as a loss, optionally at one horizon step.
//   sgp_masked_*_nodes_f32     the same kernels where y / mask hold the root nodes of a sampled batch only.
// Every reduction is a fixed tree over fixed partials: no float atomics, bit-identical from run to run.
//
// Chunk table (device, int64 [n_chunks][3]): (tensor id, element offset, length).  A chunk never crosses a tensor; its
// tensor's four base pointers come from four device pointer arrays indexed by the id.  Tensors need 4-byte alignment
// only: a chunk is walked as (head of up to 3 scalars until the walk's lead pointer is 16-byte aligned, 16-byte
// vectors, tail of up to 3 scalars); an operand that is misaligned relative to the lead is read by scalars.
#include "device_math.h"
#include "wg.h"
#include <math.h>

namespace {

using sgp::f32x4;

constexpr int TR_THREADS = 256;
constexpr int TR_WAVES = TR_THREADS / 64;
constexpr int MET_SEG = 2048;              // elements of one (horizon step, segment) unit of the metric / loss passes
constexpr int MET_COLS = 6;                // |d| sum, |d| count, d^2 sum, |d / y| sum, |d / y| count, masked y sum

// every sum below: NV doubles per thread over the workgroup in a fixed order, valid in thread 0; lds [NV * TR_WAVES]
using sgp::wg_sum_waves;

__device__ __forceinline__ int head_of(const float* p, long long len) {
    const int h = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
    return (long long)h < len ? h : (int)len;
}
__device__ __forceinline__ f32x4 load4(const float* p, bool vec) { return vec ? sgp::ld4(p) : f32x4{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void store4(float* p, bool vec, f32x4 x) {
    if (vec) { sgp::st4(p, x); return; }
    p[0] = x.x; p[1] = x.y; p[2] = x.z; p[3] = x.w;
}

// ------------------------------------------------------------------------------------------------ gradient norm
__global__ __launch_bounds__(TR_THREADS) void multi_sqnorm_kernel(const long long* __restrict__ table,
                                                                  const float* const* __restrict__ grads,
                                                                  double* __restrict__ partial) {
    __shared__ double lds[TR_WAVES];
    const long long c = blockIdx.x;
    const float* g = grads[table[3 * c]] + table[3 * c + 1];
    const long long len = table[3 * c + 2];
    const int head = head_of(g, len);
    const long long nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    double s[1] = {0.0};
    if ((int)threadIdx.x < head) { const double x = g[threadIdx.x]; s[0] += x * x; }
    for (long long i = threadIdx.x; i < nvec; i += TR_THREADS) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(g + head + 4 * i);
        s[0] += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
    }
    if (tail0 + threadIdx.x < len) { const double x = g[tail0 + threadIdx.x]; s[0] += x * x; }
    wg_sum_waves<TR_THREADS>(s, lds);
    if (threadIdx.x == 0) partial[c] = s[0];
}

__global__ __launch_bounds__(TR_THREADS) void sqnorm_final_kernel(const double* __restrict__ partial, long long n,
                                                                  float* __restrict__ norm_f32,
                                                                  double* __restrict__ norm_f64) {
    __shared__ double lds[TR_WAVES];
    double s[1] = {0.0};
    for (long long i = threadIdx.x; i < n; i += TR_THREADS) s[0] += partial[i];
    wg_sum_waves<TR_THREADS>(s, lds);
    if (threadIdx.x == 0) {
        const double nrm = sqrt(s[0]);
        if (norm_f64) norm_f64[0] = nrm;
        norm_f32[0] = (float)nrm;
    }
}

// ------------------------------------------------------------------------------------------------ Adam
struct AdamConst {
    float max_norm;        // <= 0: no clip
    float wd;              // L2: g += wd * p  (0: none)
    float decay;           // decoupled: p *= decay  (1: none)
    float w1;              // 1 - beta1 (lerp weight)
    float beta2, w2;       // v = v * beta2 + w2 * g * g
    float bc2_sqrt, eps;   // denom = sqrt(v) / bc2_sqrt + eps
    float neg_step;        // p += neg_step * m / denom,  neg_step = -lr / (1 - beta1^step)
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float coef, bool clip, const AdamConst& k) {
    if (clip) g *= coef;
    if (k.wd != 0.f) g = g + k.wd * p;
    if (k.decay != 1.f) p *= k.decay;
    // Tensor.lerp_(end, weight): start + weight * (end - start) below 0.5, end - (end - start) * (1 - weight) from there
    m = k.w1 < 0.5f ? m + k.w1 * (g - m) : g - (g - m) * (1.f - k.w1);
    v = v * k.beta2 + k.w2 * g * g;
    const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
    p = p + k.neg_step * m / denom;
}

__global__ __launch_bounds__(TR_THREADS) void adam_step_kernel(const long long* __restrict__ table,
                                                               float* const* __restrict__ params,
                                                               const float* const* __restrict__ grads,
                                                               float* const* __restrict__ exp_avg,
                                                               float* const* __restrict__ exp_avg_sq,
                                                               const float* __restrict__ norm, AdamConst k) {
    const long long c = blockIdx.x;
    const long long t = table[3 * c], off = table[3 * c + 1], len = table[3 * c + 2];
    float* p = params[t] + off;
    const float* g = grads[t] + off;
    float* m = exp_avg[t] + off;
    float* v = exp_avg_sq[t] + off;
    const bool clip = k.max_norm > 0.f;
    float coef = 1.f;
    if (clip) {
        // clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1); a NaN norm stays NaN (the comparison is false)
        coef = k.max_norm / (norm[0] + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;
    }
    const int head = head_of(p, len);
    const long long nvec = (len - head) >> 2, tail0 = head + 4 * nvec;
    if ((int)threadIdx.x < head) adam_one(p[threadIdx.x], g[threadIdx.x], m[threadIdx.x], v[threadIdx.x], coef, clip, k);
    const bool gv = sgp::aligned16(g + head), mv = sgp::aligned16(m + head), vv = sgp::aligned16(v + head);
    for (long long i = threadIdx.x; i < nvec; i += TR_THREADS) {
        const long long e = head + 4 * i;
        const f32x4 P = *reinterpret_cast<f32x4*>(p + e), G = load4(g + e, gv), M = load4(m + e, mv), V = load4(v + e, vv);
        float pp[4] = {P.x, P.y, P.z, P.w}, mm[4] = {M.x, M.y, M.z, M.w}, vs[4] = {V.x, V.y, V.z, V.w};
        const float gg[4] = {G.x, G.y, G.z, G.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) adam_one(pp[q], gg[q], mm[q], vs[q], coef, clip, k);
        const f32x4 Po = {pp[0], pp[1], pp[2], pp[3]}, Mo = {mm[0], mm[1], mm[2], mm[3]}, Vo = {vs[0], vs[1], vs[2], vs[3]};
        *reinterpret_cast<f32x4*>(p + e) = Po;
        store4(m + e, mv, Mo);
        store4(v + e, vv, Vo);
    }
    const long long e = tail0 + threadIdx.x;
    if (e < len) adam_one(p[e], g[e], m[e], v[e], coef, clip, k);
}

// ------------------------------------------------------------------------------------------------ metrics and losses
// y_hat, y, mask are contiguous [B, H, R] (R = nodes * channels).  Horizon step h owns the J = B * R elements
// j = b * R + r at address (b * H + h) * R + r; a unit is MET_SEG consecutive j of one h.
struct Transform { const float* scale; const float* bias; long long node_stride; int channels; };

__device__ __forceinline__ long long addr_of(long long j, long long R, long long H, long long h, long long& r) {
    long long b;
    if (((unsigned long long)j | (unsigned long long)R) >> 32) { b = j / R; r = j - b * R; }
    else { const unsigned q = (unsigned)j / (unsigned)R; b = q; r = (unsigned)j - q * (unsigned)R; }
    return (b * H + h) * R + r;
}

__device__ __forceinline__ float inverse_transform(float yh, const Transform& tr, long long r) {
    if (!tr.scale) return yh;
    const long long n = r / tr.channels, c = r - n * tr.channels;
    const long long at = n * tr.node_stride + c;
    return yh * (tr.scale[at] + 5e-8f) + tr.bias[at];          // ScalerModule.inverse_transform_tensor (tsl.epsilon)
}

// MaskedMetric._check_mask on the metric's own value
__device__ __forceinline__ bool counts(bool m, float val, int mask_nans, int mask_inf) {
    return m && !(mask_nans && isnan(val)) && !(mask_inf && isinf(val));
}

// Where the prediction of element `a` of y / mask lives: a policy, passed to the kernels by value, whose at(a, ah)
// gives the address in y_hat, or false for an element that has none (it is skipped).  The unit walk, the order of the
// sums and the partials do not depend on the policy, so the root-node path is bit-equal to the whole-batch path on
// y_hat[..., tn, :].contiguous(): a documented property, held by the tests.
struct WholeBatch {                         // y_hat has the shape of y: the element's own address
    __device__ __forceinline__ bool at(long long a, long long& ah) const { ah = a; return true; }
};

enum { TN_ERR_RANGE = 1, TN_ERR_REPEAT = 2 };

// y_hat is contiguous [B, H, nodes_all, C], y and mask are [B, H, roots, C], and root j sits at node tn[j] of y_hat
template <class I>
struct RootNodes {
    const I* tn;
    int* err;                               // bit TN_ERR_RANGE is set when tn[j] is no node
    long long nodes_all, Rn;                // Rn = roots * C, whatever `at` makes of the walk's R
    int channels;
    // element a = (bh * roots + j) * C + c of y
    __device__ __forceinline__ bool at(long long a, long long& ah) const {
        long long bh, r;
        if (((unsigned long long)a | (unsigned long long)Rn) >> 32) { bh = a / Rn; r = a - bh * Rn; }
        else { const unsigned q = (unsigned)a / (unsigned)Rn; bh = q; r = (unsigned)a - q * (unsigned)Rn; }
        const long long j = r / channels, c = r - j * channels;
        const I id = tn[j];
        if (!sgp::in_range(id, nodes_all)) { atomicOr(err, TN_ERR_RANGE); return false; }
        ah = (bh * nodes_all + (long long)id) * channels + c;
        return true;
    }
};

template <class Where>
__global__ __launch_bounds__(TR_THREADS) void masked_metrics_kernel(const float* __restrict__ yh, const float* __restrict__ y,
                                                                    const unsigned char* __restrict__ mask, Where where,
                                                                    long long J, long long H, long long R, long long nseg,
                                                                    Transform tr, int mask_nans, int mask_inf,
                                                                    double* __restrict__ partial) {
    __shared__ double lds[MET_COLS * TR_WAVES];
    const long long u = blockIdx.x, h = u / nseg, seg = u - h * nseg;
    const long long j1 = (seg + 1) * MET_SEG < J ? (seg + 1) * MET_SEG : J;
    double s[MET_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long j = seg * MET_SEG + threadIdx.x; j < j1; j += TR_THREADS) {
        long long r, ah;
        const long long a = addr_of(j, R, H, h, r);
        if (!where.at(a, ah)) continue;
        const float t = y[a], d = inverse_transform(yh[ah], tr, r) - t;        // r / channels: the position in y
        const bool m = mask ? mask[a] != 0 : true;
        const float ad = fabsf(d);
        if (counts(m, ad, mask_nans, mask_inf)) { s[0] += (double)ad; s[1] += 1.0; s[2] += (double)(d * d); s[5] += (double)t; }
        const float q = fabsf(d / t);
        if (counts(m, q, mask_nans, 1)) { s[3] += (double)q; s[4] += 1.0; }
    }
    wg_sum_waves<TR_THREADS>(s, lds);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < MET_COLS; ++k) partial[u * MET_COLS + k] = s[k];
}

// one workgroup per horizon step: state[h][k] += sum over the step's segments, in a fixed order
__global__ __launch_bounds__(TR_THREADS) void masked_metrics_final_kernel(const double* __restrict__ partial, long long nseg,
                                                                          double* __restrict__ state) {
    __shared__ double lds[MET_COLS * TR_WAVES];
    const long long h = blockIdx.x;
    double s[MET_COLS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long i = threadIdx.x; i < nseg; i += TR_THREADS)
#pragma unroll
        for (int k = 0; k < MET_COLS; ++k) s[k] += partial[(h * nseg + i) * MET_COLS + k];
    wg_sum_waves<TR_THREADS>(s, lds);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < MET_COLS; ++k) state[h * MET_COLS + k] += s[k];
}

enum { LOSS_MAE = 0, LOSS_MSE = 1, LOSS_MAPE = 2 };

__device__ __forceinline__ float loss_value(int kind, float d, float t) {
    return kind == LOSS_MAE ? fabsf(d) : (kind == LOSS_MSE ? d * d : fabsf(d / t));
}

// d loss / d y_hat of one element: 0 when the masking rules drop it (m: its mask byte, true without a mask)
__device__ __forceinline__ float loss_grad(int kind, float d, float t, bool m, int mask_nans, float scale) {
    if (!counts(m, loss_value(kind, d, t), mask_nans, kind == LOSS_MAPE)) return 0.f;
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f * d);
    return kind == LOSS_MAE ? scale * sgn : (kind == LOSS_MSE ? scale * 2.f * d : scale * sgn / fabsf(t));
}

// (H, R, h): without `at` one flat row (1, J, 0); with it, step `at` of [B, H, R]
template <class Where>
__global__ __launch_bounds__(TR_THREADS) void masked_loss_kernel(const float* __restrict__ yh, const float* __restrict__ y,
                                                                 const unsigned char* __restrict__ mask, Where where,
                                                                 long long J, long long H, long long R, long long h,
                                                                 int kind, int mask_nans, double* __restrict__ partial) {
    __shared__ double lds[2 * TR_WAVES];
    const long long seg = blockIdx.x;
    const long long j1 = (seg + 1) * MET_SEG < J ? (seg + 1) * MET_SEG : J;
    double s[2] = {0.0, 0.0};
    for (long long j = seg * MET_SEG + threadIdx.x; j < j1; j += TR_THREADS) {
        long long r, ah;
        const long long a = addr_of(j, R, H, h, r);
        if (!where.at(a, ah)) continue;
        const float t = y[a], val = loss_value(kind, yh[ah] - t, t);
        if (counts(mask ? mask[a] != 0 : true, val, mask_nans, kind == LOSS_MAPE)) { s[0] += (double)val; s[1] += 1.0; }
    }
    wg_sum_waves<TR_THREADS>(s, lds);
    if (threadIdx.x == 0) { partial[2 * seg] = s[0]; partial[2 * seg + 1] = s[1]; }
}

__global__ __launch_bounds__(TR_THREADS) void masked_loss_final_kernel(const double* __restrict__ partial, long long nseg,
                                                                       float* __restrict__ loss, double* __restrict__ count) {
    __shared__ double lds[2 * TR_WAVES];
    double s[2] = {0.0, 0.0};
    for (long long i = threadIdx.x; i < nseg; i += TR_THREADS) { s[0] += partial[2 * i]; s[1] += partial[2 * i + 1]; }
    wg_sum_waves<TR_THREADS>(s, lds);
    if (threadIdx.x == 0) {
        loss[0] = s[1] > 0.0 ? (float)(s[0] / s[1]) : (float)s[0];      // MaskedMetric.compute: value when numel == 0
        count[0] = s[1];
    }
}

// Two backward kernels, on purpose: this one walks the whole-batch gradient by scalars (256 lanes, at most 8192
// workgroups), masked_loss_nodes_bwd_kernel below writes the full-size root-node gradient four wide (at most 2048
// workgroups).  Merging them would change the launch shape, and with it the speed, of one training step or the other;
// they share loss_grad, the one place the gradient of an element is written.
__global__ void masked_loss_bwd_kernel(const float* __restrict__ yh, const float* __restrict__ y,
                                       const unsigned char* __restrict__ mask, long long n, long long H, long long R,
                                       long long at, int kind, int mask_nans, const float* __restrict__ gout,
                                       const double* __restrict__ count, float* __restrict__ grad) {
    const float scale = gout[0] / (float)count[0];
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        float g = 0.f;
        if (at < 0 || (e / R) % H == at) {
            const float t = y[e];
            g = loss_grad(kind, yh[e] - t, t, mask ? mask[e] != 0 : true, mask_nans, scale);
        }
        grad[e] = g;
    }
}

// ------------------------------------------------------------------------------------------------ root nodes: table, backward
// inv[tn[j]] = j over a table the entry has filled with -1; atomicMax keeps the larger j of a node named twice
template <class I>
__global__ __launch_bounds__(TR_THREADS) void target_nodes_table_kernel(const I* __restrict__ tn, long long roots,
                                                                        long long nodes_all, int* __restrict__ inv,
                                                                        int* __restrict__ err) {
    for (long long j = blockIdx.x * (long long)TR_THREADS + threadIdx.x; j < roots; j += (long long)gridDim.x * TR_THREADS) {
        const I id = tn[j];
        if (!sgp::in_range(id, nodes_all)) { atomicOr(err, TN_ERR_RANGE); continue; }
        if (atomicMax(inv + (long long)id, (int)j) != -1) atomicOr(err, TN_ERR_REPEAT);
    }
}

// One element of the full gradient: row `n` of block bh = b * H + h, channel c, at flat address e of y_hat.
__device__ __forceinline__ float loss_nodes_grad(const float* __restrict__ yh, const float* __restrict__ y,
                                                 const unsigned char* __restrict__ mask, const int* __restrict__ inv,
                                                 long long e, long long bh, long long n, long long c, long long roots,
                                                 int channels, long long H, long long at, int kind, int mask_nans,
                                                 float scale) {
    const int j = inv[n];
    if (!sgp::in_range(j, roots) || !(at < 0 || bh % H == at)) return 0.f;
    const long long a = (bh * roots + j) * channels + c;
    const float t = y[a];
    return loss_grad(kind, yh[e] - t, t, mask ? mask[a] != 0 : true, mask_nans, scale);
}

// The whole gradient [B, H, nodes_all, C] in one pass: thread -> V consecutive elements (V = 4: one 16-byte store),
// every element written once, rows outside tn as +0.
template <int V>
__global__ __launch_bounds__(TR_THREADS) void masked_loss_nodes_bwd_kernel(const float* __restrict__ yh, const float* __restrict__ y,
                                                                           const unsigned char* __restrict__ mask,
                                                                           const int* __restrict__ inv, long long n_all,
                                                                           long long nodes_all, long long roots, int channels,
                                                                           long long H, long long at, int kind, int mask_nans,
                                                                           const float* __restrict__ gout,
                                                                           const double* __restrict__ count,
                                                                           float* __restrict__ grad) {
    const float scale = gout[0] / (float)count[0];
    const long long stride = (long long)gridDim.x * TR_THREADS * V;
    for (long long e0 = (blockIdx.x * (long long)TR_THREADS + threadIdx.x) * V; e0 < n_all; e0 += stride) {
        const long long row = e0 / channels;
        long long c = e0 - row * channels, bh = row / nodes_all, n = row - bh * nodes_all;
        float g[V];
#pragma unroll
        for (int q = 0; q < V; ++q) {
            g[q] = e0 + q < n_all ? loss_nodes_grad(yh, y, mask, inv, e0 + q, bh, n, c, roots, channels, H, at, kind,
                                                    mask_nans, scale) : 0.f;
            if (++c == channels) { c = 0; if (++n == nodes_all) { n = 0; ++bh; } }
        }
        if (V == 4 && e0 + 4 <= n_all) { sgp::st4(grad + e0, f32x4{g[0], g[1], g[2], g[3]}); continue; }
#pragma unroll
        for (int q = 0; q < V; ++q)
            if (e0 + q < n_all) grad[e0 + q] = g[q];
    }
}

long long units_of(long long J) { return J > 0 ? (J + MET_SEG - 1) / MET_SEG : 0; }
constexpr long long MAX_GRID = 2147483647LL;

// ---- launch arithmetic of the root-node entries: the entries and sgp_masked_nodes_form both go through these
constexpr long long NODES_BWD_CAP = 2048;       // workgroups of the backward: 8 of 256 threads on each of 256 CUs
long long loss_J(long long batch, long long horizon, long long roots, long long channels, int at) {
    return at < 0 ? batch * horizon * roots * channels : batch * roots * channels;
}
int nodes_bwd_vec(long long n_all, bool aligned16) { return aligned16 && n_all >= 4 ? 4 : 1; }
unsigned nodes_bwd_grid(long long n_all, int vec) { return sgp::grid_for(n_all, (long long)TR_THREADS * vec, NODES_BWD_CAP); }
long long nodes_bwd_trips(long long n_all, int vec) {
    const long long per = (long long)nodes_bwd_grid(n_all, vec) * TR_THREADS * vec;
    return n_all > 0 ? (n_all + per - 1) / per : 0;
}
unsigned nodes_table_grid(long long roots) { return sgp::grid_for(roots, TR_THREADS, 1024); }
bool index_ok(int index_bytes) { return index_bytes == 4 || index_bytes == 8; }

// f(I{}) with I the index type of `index_bytes` (which index_ok has passed)
template <class F>
void with_index(int index_bytes, F&& f) {
    if (index_bytes == 8) f((long long)0);
    else f((int)0);
}

// ---- the host half of the loss / metrics entries.  `who` is the entry the caller used: it starts every message.
// what every loss entry asks of (kind, at, mask_nans)
int loss_args_ok(const char* who, int kind, int at, int horizon, int mask_nans) {
    SGP_REQUIRE(kind >= LOSS_MAE && kind <= LOSS_MAPE, "%s: kind is 0 (mae), 1 (mse) or 2 (mape)", who);
    SGP_REQUIRE(at >= -1 && (at < 0 || at < horizon), "%s: at outside the horizon", who);
    SGP_REQUIRE(mask_nans == 0 || mask_nans == 1, "%s: mask_nans is 0 or 1", who);
    return 0;
}

// The operands of [B, H, roots, C] y / mask against the prediction; nd is null in the whole-batch entries, whose
// y_hat has the shape of y (they pass their row as `roots` where they have no node axis).
struct NodesArg { const void* tn; int index_bytes; long long nodes_all; int* err; };
struct Operands {
    const float* y_hat; const float* y; const uint8_t* mask; const NodesArg* nd;
    long long batch; int horizon; long long roots; int channels;
};

// the checks both routines below start with; the caller has tested its own pointers into `ptrs`
int operands_ok(const char* who, const Operands& o, bool ptrs, bool sizes) {
    SGP_REQUIRE(ptrs && o.y_hat && o.y && (!o.nd || (o.nd->tn && o.nd->err)), "%s: null pointer", who);
    SGP_REQUIRE(sizes && o.batch >= 0 && o.horizon >= 0 && o.roots >= 0 && o.channels >= 0 && (!o.nd || o.nd->nodes_all >= 0),
                "%s: bad size", who);
    SGP_REQUIRE(!o.nd || index_ok(o.nd->index_bytes), "%s: index_bytes is 4 (int32) or 8 (int64)", who);
    return 0;
}

// f(policy) with the "where is the prediction" policy of the operands
template <class F>
void with_where(const Operands& o, F&& f) {
    if (!o.nd) return f(WholeBatch{});
    with_index(o.nd->index_bytes, [&](auto i) {
        using I = decltype(i);
        f(RootNodes<I>{(const I*)o.nd->tn, o.nd->err, o.nd->nodes_all, o.roots * o.channels, o.channels});
    });
}

// behind sgp_masked_metrics_f32 and sgp_masked_metrics_nodes_f32
int masked_metrics_run(const char* who, const Operands& o, const float* scale, const float* bias, long long sc_node_stride,
                       int mask_nans, int mask_inf, double* work, long long work_doubles, double* state,
                       hipStream_t stream) {
    if (int rc = operands_ok(who, o, work && state, sc_node_stride >= 0)) return rc;
    SGP_REQUIRE((scale == nullptr) == (bias == nullptr), "%s: scale and bias come together", who);
    SGP_REQUIRE((mask_nans == 0 || mask_nans == 1) && (mask_inf == 0 || mask_inf == 1), "%s: mask_nans / mask_inf are 0 or 1",
                who);
    const long long H = o.horizon, R = o.roots * o.channels, J = o.batch * R, nseg = units_of(J);
    if (nseg == 0 || H == 0) return 0;
    SGP_REQUIRE(nseg * H <= MAX_GRID, "%s: too many units", who);
    SGP_REQUIRE(work_doubles >= nseg * H * MET_COLS, "%s: workspace too small", who);
    const Transform tr = {scale, bias, sc_node_stride, o.channels};
    with_where(o, [&](auto where) {
        using Where = decltype(where);
        hipLaunchKernelGGL(masked_metrics_kernel<Where>, dim3((unsigned)(nseg * H)), dim3(TR_THREADS), 0, stream, o.y_hat,
                           o.y, o.mask, where, J, H, R, nseg, tr, mask_nans, mask_inf, work);
    });
    if (int rc = sgp::check_launch(who)) return rc;
    hipLaunchKernelGGL(masked_metrics_final_kernel, dim3((unsigned)H), dim3(TR_THREADS), 0, stream, (const double*)work,
                       nseg, state);
    return sgp::check_launch("masked_metrics_final");
}

// behind sgp_masked_loss_f32 and sgp_masked_loss_nodes_f32; the final kernel runs on empty operands too (loss 0, count 0)
int masked_loss_run(const char* who, const Operands& o, int kind, int at, int mask_nans, double* work,
                    long long work_doubles, float* loss, double* count, hipStream_t stream) {
    if (int rc = operands_ok(who, o, work && loss && count, true)) return rc;
    if (int rc = loss_args_ok(who, kind, at, o.horizon, mask_nans)) return rc;
    const long long J = loss_J(o.batch, o.horizon, o.roots, o.channels, at), nseg = units_of(J);
    SGP_REQUIRE(nseg <= MAX_GRID, "%s: too many units", who);
    SGP_REQUIRE(work_doubles >= 2 * nseg, "%s: workspace too small", who);
    if (nseg > 0) {
        // without `at` the tensor is one flat row; with it, step `at` of [B, H, R]
        const long long H = at < 0 ? 1LL : (long long)o.horizon, R = at < 0 ? J : o.roots * o.channels, h = at < 0 ? 0LL : at;
        with_where(o, [&](auto where) {
            using Where = decltype(where);
            hipLaunchKernelGGL(masked_loss_kernel<Where>, dim3((unsigned)nseg), dim3(TR_THREADS), 0, stream, o.y_hat, o.y,
                               o.mask, where, J, H, R, h, kind, mask_nans, work);
        });
        if (int rc = sgp::check_launch(who)) return rc;
    }
    hipLaunchKernelGGL(masked_loss_final_kernel, dim3(1), dim3(TR_THREADS), 0, stream, (const double*)work, nseg, loss, count);
    return sgp::check_launch("masked_loss_final");
}

}  // namespace

extern "C" {

int sgp_multi_sqnorm_f32(const int64_t* table, int64_t n_chunks, const float* const* grads, double* partial,
                         float* norm_f32, double* norm_f64, sgp_stream_t stream) {
    SGP_REQUIRE(table && grads && partial && norm_f32, "sgp_multi_sqnorm_f32: null pointer");
    SGP_REQUIRE(n_chunks >= 0 && n_chunks <= MAX_GRID, "sgp_multi_sqnorm_f32: bad size");
    if (n_chunks > 0) {
        hipLaunchKernelGGL(multi_sqnorm_kernel, dim3((unsigned)n_chunks), dim3(TR_THREADS), 0, (hipStream_t)stream,
                           (const long long*)table, grads, partial);
        if (int rc = sgp::check_launch("multi_sqnorm")) return rc;
    }
    hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(TR_THREADS), 0, (hipStream_t)stream, partial,
                       (long long)n_chunks, norm_f32, norm_f64);
    return sgp::check_launch("sqnorm_final");
}

int sgp_adam_step_f32(const int64_t* table, int64_t n_chunks, float* const* params, const float* const* grads,
                      float* const* exp_avg, float* const* exp_avg_sq, const float* norm, double max_norm,
                      double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                      int32_t decoupled, sgp_stream_t stream) {
    SGP_REQUIRE(table && params && grads && exp_avg && exp_avg_sq, "sgp_adam_step_f32: null pointer");
    SGP_REQUIRE(n_chunks >= 0 && n_chunks <= MAX_GRID, "sgp_adam_step_f32: bad size");
    SGP_REQUIRE(step >= 1, "sgp_adam_step_f32: step counts from 1");
    SGP_REQUIRE(decoupled == 0 || decoupled == 1, "sgp_adam_step_f32: decoupled is 0 or 1");
    SGP_REQUIRE(!(max_norm > 0.0) || norm, "sgp_adam_step_f32: a clip needs the norm (null pointer)");
    SGP_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0 && lr >= 0.0 && weight_decay >= 0.0,
                "sgp_adam_step_f32: bad hyper-parameter");
    if (n_chunks == 0) return 0;
    // torch.optim.adam._single_tensor_adam: the scalars are formed in double on the host and rounded once
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    AdamConst k;
    k.max_norm = max_norm > 0.0 ? (float)max_norm : 0.f;
    k.wd = decoupled ? 0.f : (float)weight_decay;
    k.decay = decoupled ? (float)(1.0 - lr * weight_decay) : 1.f;
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.bc2_sqrt = (float)sqrt(bc2);
    k.eps = (float)eps;
    k.neg_step = (float)(-(lr / bc1));
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)n_chunks), dim3(TR_THREADS), 0, (hipStream_t)stream,
                       (const long long*)table, params, grads, exp_avg, exp_avg_sq, norm, k);
    return sgp::check_launch("adam_step");
}

int64_t sgp_masked_metrics_workspace_doubles(int64_t batch, int32_t horizon, int64_t nodes, int32_t channels) {
    if (batch < 0 || horizon < 0 || nodes < 0 || channels < 0) return -1;
    return (int64_t)horizon * units_of(batch * nodes * channels) * MET_COLS;
}

int sgp_masked_metrics_f32(const float* y_hat, const float* y, const uint8_t* mask, int64_t batch, int32_t horizon,
                           int64_t nodes, int32_t channels, const float* scale, const float* bias,
                           int64_t sc_node_stride, int32_t mask_nans, int32_t mask_inf, double* work,
                           int64_t work_doubles, double* state, sgp_stream_t stream) {
    return masked_metrics_run("sgp_masked_metrics_f32", {y_hat, y, mask, nullptr, batch, horizon, nodes, channels}, scale,
                              bias, sc_node_stride, mask_nans, mask_inf, work, work_doubles, state, (hipStream_t)stream);
}

int64_t sgp_masked_loss_workspace_doubles(int64_t batch, int32_t horizon, int64_t row, int32_t at) {
    if (batch < 0 || horizon < 0 || row < 0) return -1;
    return 2 * units_of(loss_J(batch, horizon, row, 1, at));
}

int sgp_masked_loss_f32(const float* y_hat, const float* y, const uint8_t* mask, int64_t batch, int32_t horizon,
                        int64_t row, int32_t kind, int32_t at, int32_t mask_nans, double* work, int64_t work_doubles,
                        float* loss, double* count, sgp_stream_t stream) {
    return masked_loss_run("sgp_masked_loss_f32", {y_hat, y, mask, nullptr, batch, horizon, row, 1}, kind, at, mask_nans,
                           work, work_doubles, loss, count, (hipStream_t)stream);
}

int sgp_masked_loss_bwd_f32(const float* y_hat, const float* y, const uint8_t* mask, int64_t batch, int32_t horizon,
                            int64_t row, int32_t kind, int32_t at, int32_t mask_nans, const float* grad_out,
                            const double* count, float* grad, sgp_stream_t stream) {
    SGP_REQUIRE(y_hat && y && grad_out && count && grad, "sgp_masked_loss_bwd_f32: null pointer");
    SGP_REQUIRE(batch >= 0 && horizon >= 0 && row >= 0, "sgp_masked_loss_bwd_f32: bad size");
    if (int rc = loss_args_ok("sgp_masked_loss_bwd_f32", kind, at, horizon, mask_nans)) return rc;
    const long long n = batch * horizon * row;
    if (n == 0) return 0;
    hipLaunchKernelGGL(masked_loss_bwd_kernel, dim3(sgp::grid_for(n, 256, 8192)), dim3(256), 0, (hipStream_t)stream,
                       y_hat, y, mask, n, (long long)horizon, (long long)row, (long long)at, kind, mask_nans, grad_out,
                       count, grad);
    return sgp::check_launch("masked_loss_bwd");
}

int sgp_masked_nodes_form(int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots, int32_t channels,
                          int32_t at, int32_t index_bytes, int32_t grad_aligned16, int64_t* out) {
    SGP_REQUIRE(out, "sgp_masked_nodes_form: null pointer");
    SGP_REQUIRE(batch >= 0 && horizon >= 0 && nodes_all >= 0 && roots >= 0 && channels >= 0,
                "sgp_masked_nodes_form: bad size");
    if (int rc = loss_args_ok("sgp_masked_nodes_form", LOSS_MAE, at, horizon, 0)) return rc;      // (only `at` is the caller's)
    SGP_REQUIRE(index_ok(index_bytes), "sgp_masked_nodes_form: index_bytes is 4 (int32) or 8 (int64)");
    const long long n_all = batch * horizon * nodes_all * channels;
    const int vec = nodes_bwd_vec(n_all, grad_aligned16 != 0);
    out[0] = units_of(loss_J(batch, horizon, roots, channels, at));
    out[1] = units_of(batch * roots * channels);
    out[2] = n_all > 0 ? (long long)nodes_bwd_grid(n_all, vec) : 0;
    out[3] = nodes_bwd_trips(n_all, vec);
    out[4] = vec;
    out[5] = index_bytes == 8;
    out[6] = roots > 0 ? (long long)nodes_table_grid(roots) : 0;
    return 0;
}

int sgp_target_nodes_table(const void* target_nodes, int32_t index_bytes, int64_t roots, int64_t nodes_all,
                           int32_t* inv, int32_t* err, sgp_stream_t stream) {
    SGP_REQUIRE(inv && err && (target_nodes || roots == 0), "sgp_target_nodes_table: null pointer");
    SGP_REQUIRE(roots >= 0 && nodes_all > 0 && roots <= 2147483647LL && nodes_all <= 2147483647LL,
                "sgp_target_nodes_table: bad size");
    SGP_REQUIRE(index_ok(index_bytes), "sgp_target_nodes_table: index_bytes is 4 (int32) or 8 (int64)");
    hipError_t e = hipMemsetAsync(inv, 0xFF, (size_t)nodes_all * sizeof(int32_t), (hipStream_t)stream);   // every entry -1
    if (e != hipSuccess) return sgp::fail((int)e, "hipMemsetAsync: %s", hipGetErrorString(e));
    if (roots == 0) return 0;
    with_index(index_bytes, [&](auto i) {
        using I = decltype(i);
        hipLaunchKernelGGL(target_nodes_table_kernel<I>, dim3(nodes_table_grid(roots)), dim3(TR_THREADS), 0,
                           (hipStream_t)stream, (const I*)target_nodes, (long long)roots, (long long)nodes_all, inv, err);
    });
    return sgp::check_launch("target_nodes_table");
}

int sgp_masked_metrics_nodes_f32(const float* y_hat, const float* y, const uint8_t* mask, const void* target_nodes,
                                 int32_t index_bytes, int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots,
                                 int32_t channels, const float* scale, const float* bias, int64_t sc_node_stride,
                                 int32_t mask_nans, int32_t mask_inf, int32_t* err, double* work, int64_t work_doubles,
                                 double* state, sgp_stream_t stream) {
    const NodesArg nd = {target_nodes, index_bytes, nodes_all, err};
    return masked_metrics_run("sgp_masked_metrics_nodes_f32", {y_hat, y, mask, &nd, batch, horizon, roots, channels}, scale,
                              bias, sc_node_stride, mask_nans, mask_inf, work, work_doubles, state, (hipStream_t)stream);
}

int sgp_masked_loss_nodes_f32(const float* y_hat, const float* y, const uint8_t* mask, const void* target_nodes,
                              int32_t index_bytes, int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots,
                              int32_t channels, int32_t kind, int32_t at, int32_t mask_nans, int32_t* err, double* work,
                              int64_t work_doubles, float* loss, double* count, sgp_stream_t stream) {
    const NodesArg nd = {target_nodes, index_bytes, nodes_all, err};
    return masked_loss_run("sgp_masked_loss_nodes_f32", {y_hat, y, mask, &nd, batch, horizon, roots, channels}, kind, at,
                           mask_nans, work, work_doubles, loss, count, (hipStream_t)stream);
}

int sgp_masked_loss_nodes_bwd_f32(const float* y_hat, const float* y, const uint8_t* mask, const int32_t* inv,
                                  int64_t batch, int32_t horizon, int64_t nodes_all, int64_t roots, int32_t channels,
                                  int32_t kind, int32_t at, int32_t mask_nans, const float* grad_out,
                                  const double* count, float* grad, sgp_stream_t stream) {
    SGP_REQUIRE(y_hat && inv && grad_out && count && grad && (y || roots == 0), "sgp_masked_loss_nodes_bwd_f32: null pointer");
    SGP_REQUIRE(batch >= 0 && horizon >= 0 && nodes_all >= 0 && roots >= 0 && channels >= 0 && roots <= 2147483647LL,
                "sgp_masked_loss_nodes_bwd_f32: bad size");
    if (int rc = loss_args_ok("sgp_masked_loss_nodes_bwd_f32", kind, at, horizon, mask_nans)) return rc;
    const long long n_all = batch * horizon * nodes_all * channels;
    if (n_all == 0) return 0;
    const int vec = nodes_bwd_vec(n_all, sgp::aligned16(grad));
    const dim3 grid(nodes_bwd_grid(n_all, vec)), block(TR_THREADS);
    if (vec == 4)
        hipLaunchKernelGGL(masked_loss_nodes_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, y_hat, y, mask, inv, n_all,
                           (long long)nodes_all, (long long)roots, channels, (long long)horizon, (long long)at, kind,
                           mask_nans, grad_out, count, grad);
    else
        hipLaunchKernelGGL(masked_loss_nodes_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, y_hat, y, mask, inv, n_all,
                           (long long)nodes_all, (long long)roots, channels, (long long)horizon, (long long)at, kind,
                           mask_nans, grad_out, count, grad);
    return sgp::check_launch("masked_loss_nodes_bwd");
}

}  // extern "C"
