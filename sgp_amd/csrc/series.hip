// Preparing a raw series: temporal resampling, node groups and time encodings -- the arithmetic of tsl's
// PandasDataset.resample_ / TabularDataset.aggregate_ / TemporalFeaturesMixin.datetime_encoded on the device.
//
// All three are bandwidth-bound walks with nothing to reuse: no LDS staging, no vector tricks.  The resample kernel
// gives a lane one output column, so a bin's rows are read as consecutive columns across the wave.  Every element
// offset is a 64-bit product (rows x cols above 2^31 elements works by construction; only the ROW, NODE and BIN numbers
// are 32-bit, as their int32 tables are).  Every sum has one fixed order: a thread adds its rows / nodes in ascending
// order into fp64, and the workgroup form folds its 256 partials with wg.h's halving tree -- no float atomics, so two
// runs give the same bits.
#include "wg.h"
#include <limits.h>
#include <math.h>

namespace {

using sgp::in_range;

constexpr int THREADS = 256;
constexpr int FEAT_CHUNK = 4;         // features a thread of the workgroup form keeps partials for at a time

// what one output element needs of its rows / nodes, whatever the operation: a NaN is skipped (pandas' skipna)
struct Acc {
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    int n = 0, valid = 0, count = 0;              // non-NaN values | valid mask entries | entries walked (mask)
    __device__ __forceinline__ void value(float v) {
        if (v == v) { s += (double)v; lo = v < lo ? v : lo; hi = v > hi ? v : hi; ++n; }
    }
    __device__ __forceinline__ void flag(uint8_t m) { valid += m != 0; ++count; }
    __device__ __forceinline__ void fold(const Acc& o) {
        s += o.s; lo = o.lo < lo ? o.lo : lo; hi = o.hi > hi ? o.hi : hi; n += o.n; valid += o.valid; count += o.count;
    }
    __device__ __forceinline__ float result(int op) const {
        if (op == SGP_SERIES_SUM) return (float)s;
        if (n == 0) return NAN;
        return op == SGP_SERIES_MEAN ? (float)(s / (double)n) : op == SGP_SERIES_MIN ? lo : hi;
    }
    // an empty bin or group is invalid; the comparison is in fp64
    __device__ __forceinline__ uint8_t mask_result(double tol) const {
        return count > 0 && (double)valid / (double)count >= 1.0 - tol;
    }
};

__device__ __forceinline__ int clamp_row(int v, long long n) { return v < 0 ? 0 : (v > n ? (int)n : v); }

// ----------------------------------------------------------------------------------------------------------- resample
// thread i = b * cols + c (64-bit).  With a per-node mask the lane of feature 0 forms the node's mask.
__global__ __launch_bounds__(THREADS) void resample_kernel(const float* __restrict__ x, long long rows, long long cols, int feat,
                                                           const uint8_t* __restrict__ mask, int per_node,
                                                           const int* __restrict__ bin_ptr, const int* __restrict__ src_row,
                                                           long long bins, int op, int flags, double tol,
                                                           float* __restrict__ y, uint8_t* __restrict__ mask_out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (!in_range(i, bins * cols)) return;
    const long long b = i / cols, c = i - b * cols;
    int r0 = 0, r1 = 0;
    if (bin_ptr) {
        r0 = clamp_row(bin_ptr[b], rows);
        r1 = clamp_row(bin_ptr[b + 1], rows);
        if (r1 < r0) r1 = r0;
    }
    Acc a;
    if (op == SGP_SERIES_TAKE) {
        const int r = src_row[b];
        float v = in_range(r, rows) ? x[(long long)r * cols + c] : NAN;
        if (flags & SGP_SERIES_NAN_TO_MASK) {
            mask_out[i] = v == v;
            v = v == v ? v : 0.0f;
        }
        y[i] = v;
    } else {
        for (int r = r0; r < r1; ++r) a.value(x[(long long)r * cols + c]);
        y[i] = a.result(op);
    }
    if (!mask) return;
    long long mcols = cols, mc = c;
    if (per_node) {
        mcols = cols / feat;
        mc = c / feat;
        if (c - mc * feat != 0) return;
    }
    for (int r = r0; r < r1; ++r) a.flag(mask[(long long)r * mcols + mc]);
    mask_out[b * mcols + mc] = a.mask_result(tol);
}

// -------------------------------------------------------------------------------------------------------------- groups
struct Groups {
    const float* x; const uint8_t* mask; const int* ptr; const int* node;
    long long steps, nodes, groups; int feat, per_node;
    // the clamped node range [k0, k1) of group g in `node`
    __device__ __forceinline__ void range(long long g, int& k0, int& k1) const {
        k0 = clamp_row(ptr[g], nodes);
        k1 = clamp_row(ptr[g + 1], nodes);
        if (k1 < k0) k1 = k0;
    }
    // entry k of the node list into `a` for (step t, feature f); with_mask: this lane owns the mask entry too
    __device__ __forceinline__ void take(Acc& a, long long t, int k, int f, bool with_mask) const {
        const int n = node[k];
        if (!in_range(n, nodes)) return;
        const long long row = t * nodes + n;
        a.value(x[row * feat + f]);
        if (with_mask) a.flag(per_node ? mask[row] : mask[row * feat + f]);
    }
};

// regime 0: thread i = (t * groups + g) * feat + f walks its group in node order
__global__ __launch_bounds__(THREADS) void group_thread_kernel(Groups G, int op, double tol, float* __restrict__ y,
                                                               uint8_t* __restrict__ mask_out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (!in_range(i, G.steps * G.groups * G.feat)) return;
    const long long tg = i / G.feat, t = tg / G.groups, g = tg - t * G.groups;
    const int f = (int)(i - tg * G.feat);
    const bool with_mask = G.mask && (!G.per_node || f == 0);
    int k0, k1;
    G.range(g, k0, k1);
    Acc a;
    for (int k = k0; k < k1; ++k) G.take(a, t, k, f, with_mask);
    y[i] = a.result(op);
    if (with_mask) mask_out[G.per_node ? tg : i] = a.mask_result(tol);
}

// regime 1: workgroup blockIdx.x = t * groups + g.  Thread k takes the nodes k, k + 256, .. of the group in order, for
// FEAT_CHUNK features at a time; the 256 partials of each feature go through wg_reduce's halving tree.
__global__ __launch_bounds__(THREADS) void group_wg_kernel(Groups G, int op, double tol, float* __restrict__ y,
                                                           uint8_t* __restrict__ mask_out) {
    __shared__ double sh_s[FEAT_CHUNK][THREADS];
    __shared__ float sh_lo[FEAT_CHUNK][THREADS], sh_hi[FEAT_CHUNK][THREADS];
    __shared__ int sh_n[FEAT_CHUNK][3][THREADS];
    const long long tg = blockIdx.x, t = tg / G.groups, g = tg - t * G.groups;
    if (!in_range(t, G.steps)) return;                      // (workgroup-uniform)
    int k0, k1;
    G.range(g, k0, k1);
    for (int f0 = 0; f0 < G.feat; f0 += FEAT_CHUNK) {
        const int nf = G.feat - f0 < FEAT_CHUNK ? G.feat - f0 : FEAT_CHUNK;
        Acc a[FEAT_CHUNK];
        for (int k = k0 + (int)threadIdx.x; k < k1; k += THREADS)
#pragma unroll
            for (int j = 0; j < FEAT_CHUNK; ++j)
                if (j < nf) G.take(a[j], t, k, f0 + j, G.mask && (!G.per_node || f0 + j == 0));
#pragma unroll
        for (int j = 0; j < FEAT_CHUNK; ++j) {
            sh_s[j][threadIdx.x] = a[j].s; sh_lo[j][threadIdx.x] = a[j].lo; sh_hi[j][threadIdx.x] = a[j].hi;
            sh_n[j][0][threadIdx.x] = a[j].n; sh_n[j][1][threadIdx.x] = a[j].valid; sh_n[j][2][threadIdx.x] = a[j].count;
        }
        sgp::wg_reduce<THREADS>([&](int p, int q) {
#pragma unroll
            for (int j = 0; j < FEAT_CHUNK; ++j) {
                sh_s[j][p] += sh_s[j][q];
                sh_lo[j][p] = sh_lo[j][q] < sh_lo[j][p] ? sh_lo[j][q] : sh_lo[j][p];
                sh_hi[j][p] = sh_hi[j][q] > sh_hi[j][p] ? sh_hi[j][q] : sh_hi[j][p];
#pragma unroll
                for (int c = 0; c < 3; ++c) sh_n[j][c][p] += sh_n[j][c][q];
            }
        });
        if ((int)threadIdx.x < nf) {
            const int j = threadIdx.x, f = f0 + j;
            Acc r;
            r.s = sh_s[j][0]; r.lo = sh_lo[j][0]; r.hi = sh_hi[j][0];
            r.n = sh_n[j][0][0]; r.valid = sh_n[j][1][0]; r.count = sh_n[j][2][0];
            y[tg * G.feat + f] = r.result(op);
            if (G.mask && (!G.per_node || f == 0)) mask_out[G.per_node ? tg : tg * G.feat + f] = r.mask_result(tol);
        }
        __syncthreads();                                    // the slots are refilled by the next chunk
    }
}

// ------------------------------------------------------------------------------------------------------ time encodings
__global__ __launch_bounds__(THREADS) void datetime_kernel(const long long* __restrict__ index_ns, long long steps,
                                                           const long long* __restrict__ period_ns, int units,
                                                           float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (!in_range(i, steps * units)) return;
    const long long t = i / units;
    const int u = (int)(i - t * units);
    const long long p = period_ns[u];
    if (p <= 0) { out[2 * i] = NAN; out[2 * i + 1] = NAN; return; }
    long long r = index_ns[t] % p;                          // C's remainder has the dividend's sign: floor it
    if (r < 0) r += p;
    const double angle = 6.283185307179586476925 * (double)r / (double)p;
    out[2 * i] = (float)sin(angle);
    out[2 * i + 1] = (float)cos(angle);
}

int check_mask(const char* what, const void* mask, const void* mask_out, int64_t cols, int32_t feat, double tol) {
    SGP_REQUIRE(feat > 0 && cols % feat == 0, "%s: cols=%lld is not a multiple of feat=%d", what, (long long)cols, (int)feat);
    SGP_REQUIRE(!mask || mask_out, "%s: a mask needs mask_out", what);
    SGP_REQUIRE(tol == tol, "%s: mask_tol is NaN", what);
    return 0;
}

}  // namespace

extern "C" {

int sgp_series_resample_f32(const float* x, int64_t rows, int64_t cols, int32_t feat, const uint8_t* mask,
                            int32_t mask_per_node, const int32_t* bin_ptr, const int32_t* src_row, int64_t bins, int32_t op,
                            int32_t flags, double mask_tol, float* y, uint8_t* mask_out, sgp_stream_t stream) {
    SGP_REQUIRE(x && y, "sgp_series_resample_f32: null pointer");
    SGP_REQUIRE(rows > 0 && rows < INT_MAX && cols > 0 && bins > 0 && bins < INT_MAX,
                "sgp_series_resample_f32: bad sizes (rows=%lld, cols=%lld, bins=%lld)", (long long)rows, (long long)cols,
                (long long)bins);
    SGP_REQUIRE(op >= SGP_SERIES_SUM && op <= SGP_SERIES_TAKE, "sgp_series_resample_f32: unknown op %d", (int)op);
    if (int rc = check_mask("sgp_series_resample_f32", mask, mask_out, cols, feat, mask_tol)) return rc;
    SGP_REQUIRE(op == SGP_SERIES_TAKE ? src_row != nullptr : bin_ptr != nullptr,
                "sgp_series_resample_f32: op %d needs %s", (int)op, op == SGP_SERIES_TAKE ? "src_row" : "bin_ptr");
    SGP_REQUIRE(!mask || bin_ptr, "sgp_series_resample_f32: a mask needs bin_ptr");
    SGP_REQUIRE((flags & ~SGP_SERIES_NAN_TO_MASK) == 0, "sgp_series_resample_f32: unknown flags %d", (int)flags);
    SGP_REQUIRE(!(flags & SGP_SERIES_NAN_TO_MASK) || (op == SGP_SERIES_TAKE && !mask && mask_out),
                "sgp_series_resample_f32: SGP_SERIES_NAN_TO_MASK goes with op TAKE, no mask and a mask_out");
    SGP_REQUIRE(cols <= LLONG_MAX / 4 / (rows > bins ? rows : bins), "sgp_series_resample_f32: the series is out of range");
    const long long blocks = (bins * cols + THREADS - 1) / THREADS;
    SGP_REQUIRE(blocks <= INT_MAX, "sgp_series_resample_f32: %lld workgroups are out of range", blocks);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, x, (long long)rows,
                       (long long)cols, (int)feat, mask, (int)(mask_per_node != 0), bin_ptr, src_row, (long long)bins,
                       (int)op, (int)flags, mask_tol, y, mask_out);
    return sgp::check_launch("sgp_series_resample_f32");
}

int sgp_series_group_f32(const float* x, int64_t steps, int64_t nodes, int32_t feat, const uint8_t* mask,
                         int32_t mask_per_node, const int32_t* grp_ptr, const int32_t* grp_node, int64_t groups, int32_t op,
                         int32_t regime, double mask_tol, float* y, uint8_t* mask_out, sgp_stream_t stream) {
    SGP_REQUIRE(x && y && grp_ptr && grp_node, "sgp_series_group_f32: null pointer");
    SGP_REQUIRE(steps > 0 && nodes > 0 && nodes < INT_MAX && groups > 0 && groups <= nodes,
                "sgp_series_group_f32: bad sizes (steps=%lld, nodes=%lld, groups=%lld)", (long long)steps, (long long)nodes,
                (long long)groups);
    SGP_REQUIRE(op >= SGP_SERIES_SUM && op <= SGP_SERIES_MAX, "sgp_series_group_f32: unknown op %d", (int)op);
    SGP_REQUIRE(regime == 0 || regime == 1, "sgp_series_group_f32: regime must be 0 (thread) or 1 (workgroup)");
    if (int rc = check_mask("sgp_series_group_f32", mask, mask_out, (int64_t)feat, feat, mask_tol)) return rc;
    SGP_REQUIRE(nodes <= LLONG_MAX / 4 / feat / steps, "sgp_series_group_f32: the series is out of range");
    const long long items = regime == 0 ? steps * groups * feat : steps * groups;
    const long long blocks = regime == 0 ? (items + THREADS - 1) / THREADS : items;
    SGP_REQUIRE(blocks <= INT_MAX, "sgp_series_group_f32: %lld workgroups are out of range", blocks);
    const Groups G{x, mask, grp_ptr, grp_node, (long long)steps, (long long)nodes, (long long)groups, (int)feat,
                   (int)(mask_per_node != 0)};
    if (regime == 0)
        hipLaunchKernelGGL(group_thread_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, G, (int)op,
                           mask_tol, y, mask_out);
    else
        hipLaunchKernelGGL(group_wg_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, G, (int)op,
                           mask_tol, y, mask_out);
    return sgp::check_launch("sgp_series_group_f32");
}

int sgp_datetime_encode_f32(const int64_t* index_ns, int64_t steps, const int64_t* period_ns, int32_t units, float* out,
                            sgp_stream_t stream) {
    SGP_REQUIRE(index_ns && period_ns && out, "sgp_datetime_encode_f32: null pointer");
    SGP_REQUIRE(steps > 0 && units > 0 && steps <= LLONG_MAX / 8 / units, "sgp_datetime_encode_f32: bad sizes (steps=%lld, "
                "units=%d)", (long long)steps, (int)units);
    const long long blocks = (steps * units + THREADS - 1) / THREADS;
    SGP_REQUIRE(blocks <= INT_MAX, "sgp_datetime_encode_f32: %lld workgroups are out of range", blocks);
    hipLaunchKernelGGL(datetime_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream,
                       (const long long*)index_ns, (long long)steps, (const long long*)period_ns, (int)units, out);
    return sgp::check_launch("sgp_datetime_encode_f32");
}

}  // extern "C"
