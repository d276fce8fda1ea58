// Graph construction on the device: what the reference's drivers get from
// `dataset.get_connectivity(threshold, knn, ...)` (tsl/datasets/prototypes/dataset.py:347-438) -- a dense N x N fp64
// similarity on the host, then top_k / threshold / fill_diagonal / adj_to_edge_index over it.
//
// Row selection.  One wave owns one row i and streams the columns 64 at a time in ascending order.  A candidate is a
// pair (key, column), smaller key = better:
//   geographic  key = min(|u_i - u_j|^2, chord_zero) on fp64 unit vectors: the squared chord is monotone in the haversine
//               distance, so neither asin nor exp is evaluated per pair; chords at and beyond chord_zero (where the
//               fp64 weight is exactly 0) tie, as the weights do
//   dense       key = -sim[i, j], compared as fp64 (fp32 input converts exactly)
// knn mode keeps a buffer of SEL_CAP candidates in LDS: before the first trim every candidate enters, afterwards only
// those whose key is strictly below the current k-th (columns arrive ascending, so a tie at the k-th key always loses
// to the lower column already held).  When fewer than 64 free slots are left the wave sorts the buffer by
// (key, column) -- a bitonic network over the LDS arrays -- and keeps the first k.  After the fill the expected
// number of entrants is k ln(N / SEL_CAP): one or two more sorts per row.  The epilogue evaluates the weight in fp64
// for the k survivors only.
// threshold mode (no knn) is a count pass, a scan of the row counts by the caller and a fill pass that runs the same
// predicate again and writes CSR rows with ascending columns; the geographic predicate is a chord bound, with the
// transcendental evaluated only inside the narrow band [chord_lo, chord_hi] around it.
//
// Correntropy.  One workgroup owns a 64 x 64 output tile for ALL chunks: per chunk the Gram tile on
// v_mfma_f32_32x32x2_f32 (exact fp32; 4 waves as 2 x 2 of 32 x 32), exp(-gamma max(0, n_a + n_b - 2 G)) in the
// epilogue into a register accumulator, one store of acc / n_chunks.
#include "wg.h"
#include <math.h>

namespace {

constexpr int SEL_MAX_KNN = 512;
constexpr int SEL_CAP = 1024;            // candidates one wave holds: k kept + entrants since the last trim
constexpr long long MAX_N = 2147483647ll;
constexpr long long MAX_ROW_GRID = 65535 * 16;     // one wave per row; longer inputs are walked by a grid stride
constexpr double F32_ZERO = 0x1p-150;    // |v| <= 2^-150 rounds to 0 in fp32 (round to nearest even)
constexpr double FP64_EXP_ZERO = 745.1332191019412;   // 1075 ln 2: exp(-a) <= 2^-1075 rounds to 0 in fp64


struct Filter {
    double threshold;      // entries below it are dropped; -inf: none
    int binary;            // kept entries become 1 (knn) / sim > 0 (threshold mode)
    int include_self;
};

__device__ __forceinline__ bool is_edge(double v, double threshold) { return !(v < threshold) && fabs(v) > F32_ZERO; }

// ------------------------------------------------------------------ sources
struct GeoSrc {
    const double* ux; const double* uy; const double* uz;     // unit vectors, one array per coordinate
    double chord_zero, chord_lo, chord_hi, scale;             // scale = 2 R / theta
    double xi, yi, zi;
    __device__ __forceinline__ void begin_row(long long i) { xi = ux[i]; yi = uy[i]; zi = uz[i]; }
    __device__ __forceinline__ double chord(long long j) const {
        const double dx = ux[j] - xi, dy = uy[j] - yi, dz = uz[j] - zi;
        return dx * dx + dy * dy + dz * dz;
    }
    __device__ __forceinline__ double weight(double c) const {
        const double h = fmin(1.0, 0.5 * sqrt(c));
        const double d = scale * asin(h);
        return exp(-d * d);
    }
    __device__ __forceinline__ double key(long long, long long j) const { return fmin(chord(j), chord_zero); }
    __device__ __forceinline__ double value(long long, long long j) const { return weight(chord(j)); }
    // threshold mode: is (i, j) an entry?  Only the band around the bound pays for the weight.
    __device__ __forceinline__ bool keep(long long, long long j, const Filter& f) const {
        const double c = chord(j);
        if (c > chord_hi) return false;
        if (c < chord_lo) return true;
        if (f.binary) {                             // `sim > 0`: exp(-a) rounds to 0 in fp64 from a = 1075 ln 2 on
            const double d = scale * asin(fmin(1.0, 0.5 * sqrt(c)));
            return d * d < FP64_EXP_ZERO && !(1.0 < f.threshold);
        }
        return is_edge(weight(c), f.threshold);
    }
    __device__ __forceinline__ double kept_value(long long i, long long j, const Filter& f) const {
        return f.binary ? 1.0 : value(i, j);
    }
};

template <class T>
struct DenseSrc {
    const T* sim; long long rs, cs;
    const T* row;
    __device__ __forceinline__ void begin_row(long long i) { row = sim + i * rs; }
    __device__ __forceinline__ double value(long long, long long j) const { return (double)row[j * cs]; }
    __device__ __forceinline__ double key(long long i, long long j) const {
        const double v = -value(i, j);
        return v != v ? INFINITY : v;
    }
    __device__ __forceinline__ bool keep(long long i, long long j, const Filter& f) const {
        return is_edge(kept_value(i, j, f), f.threshold);
    }
    __device__ __forceinline__ double kept_value(long long i, long long j, const Filter& f) const {
        const double v = value(i, j);
        return f.binary ? (v > 0.0 ? 1.0 : 0.0) : v;
    }
};

// ------------------------------------------------------------------ knn mode
// ascending by (key, column) over keys[0 .. count), one wave; count is wave-uniform
__device__ __forceinline__ void sort_candidates(double* keys, int* cols, int count, int lane) {
    int np = 64;
    while (np < count) np <<= 1;
    for (int s = count + lane; s < np; s += 64) { keys[s] = INFINITY; cols[s] = 2147483647; }
    __syncthreads();
    for (int size = 2; size <= np; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (np >> 1); t += 64) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const double ka = keys[lo], kb = keys[hi];
                const int ca = cols[lo], cb = cols[hi];
                const bool gt = ka > kb || (ka == kb && ca > cb);
                if (gt == up) { keys[lo] = kb; keys[hi] = ka; cols[lo] = cb; cols[hi] = ca; }
            }
            __syncthreads();
        }
}

template <class Src>
__global__ __launch_bounds__(64) void knn_kernel(Src src, long long n, int k, Filter f, int* __restrict__ out_col,
                                                 double* __restrict__ out_val) {
    __shared__ double keys[SEL_CAP];
    __shared__ int cols[SEL_CAP];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {                     // block-uniform
        src.begin_row(i);
        int count = 0;
        bool full = false;
        double kth = INFINITY;
        for (long long j0 = 0; j0 < n; j0 += 64) {
            const long long j = j0 + lane;
            const bool ok = j < n && (f.include_self || j != i);
            const double key = ok ? src.key(i, j) : INFINITY;
            const bool enter = ok && (!full || key < kth);
            const unsigned long long m = __ballot(enter);
            if (m == 0ull) continue;                                            // wave-uniform
            if (enter) {
                const int pos = count + __popcll(m & below);                    // < SEL_CAP: count <= SEL_CAP - 64 here
                keys[pos] = key;
                cols[pos] = (int)j;
            }
            count += __popcll(m);
            if (count > SEL_CAP - 64) {
                __syncthreads();
                sort_candidates(keys, cols, count, lane);
                count = k;                                                      // count > SEL_CAP - 64 >= k
                kth = keys[k - 1];
                full = true;
                __syncthreads();
            }
        }
        __syncthreads();
        sort_candidates(keys, cols, count, lane);
        if (count > k) count = k;
        for (int s = lane; s < k; s += 64) {
            int c = 0;
            double v = 0.0;
            if (s < count) {
                c = cols[s];
                v = f.binary ? 1.0 : src.value(i, c);
                if (!is_edge(v, f.threshold)) v = 0.0;
            }
            out_col[i * k + s] = c;
            out_val[i * k + s] = v;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ threshold mode
template <class Src, bool FILL>
__global__ __launch_bounds__(64) void rows_kernel(Src src, long long n, Filter f, int* __restrict__ row_count,
                                                  const long long* __restrict__ rowptr, int* __restrict__ out_col,
                                                  double* __restrict__ out_val) {
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        src.begin_row(i);
        long long count = 0;
        long long base = 0, end = 0;
        if (FILL) { base = rowptr[i]; end = rowptr[i + 1]; }
        for (long long j0 = 0; j0 < n; j0 += 64) {
            const long long j = j0 + lane;
            const bool k = j < n && (f.include_self || j != i) && src.keep(i, j, f);
            const unsigned long long m = __ballot(k);
            if (FILL && k) {
                const long long pos = base + count + __popcll(m & below);
                if (pos < end) {                                                // (the count pass ran the same predicate)
                    out_col[pos] = (int)j;
                    out_val[pos] = src.kept_value(i, j, f);
                }
            }
            count += __popcll(m);
        }
        if (!FILL && lane == 0) row_count[i] = (int)count;
    }
}

// ------------------------------------------------------------------ correntropy
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int CT = 64;            // output tile
constexpr int CKB = 16;           // time rows per LDS stage
constexpr int CLD = CT + 32;      // LDS row stride: the two half-waves of an operand read land on disjoint banks

// norms[c, a] = sum over the chunk's rows of x[t, a]^2 (fp64 sum, rounded once)
__global__ __launch_bounds__(256) void chunk_norms_kernel(const float* __restrict__ x, long long ld, int n, int period,
                                                          int n_chunks, float* __restrict__ norms) {
    const long long total = (long long)n_chunks * n;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long c = e / n, a = e - c * n;
        const float* p = x + c * period * ld + a;
        double s = 0.0;
        for (int r = 0; r < period; ++r) { const double v = p[r * ld]; s += v * v; }
        norms[e] = (float)s;
    }
}

__global__ __launch_bounds__(256) void correntropy_kernel(const float* __restrict__ x, long long ld,
                                                          const float* __restrict__ norms, int n, int period,
                                                          int n_chunks, float gamma, float* __restrict__ out,
                                                          long long out_ld) {
    __shared__ float sA[CKB * CLD], sB[CKB * CLD];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int wi = w >> 1, wj = w & 1, kl = lane >> 5, il = lane & 31;
    const int ldcol = tid & 63, ldrow = tid >> 6;                               // staging: one column, rows ldrow + 4 q
    const long long a0 = (long long)blockIdx.y * CT, b0 = (long long)blockIdx.x * CT;
    const bool a_ok = a0 + ldcol < n, b_ok = b0 + ldcol < n;
    const long long j = b0 + wj * 32 + il;                                      // this lane's output column
    f32x16 acc = (f32x16){};
    for (int c = 0; c < n_chunks; ++c) {
        const float* xc = x + (long long)c * period * ld;
        f32x16 g = (f32x16){};
        for (int kb = 0; kb < period; kb += CKB) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < CKB / 4; ++q) {
                const int r = ldrow + 4 * q;
                const bool r_ok = kb + r < period;
                sA[r * CLD + ldcol] = (r_ok && a_ok) ? xc[(long long)(kb + r) * ld + a0 + ldcol] : 0.f;
                sB[r * CLD + ldcol] = (r_ok && b_ok) ? xc[(long long)(kb + r) * ld + b0 + ldcol] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < CKB / 2; ++kk) {
                const float a = sA[(2 * kk + kl) * CLD + wi * 32 + il];
                const float b = sB[(2 * kk + kl) * CLD + wj * 32 + il];
                g = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, g, 0, 0, 0);
            }
        }
        const float* nc = norms + (long long)c * n;
        const float nb = j < n ? nc[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // 32x32 C/D map: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
            const long long i = a0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
            const float na = i < n ? nc[i] : 0.f;
            float d2 = fmaxf(0.f, na + nb - 2.f * g[r]);
            if (i == j) d2 = 0.f;
            acc[r] += expf(-gamma * d2);
        }
    }
    const float inv = 1.f / (float)n_chunks;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long i = a0 + wi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
        if (i < n && j < n) out[i * out_ld + j] = (i == j) ? 1.f : acc[r] * inv;
    }
}

inline int check_select(const char* what, int64_t n, int32_t k, const void* out_col, const void* out_val) {
    if (n < 0 || n > MAX_N) return sgp::fail(SGP_EINVAL, "%s: bad size", what);
    if (k < 1 || k > n) return sgp::fail(SGP_EINVAL, "%s: knn must be in [1, n]", what);
    if (k > SEL_MAX_KNN) return sgp::fail(SGP_EUNSUP, "%s: knn = %d exceeds the kernel's limit %d", what, k, SEL_MAX_KNN);
    if (!out_col || !out_val) return sgp::fail(SGP_EINVAL, "%s: null pointer", what);
    return 0;
}

}  // namespace

extern "C" {

int32_t sgp_conn_max_knn(void) { return SEL_MAX_KNN; }

int sgp_conn_geo_knn_f64(const double* unit, int64_t n, int32_t k, int32_t include_self, int32_t binary,
                         double threshold, double chord_zero, double scale, int32_t* out_col, double* out_val,
                         sgp_stream_t stream) {
    if (int rc = check_select("sgp_conn_geo_knn_f64", n, k, out_col, out_val)) return rc;
    SGP_REQUIRE(unit, "sgp_conn_geo_knn_f64: null pointer");
    SGP_REQUIRE(scale > 0.0 && chord_zero >= 0.0, "sgp_conn_geo_knn_f64: bad scale / chord bound");
    GeoSrc src{unit, unit + n, unit + 2 * n, chord_zero, 0.0, 0.0, scale, 0.0, 0.0, 0.0};
    Filter f{threshold, binary != 0, include_self != 0};
    hipLaunchKernelGGL(knn_kernel<GeoSrc>, dim3(sgp::grid_for(n, 1, MAX_ROW_GRID)), dim3(64), 0, (hipStream_t)stream, src, (long long)n, (int)k,
                       f, out_col, out_val);
    return sgp::check_launch("sgp_conn_geo_knn_f64");
}

int sgp_conn_geo_rows_f64(const double* unit, int64_t n, int32_t include_self, int32_t binary, double threshold,
                          double chord_lo, double chord_hi, double scale, int32_t* row_count, const int64_t* rowptr,
                          int32_t* out_col, double* out_val, sgp_stream_t stream) {
    SGP_REQUIRE(n >= 0 && n <= MAX_N, "sgp_conn_geo_rows_f64: bad size");
    if (!n) return 0;
    SGP_REQUIRE(unit, "sgp_conn_geo_rows_f64: null pointer");
    SGP_REQUIRE(scale > 0.0 && chord_lo <= chord_hi, "sgp_conn_geo_rows_f64: bad scale / chord band");
    SGP_REQUIRE(row_count || (rowptr && out_col && out_val), "sgp_conn_geo_rows_f64: null pointer");
    GeoSrc src{unit, unit + n, unit + 2 * n, 0.0, chord_lo, chord_hi, scale, 0.0, 0.0, 0.0};
    Filter f{threshold, binary != 0, include_self != 0};
    if (row_count)
        hipLaunchKernelGGL((rows_kernel<GeoSrc, false>), dim3(sgp::grid_for(n, 1, MAX_ROW_GRID)), dim3(64), 0, (hipStream_t)stream, src,
                           (long long)n, f, row_count, (const long long*)nullptr, (int*)nullptr, (double*)nullptr);
    else
        hipLaunchKernelGGL((rows_kernel<GeoSrc, true>), dim3(sgp::grid_for(n, 1, MAX_ROW_GRID)), dim3(64), 0, (hipStream_t)stream, src,
                           (long long)n, f, (int*)nullptr, (const long long*)rowptr, out_col, out_val);
    return sgp::check_launch("sgp_conn_geo_rows_f64");
}

int sgp_conn_dense_knn(const void* sim, int32_t is_f64, int64_t row_stride, int64_t col_stride, int64_t n, int32_t k,
                       int32_t include_self, int32_t binary, double threshold, int32_t* out_col, double* out_val,
                       sgp_stream_t stream) {
    if (int rc = check_select("sgp_conn_dense_knn", n, k, out_col, out_val)) return rc;
    SGP_REQUIRE(sim, "sgp_conn_dense_knn: null pointer");
    Filter f{threshold, binary != 0, include_self != 0};
    if (is_f64) {
        DenseSrc<double> src{(const double*)sim, (long long)row_stride, (long long)col_stride, nullptr};
        hipLaunchKernelGGL(knn_kernel<DenseSrc<double>>, dim3(sgp::grid_for(n, 1, MAX_ROW_GRID)), dim3(64), 0, (hipStream_t)stream, src,
                           (long long)n, (int)k, f, out_col, out_val);
    } else {
        DenseSrc<float> src{(const float*)sim, (long long)row_stride, (long long)col_stride, nullptr};
        hipLaunchKernelGGL(knn_kernel<DenseSrc<float>>, dim3(sgp::grid_for(n, 1, MAX_ROW_GRID)), dim3(64), 0, (hipStream_t)stream, src,
                           (long long)n, (int)k, f, out_col, out_val);
    }
    return sgp::check_launch("sgp_conn_dense_knn");
}

int sgp_conn_dense_rows(const void* sim, int32_t is_f64, int64_t row_stride, int64_t col_stride, int64_t n,
                        int32_t include_self, int32_t binary, double threshold, int32_t* row_count,
                        const int64_t* rowptr, int32_t* out_col, double* out_val, sgp_stream_t stream) {
    SGP_REQUIRE(n >= 0 && n <= MAX_N, "sgp_conn_dense_rows: bad size");
    if (!n) return 0;
    SGP_REQUIRE(sim, "sgp_conn_dense_rows: null pointer");
    SGP_REQUIRE(row_count || (rowptr && out_col && out_val), "sgp_conn_dense_rows: null pointer");
    Filter f{threshold, binary != 0, include_self != 0};
    const dim3 grid(sgp::grid_for(n, 1, MAX_ROW_GRID)), block(64);
    hipStream_t s = (hipStream_t)stream;
    const long long* rp = (const long long*)rowptr;
    if (is_f64) {
        DenseSrc<double> src{(const double*)sim, (long long)row_stride, (long long)col_stride, nullptr};
        if (row_count)
            hipLaunchKernelGGL((rows_kernel<DenseSrc<double>, false>), grid, block, 0, s, src, (long long)n, f, row_count,
                               (const long long*)nullptr, (int*)nullptr, (double*)nullptr);
        else
            hipLaunchKernelGGL((rows_kernel<DenseSrc<double>, true>), grid, block, 0, s, src, (long long)n, f,
                               (int*)nullptr, rp, out_col, out_val);
    } else {
        DenseSrc<float> src{(const float*)sim, (long long)row_stride, (long long)col_stride, nullptr};
        if (row_count)
            hipLaunchKernelGGL((rows_kernel<DenseSrc<float>, false>), grid, block, 0, s, src, (long long)n, f, row_count,
                               (const long long*)nullptr, (int*)nullptr, (double*)nullptr);
        else
            hipLaunchKernelGGL((rows_kernel<DenseSrc<float>, true>), grid, block, 0, s, src, (long long)n, f,
                               (int*)nullptr, rp, out_col, out_val);
    }
    return sgp::check_launch("sgp_conn_dense_rows");
}

int sgp_correntropy_f32(const float* x, int64_t x_row_stride, int32_t n, int32_t period, int32_t n_chunks, double gamma,
                        float* norms, float* out, int64_t out_row_stride, sgp_stream_t stream) {
    SGP_REQUIRE(n >= 1 && period >= 1 && n_chunks >= 1, "sgp_correntropy_f32: bad size");
    SGP_REQUIRE((int64_t)n_chunks * period <= MAX_N && (int64_t)n_chunks * n <= MAX_N, "sgp_correntropy_f32: bad size");
    SGP_REQUIRE(x && norms && out, "sgp_correntropy_f32: null pointer");
    SGP_REQUIRE(x_row_stride >= n && out_row_stride >= n, "sgp_correntropy_f32: row stride below the row length");
    const unsigned tiles = (unsigned)((n + CT - 1) / CT);
    SGP_REQUIRE(tiles <= 65535, "sgp_correntropy_f32: more than 65535 x 64 nodes");
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)n_chunks * n;
    const unsigned g = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(chunk_norms_kernel, dim3(g), dim3(256), 0, s, x, (long long)x_row_stride, (int)n, (int)period,
                       (int)n_chunks, norms);
    hipLaunchKernelGGL(correntropy_kernel, dim3(tiles, tiles), dim3(256), 0, s, x, (long long)x_row_stride, norms, (int)n,
                       (int)period, (int)n_chunks, (float)gamma, out, (long long)out_row_stride);
    return sgp::check_launch("sgp_correntropy_f32");
}

}  // extern "C"
