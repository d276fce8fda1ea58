// The product of two CSR operators on the device, and the row subset of one: what scipy's
// (A_hat @ A_hat) gives sgp_spatial_support on the host (lib/sgp_preprocessing.py:143-145), bit for bit, and what
// ShiftOperator.index_select(0, index) copies there (lib/datasets/iid_dataset.py:113).
//
//   product (count)  ONE wave per output row i, a band of BAND columns at a time: a dense fp32 accumulator and a
//                    touched flag per column in LDS.  k walks row i of A in order; the lanes stride over row k of B (a
//                    column occurs once in a row of B, so no two lanes meet) and do acc[j] = acc[j] + a * b: one
//                    multiply, one add, from +0.0f, ascending k -- scipy's order.  A flag scan over the touched part
//                    of the band counts the entries whose sum does not compare equal to zero (NaN stays).  A band
//                    pass also finds the smallest column beyond the band: the next band is the one that holds it, so
//                    only bands with entries are walked.
//   scan             ONE workgroup: exclusive scan of the row counts in 64 bits -> rowptr, clamped to the capacity;
//                    the total (clamped) is *nnz; a total beyond the capacity sets SGP_SPGEMM_ERR_CAPACITY
//   product (emit)   the same walk; the flag scan writes column and sum at the row's place, in column order
//
//   take rows        lengths (one thread per selected row), the same scan, copy (one wave per selected row)
//
// The waves of a workgroup never wait for one another and no workgroup waits for another.  Every position that comes
// from device data -- a rowptr entry of A, B or the result, a column of A used as a row of B, a column of B used as an
// accumulator slot, an index of the row subset -- is compared with the size of what it indexes first.
#include "wg.h"

#pragma clang fp contract(off)

namespace {
using sgp::grid_for;
using sgp::in_range;

constexpr int WAVE = 64;
constexpr int BAND = 4096;                        // columns per band: 16 KiB of sums + 4 KiB of flags per wave, 8 waves per CU
constexpr int COPY_THREADS = 256;
constexpr int SCAN_THREADS = 1024;
constexpr long long MAX_ITEMS = 2147483647ll;
constexpr long long NO_COLUMN = 0x7fffffffffffffffll;

static_assert(BAND % WAVE == 0, "the flag scan walks whole groups of 64 columns");

inline long long align256(long long b) { return (b + 255) & ~255ll; }

struct Csr {
    const int* rowptr;
    const int* col;
    const float* val;
    long long rows, cols, cap;                    // cap: the entries behind col / val
};

// the entries [lo, hi) of row r (r in range): inside [0, cap] and lo <= hi, whatever rowptr holds
__device__ __forceinline__ bool row_span(const Csr& m, long long r, long long& lo, long long& hi) {
    const long long a = m.rowptr[r], b = m.rowptr[r + 1];
    lo = a < 0 ? 0 : (a > m.cap ? m.cap : a);
    hi = b < lo ? lo : (b > m.cap ? m.cap : b);
    return a == lo && b == hi;
}

// Orders the LDS accesses of the ONE wave of a workgroup: the instructions of a wave reach the LDS in program order,
// so the compiler is the only one that has to be told.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool EMIT>
__global__ __launch_bounds__(WAVE) void product_kernel(Csr A, Csr B, int* __restrict__ counts,
                                                       const int* __restrict__ rowptr, int* __restrict__ col,
                                                       float* __restrict__ val, long long capacity, int* err) {
    __shared__ float acc[BAND];
    __shared__ unsigned char hit[BAND];
    const int lane = threadIdx.x;
    for (int s = lane; s < BAND; s += WAVE) { acc[s] = 0.f; hit[s] = 0; }
    wave_sync();
    for (long long i = blockIdx.x; i < A.rows; i += gridDim.x) {                // wave-uniform
        long long a0, a1;
        bool bad = !row_span(A, i, a0, a1);
        long long out = 0, end = 0;                                             // the row's places in col / val
        if (EMIT) {
            const long long p = rowptr[i], q = rowptr[i + 1];
            out = p < 0 ? 0 : (p > capacity ? capacity : p);
            end = q < out ? out : (q > capacity ? capacity : q);
        }
        long long kept = 0, lo = 0;
        for (;;) {                                                              // one band [lo, lo + BAND) per round
            const long long hi = lo + BAND;
            int first = BAND, last = -1;                                        // the slots this lane touched
            long long next = NO_COLUMN;                                         // the smallest column at or beyond hi
            for (long long c0 = a0; c0 < a1; c0 += WAVE) {                      // 64 entries of A's row at a time
                const int cnt = (int)(a1 - c0 < WAVE ? a1 - c0 : WAVE);
                float mine = 0.f;
                long long b0 = 0, b1 = 0;                                       // the lane's entry: its value, its row of B
                if (lane < cnt) {
                    const int k = A.col[c0 + lane];
                    mine = A.val[c0 + lane];
                    if (!in_range(k, B.rows)) bad = true;
                    else if (!row_span(B, k, b0, b1)) bad = true;
                }
                for (int t = 0; t < cnt; ++t) {                                 // ascending k
                    const float a = __shfl(mine, t, WAVE);
                    const long long f0 = __shfl(b0, t, WAVE), f1 = __shfl(b1, t, WAVE);
                    for (long long f = f0 + lane; f < f1; f += WAVE) {
                        const int j = B.col[f];
                        if (!in_range(j, B.cols)) { bad = true; continue; }
                        if (j < lo) continue;
                        if (j >= hi) { next = j < next ? j : next; continue; }
                        const int s = (int)(j - lo);
                        const float term = a * B.val[f];                        // (the Makefile builds this file with
                        acc[s] = acc[s] + term;                                 // -ffp-contract=off: never one fma)
                        hit[s] = 1;
                        first = s < first ? s : first;
                        last = s > last ? s : last;
                    }
                    wave_sync();
                }
            }
            first = sgp::wave_min(first);
            last = sgp::wave_max(last);
            next = sgp::wave_min(next);
            for (int base = first & ~(WAVE - 1); base <= last; base += WAVE) {  // the flag scan; base + lane < BAND
                const int s = base + lane;
                const float v = acc[s];
                const bool keep = hit[s] && !(v == 0.f);
                acc[s] = 0.f;
                hit[s] = 0;
                int total;
                const int rank = sgp::wave_rank(keep, total);
                if (EMIT && keep) {
                    const long long at = out + kept + rank;
                    if (at < end) { col[at] = (int)(lo + s); val[at] = v; }
                }
                kept += total;
            }
            wave_sync();
            if (next == NO_COLUMN) break;
            lo = next / BAND * BAND;                                            // next < B.cols: a column of a later band
        }
        if (!EMIT && lane == 0) counts[i] = (int)kept;                          // kept <= B.cols < 2^31
        if (bad) atomicOr(err, SGP_SPGEMM_ERR_INDEX);
    }
}

// ONE workgroup: counts -> rowptr (the entries of the rows before, at most `capacity`), rowptr[n] = *nnz
__global__ __launch_bounds__(SCAN_THREADS) void row_scan_kernel(const int* __restrict__ counts, long long n, long long capacity,
                                                                int* __restrict__ rowptr, int* nnz, int* err) {
    __shared__ long long sums[1][SCAN_THREADS];
    long long tot[1];
    sgp::wg_exclusive_scan<SCAN_THREADS, 1>(
        n, sums, [=](long long i, long long (&v)[1]) { const int c = counts[i]; v[0] = c < 0 ? 0 : c; },
        [=](long long i, const long long (&run)[1]) { rowptr[i] = (int)(run[0] < capacity ? run[0] : capacity); }, tot);
    if (threadIdx.x == 0) {
        const int total = (int)(tot[0] < capacity ? tot[0] : capacity);
        rowptr[n] = total;
        *nnz = total;
        if (tot[0] > capacity) atomicOr(err, SGP_SPGEMM_ERR_CAPACITY);
    }
}

__device__ __forceinline__ long long load_id(const void* p, int is64, long long at) {
    return is64 ? static_cast<const long long*>(p)[at] : (long long)static_cast<const int*>(p)[at];
}

__global__ __launch_bounds__(256) void take_lengths_kernel(Csr A, const void* index, int idx64, long long n_index,
                                                           int* __restrict__ counts, int* err) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n_index; t += (long long)gridDim.x * blockDim.x) {
        const long long r = load_id(index, idx64, t);
        long long lo = 0, hi = 0;
        if (!in_range(r, A.rows) || !row_span(A, r, lo, hi)) atomicOr(err, SGP_SPGEMM_ERR_INDEX);
        counts[t] = in_range(r, A.rows) ? (int)(hi - lo) : 0;
    }
}

__global__ __launch_bounds__(COPY_THREADS) void take_copy_kernel(Csr A, const void* index, int idx64, long long n_index,
                                                                 const int* __restrict__ rowptr, int* __restrict__ col,
                                                                 float* __restrict__ val, long long capacity) {
    const int lane = threadIdx.x & (WAVE - 1);
    const long long wave = blockIdx.x * (long long)(COPY_THREADS / WAVE) + (threadIdx.x >> 6);
    for (long long t = wave; t < n_index; t += (long long)gridDim.x * (COPY_THREADS / WAVE)) {
        const long long r = load_id(index, idx64, t);
        if (!in_range(r, A.rows)) continue;
        long long lo, hi;
        row_span(A, r, lo, hi);
        const long long p = rowptr[t], q = rowptr[t + 1];
        const long long out = p < 0 ? 0 : (p > capacity ? capacity : p);
        const long long end = q < out ? out : (q > capacity ? capacity : q);
        const long long len = hi - lo < end - out ? hi - lo : end - out;
        for (long long e = lane; e < len; e += WAVE) { col[out + e] = A.col[lo + e]; val[out + e] = A.val[lo + e]; }
    }
}

bool good_sizes(long long rows, long long cols) { return rows >= 0 && rows < MAX_ITEMS && cols >= 0 && cols < MAX_ITEMS; }

}  // namespace

extern "C" {

int64_t sgp_spgemm_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0 || n_rows >= MAX_ITEMS) return -1;
    return align256(4 * (n_rows > 0 ? n_rows : 1));
}

int sgp_spgemm_form(int64_t n_rows, int64_t n_cols, int64_t* out) {
    SGP_REQUIRE(out, "sgp_spgemm_form: null pointer");
    SGP_REQUIRE(good_sizes(n_rows, n_cols), "sgp_spgemm_form: bad size (%lld rows, %lld columns)", (long long)n_rows,
                (long long)n_cols);
    const long long bands = (n_cols + BAND - 1) / BAND;
    out[0] = BAND;
    out[1] = bands;
    out[2] = !n_rows || !n_cols ? 0 : (bands == 1 ? 1 : 2);
    out[3] = n_rows ? grid_for(n_rows, 1) : 0;
    return 0;
}

int sgp_spgemm_f32(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val, int64_t a_capacity, int64_t n_rows,
                   int64_t n_mid, const int32_t* b_rowptr, const int32_t* b_col, const float* b_val, int64_t b_capacity,
                   int64_t n_cols, int32_t phase, int32_t* rowptr, int32_t* col, float* val, int64_t capacity,
                   int32_t* nnz, int32_t* err, void* ws, int64_t ws_bytes, sgp_stream_t stream) {
    const char* what = "sgp_spgemm_f32";
    SGP_REQUIRE(a_rowptr && a_col && a_val && b_rowptr && b_col && b_val && rowptr && nnz && err && ws, "%s: null pointer", what);
    SGP_REQUIRE(phase >= 1 && phase <= 3, "%s: phase is SGP_SPGEMM_COUNT, SGP_SPGEMM_EMIT or both", what);
    SGP_REQUIRE(good_sizes(n_rows, n_cols) && n_mid >= 0 && n_mid < MAX_ITEMS, "%s: bad size", what);
    SGP_REQUIRE(a_capacity >= 1 && a_capacity <= MAX_ITEMS && b_capacity >= 1 && b_capacity <= MAX_ITEMS,
                "%s: operand capacity outside [1, 2^31)", what);
    const bool emit = (phase & SGP_SPGEMM_EMIT) != 0;
    if (emit) {
        SGP_REQUIRE(col && val, "%s: null pointer", what);
        SGP_REQUIRE(capacity >= 0 && capacity <= MAX_ITEMS, "%s: capacity %lld outside [0, 2^31)", what, (long long)capacity);
    }
    SGP_REQUIRE(ws_bytes >= sgp_spgemm_workspace_bytes(n_rows), "%s: workspace of %lld bytes, %lld needed", what,
                (long long)ws_bytes, (long long)sgp_spgemm_workspace_bytes(n_rows));
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "%s: misaligned workspace", what);
    hipStream_t s = (hipStream_t)stream;
    int* counts = static_cast<int*>(ws);
    const Csr A{a_rowptr, a_col, a_val, n_rows, n_mid, a_capacity}, B{b_rowptr, b_col, b_val, n_mid, n_cols, b_capacity};
    const long long cap = emit ? (long long)capacity : MAX_ITEMS;
    const unsigned grid = grid_for(n_rows, 1);
    if (phase & SGP_SPGEMM_COUNT)
        hipLaunchKernelGGL(product_kernel<false>, dim3(grid), dim3(WAVE), 0, s, A, B, counts, (const int*)nullptr,
                           (int*)nullptr, (float*)nullptr, 0ll, err);
    hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)counts, (long long)n_rows, cap, rowptr,
                       nnz, err);
    if (emit)
        hipLaunchKernelGGL(product_kernel<true>, dim3(grid), dim3(WAVE), 0, s, A, B, (int*)nullptr, (const int*)rowptr, col,
                           val, cap, err);
    return sgp::check_launch(what);
}

int sgp_csr_take_rows_f32(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val, int64_t a_capacity,
                          int64_t n_rows, const void* index, int32_t idx64, int64_t n_index, int32_t phase,
                          int32_t* rowptr, int32_t* col, float* val, int64_t capacity, int32_t* nnz, int32_t* err, void* ws,
                          int64_t ws_bytes, sgp_stream_t stream) {
    const char* what = "sgp_csr_take_rows_f32";
    SGP_REQUIRE(a_rowptr && a_col && a_val && rowptr && nnz && err && ws, "%s: null pointer", what);
    SGP_REQUIRE(phase >= 1 && phase <= 3, "%s: phase is SGP_SPGEMM_COUNT, SGP_SPGEMM_EMIT or both", what);
    SGP_REQUIRE(idx64 == 0 || idx64 == 1, "%s: idx64 is 0 or 1", what);
    SGP_REQUIRE(good_sizes(n_rows, n_index), "%s: bad size", what);
    SGP_REQUIRE(a_capacity >= 1 && a_capacity <= MAX_ITEMS, "%s: operand capacity outside [1, 2^31)", what);
    SGP_REQUIRE(!n_index || index, "%s: null pointer", what);
    const bool emit = (phase & SGP_SPGEMM_EMIT) != 0;
    if (emit) {
        SGP_REQUIRE(col && val, "%s: null pointer", what);
        SGP_REQUIRE(capacity >= 0 && capacity <= MAX_ITEMS, "%s: capacity %lld outside [0, 2^31)", what, (long long)capacity);
    }
    SGP_REQUIRE(ws_bytes >= sgp_spgemm_workspace_bytes(n_index), "%s: workspace of %lld bytes, %lld needed", what,
                (long long)ws_bytes, (long long)sgp_spgemm_workspace_bytes(n_index));
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "%s: misaligned workspace", what);
    hipStream_t s = (hipStream_t)stream;
    int* counts = static_cast<int*>(ws);
    const Csr A{a_rowptr, a_col, a_val, n_rows, 0, a_capacity};
    const long long cap = emit ? (long long)capacity : MAX_ITEMS;
    if (phase & SGP_SPGEMM_COUNT)
        hipLaunchKernelGGL(take_lengths_kernel, dim3(grid_for(n_index, 256)), dim3(256), 0, s, A, index, (int)idx64,
                           (long long)n_index, counts, err);
    hipLaunchKernelGGL(row_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)counts, (long long)n_index, cap, rowptr,
                       nnz, err);
    if (emit)
        hipLaunchKernelGGL(take_copy_kernel, dim3(grid_for(n_index, COPY_THREADS / WAVE)), dim3(COPY_THREADS), 0, s, A, index,
                           (int)idx64, (long long)n_index, (const int*)rowptr, col, val, cap);
    return sgp::check_launch(what);
}

}  // extern "C"
