// Per-batch edge tables on the device: a stable sort of an edge list by node and the tables the models
// derive from it -- CSR (rowptr, col, val) of the diffusion supports, the chunk tables of the gated graph network --
// built on the stream, without a trip to the host.
//
// Stable key sort = LSD radix sort, 8-bit digits, ceil(bits(n - 1) / 8) passes; a pass is three launches on one stream
// and no workgroup waits for another (the rule of 9f's compaction):
//   histogram  one tile of 4096 items per workgroup: digit counts in LDS -> tile_hist[digit][tile] (digit-major), and
//              the workgroup's sums of them -> totals[digit] (integer atomics: the sum does not depend on the order)
//   scan       workgroup d: base = totals[0 .. d) summed, then the exclusive scan of row d of tile_hist in place
//   scatter    per tile, 16 rounds of 256 items in list order: every wave matches its lanes by ballots on the 8 digit
//              bits (rank in wave = lanes below with the same digit), the lowest lane of a group leaves the group's size
//              in the wave's counter row in LDS, thread d scans counter d over the 4 waves in wave order onto its
//              running offset, and every item goes to offset + rank.  Items of one digit keep their list order.
// Integer arithmetic only: the result is unique and two runs are identical.  A key outside [0, n) (compared unsigned,
// before it indexes anything) sets the error word and is dropped in the first histogram AND the first scatter: the
// later passes and ptr see the `valid` items that remain (a device word), the tail of `order` stays unwritten, and
// every consumer below checks order[e] against the list length before it indexes with it.
#include "wg.h"

namespace {
using sgp::grid_for;
using sgp::in_range;

constexpr int THREADS = 256;                      // 4 waves
constexpr int WAVES = THREADS / 64;
constexpr int ITEMS = 16;                         // rounds of a tile
constexpr int TILE = THREADS * ITEMS;             // 4096 items
constexpr int RADIX = 256;
constexpr int MAX_PASSES = 4;
constexpr long long MAX_ITEMS = 2147483647ll;
constexpr int SCAN_THREADS = 1024;

static_assert(RADIX == THREADS, "thread d owns digit d");

inline long long align256(long long b) { return (b + 255) & ~255ll; }

inline int passes_for(long long n) {
    int p = 1;
    while (p < MAX_PASSES && n > 1 && ((n - 1) >> (8 * p))) ++p;
    return p;
}

inline long long tiles_for(long long items) { return items > 0 ? (items + TILE - 1) / TILE : 1; }

// workspace: keys A | keys B | payload A | payload B (n_items int32 each) | tile_hist [256][tiles] | totals
// [MAX_PASSES][256] and the `valid` word behind them
struct Layout {
    long long keys[2], pay[2], hist, totals, bytes;
    Layout(long long n_items, long long n_tiles) {
        const long long per = align256(4 * (n_items > 0 ? n_items : 1));
        keys[0] = 0; keys[1] = per; pay[0] = 2 * per; pay[1] = 3 * per;
        hist = 4 * per;
        totals = hist + align256(4ll * RADIX * n_tiles);
        bytes = totals + align256(4ll * (MAX_PASSES * RADIX + 1));
    }
};

// MODE 0 / 1: the caller's int32 / int64 keys (first pass; read through `via` when given), MODE 2: a pass's own buffers
struct SortIn {
    const void* keys;
    const int* via;
    long long n_keys;
    const int* bkeys;
    const int* bpay;
    const int* valid;                              // MODE 2: the number of items
};

template <int MODE>
__device__ __forceinline__ bool load_item(const SortIn& in, long long i, long long count, long long n, int* err, int& key,
                                          int& pay) {
    if (i >= count) return false;
    if (MODE == 2) { key = in.bkeys[i]; pay = in.bpay[i]; return true; }
    long long at = i;
    if (in.via) {
        const int p = in.via[i];
        if (!in_range(p, in.n_keys)) { *err = 1; return false; }
        at = p;
    }
    pay = (int)i;
    if (MODE == 1) {
        const long long k = static_cast<const long long*>(in.keys)[at];
        if (!in_range(k, n)) { *err = 1; return false; }
        key = (int)k;
    } else {
        const int k = static_cast<const int*>(in.keys)[at];
        if (!in_range(k, n)) { *err = 1; return false; }
        key = k;
    }
    return true;
}

// the lanes of this wave that hold the same digit as this one (valid lanes only; meaningless on the others)
__device__ __forceinline__ unsigned long long match_digit(int digit, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1;
        const unsigned long long bal = __ballot(valid && bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void hist_kernel(SortIn in, long long n_items, long long n, int shift,
                                                       long long n_tiles, int* __restrict__ tile_hist,
                                                       int* __restrict__ totals, int* err) {
    __shared__ int hist[RADIX];
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long count = MODE == 2 ? (long long)*in.valid : n_items;
    int mine = 0;                                                               // digit threadIdx.x over this workgroup's tiles
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // block-uniform
        hist[threadIdx.x] = 0;
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < ITEMS; ++r) {
            int key = 0, pay = 0;
            const bool ok = load_item<MODE>(in, tile * TILE + r * THREADS + threadIdx.x, count, n, err, key, pay);
            const int digit = (key >> shift) & (RADIX - 1);
            const unsigned long long m = match_digit(digit, ok);
            if (ok && !(m & below)) atomicAdd(&hist[digit], __popcll(m));
        }
        __syncthreads();
        const int h = hist[threadIdx.x];
        tile_hist[threadIdx.x * n_tiles + tile] = h;
        mine += h;
        __syncthreads();
    }
    if (mine) atomicAdd(&totals[threadIdx.x], mine);
}

// workgroup d: exclusive scan of tile_hist[d][0 .. n_tiles) in place, started at the items of the digits below d
__global__ __launch_bounds__(THREADS) void digit_scan_kernel(int* tile_hist, long long n_tiles, const int* __restrict__ totals,
                                                             int* valid) {
    __shared__ int sums[1][THREADS];
    const int d = blockIdx.x;
    sums[0][threadIdx.x] = totals[threadIdx.x];
    __syncthreads();
    int base = 0;
    for (int k = 0; k < d; ++k) base += sums[0][k];
    if (valid && d == RADIX - 1 && threadIdx.x == 0) *valid = base + sums[0][RADIX - 1];
    __syncthreads();
    int* row = tile_hist + d * n_tiles;
    int tot[1];
    sgp::wg_exclusive_scan<THREADS, 1>(
        n_tiles, sums, [=](long long i, int (&v)[1]) { v[0] = row[i]; },
        [=](long long i, const int (&run)[1]) { row[i] = base + run[0]; }, tot);
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void scatter_kernel(SortIn in, long long n_items, long long n, int shift,
                                                          long long n_tiles, const int* __restrict__ tile_offsets,
                                                          int* __restrict__ out_keys, int* __restrict__ out_pay, int* err) {
    __shared__ int wcnt[WAVES][RADIX];                                          // a round's group sizes, else 0
    __shared__ int woff[WAVES][RADIX];                                          // where a wave's items of a digit start
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long count = MODE == 2 ? (long long)*in.valid : n_items;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) wcnt[w][threadIdx.x] = 0;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // block-uniform
        int key[ITEMS], pay[ITEMS];
        bool ok[ITEMS];
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            key[r] = 0; pay[r] = 0;
            ok[r] = load_item<MODE>(in, tile * TILE + r * THREADS + threadIdx.x, count, n, err, key[r], pay[r]);
        }
        int run = tile_offsets[threadIdx.x * n_tiles + tile];                   // where digit threadIdx.x of this tile goes next
        __syncthreads();                                                        // the zeroed counters (first tile)
#pragma unroll
        for (int r = 0; r < ITEMS; ++r) {
            const int digit = (key[r] >> shift) & (RADIX - 1);
            const unsigned long long m = match_digit(digit, ok[r]);
            if (ok[r] && !(m & below)) wcnt[wv][digit] = __popcll(m);           // the group's lowest lane
            __syncthreads();                                                    // also: every read of woff of the round before
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {                                   // wave order = list order
                const int c = wcnt[w][threadIdx.x];
                wcnt[w][threadIdx.x] = 0;
                woff[w][threadIdx.x] = run;
                run += c;
            }
            __syncthreads();
            if (ok[r]) {
                const long long pos = (long long)woff[wv][digit] + __popcll(m & below);
                out_keys[pos] = key[r];
                out_pay[pos] = pay[r];
            }
        }
        __syncthreads();                                                        // the last reads of woff before the next tile's
    }
}

// ptr[k] = the items with a key below k = the first position of the sorted list whose key is >= k
__global__ __launch_bounds__(256) void ptr_kernel(const int* __restrict__ sorted_keys, const int* __restrict__ valid,
                                                  long long n_items, long long n, int* __restrict__ ptr) {
    const long long count = valid ? (long long)*valid : n_items;
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k <= n; k += (long long)gridDim.x * blockDim.x) {
        long long lo = 0, hi = count;
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (sorted_keys[mid] < k) lo = mid + 1; else hi = mid;
        }
        ptr[k] = (int)lo;
    }
}

// deg[k] = w[order[ptr[k]]] + ... one after the other in list order, from 0: the host's scatter_add_ in edge order
__global__ __launch_bounds__(256) void segment_sum_kernel(const int* __restrict__ ptr, const int* __restrict__ order,
                                                          const float* __restrict__ w, long long n, long long n_items,
                                                          float* __restrict__ deg) {
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        long long e0 = ptr[k], e1 = ptr[k + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > n_items) e1 = n_items;
        float s = 0.f;
        for (long long e = e0; e < e1; ++e) {
            const int o = order[e];
            if (!in_range(o, n_items)) continue;
            s += w ? w[o] : 1.f;
        }
        deg[k] = s;
    }
}

__device__ __forceinline__ long long load_id(const void* p, int is64, long long at) {
    return is64 ? static_cast<const long long*>(p)[at] : (long long)static_cast<const int*>(p)[at];
}

// col[e] = other[o], val_x[e] = w[o] / deg_x[idx_x[o]] with o = order[e] (IEEE division; nothing here can be fused);
// deg_x NULL: val_x[e] = w[o]
__global__ __launch_bounds__(256) void gather_kernel(const int* __restrict__ order, long long n_items, const void* other,
                                                     int other64, const float* __restrict__ w, const void* idx_a,
                                                     const float* __restrict__ deg_a, const void* idx_b,
                                                     const float* __restrict__ deg_b, int idx64, long long n,
                                                     int* __restrict__ col, float* __restrict__ val_a,
                                                     float* __restrict__ val_b) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n_items;
         e += (long long)gridDim.x * blockDim.x) {
        const int o = order[e];
        const bool ok = in_range(o, n_items);
        if (col) col[e] = ok ? (int)load_id(other, other64, o) : 0;
        const float we = !ok ? 0.f : (w ? w[o] : 1.f);
        if (val_a && !deg_a) val_a[e] = we;
        else if (val_a) {
            const long long i = ok ? load_id(idx_a, idx64, o) : -1;
            val_a[e] = in_range(i, n) ? we / deg_a[i] : 0.f;
        }
        if (val_b && !deg_b) val_b[e] = we;
        else if (val_b) {
            const long long i = ok ? load_id(idx_b, idx64, o) : -1;
            val_b[e] = in_range(i, n) ? we / deg_b[i] : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------- chunk tables of the gated graph network
__device__ __forceinline__ int chunks_of(const int* __restrict__ ptr, long long k, int chunk) {
    const long long deg = (long long)ptr[k + 1] - ptr[k];
    const long long c = (deg + chunk - 1) / chunk;
    return c < 1 ? 1 : (int)c;
}

// ONE workgroup: per node the exclusive sums of (chunks, chunks of split targets, split targets) -> scan[3][n], the
// totals -> counts[0 .. 3) = (n_chunks, n_fix, n_parts)
__global__ __launch_bounds__(SCAN_THREADS) void chunk_scan_kernel(const int* __restrict__ ptr, long long n, int chunk,
                                                                  int* __restrict__ scan, int* counts) {
    __shared__ long long sums[3][SCAN_THREADS];
    long long tot[3];
    sgp::wg_exclusive_scan<SCAN_THREADS, 3>(
        n, sums,
        [=](long long k, long long (&v)[3]) {
            const int c = chunks_of(ptr, k, chunk);
            v[0] = c; v[1] = c > 1 ? c : 0; v[2] = c > 1 ? 1 : 0;
        },
        [=](long long k, const long long (&run)[3]) {
            scan[k] = (int)run[0]; scan[n + k] = (int)run[1]; scan[2 * n + k] = (int)run[2];
        }, tot);
    if (threadIdx.x == 0) { counts[0] = (int)tot[0]; counts[1] = (int)tot[2]; counts[2] = (int)tot[1]; }
}

// chunk row c belongs to the last node whose first chunk is <= c (every node has at least one chunk)
__global__ __launch_bounds__(256) void chunk_emit_kernel(const int* __restrict__ ptr, long long n, int chunk,
                                                         const int* __restrict__ scan, const int* __restrict__ counts,
                                                         long long max_chunks, long long max_fix, int* __restrict__ chunks,
                                                         int* __restrict__ fix) {
    long long total = counts[0];
    if (total > max_chunks) total = max_chunks;
    for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < total; c += (long long)gridDim.x * blockDim.x) {
        long long lo = 0, hi = n;                                               // first node with scan[node] > c
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (scan[mid] <= c) lo = mid + 1; else hi = mid;
        }
        const long long k = lo - 1;
        const long long j = c - scan[k];
        const int nch = chunks_of(ptr, k, chunk);
        const long long e0 = (long long)ptr[k] + j * chunk;
        const long long e1 = e0 + chunk < ptr[k + 1] ? e0 + chunk : ptr[k + 1];
        int* row = chunks + 4 * c;
        row[0] = (int)k;
        row[1] = (int)e0;
        row[2] = (int)e1;
        row[3] = nch > 1 ? (int)(scan[n + k] + j) : -1;
        if (nch > 1 && j == 0) {
            const long long f = scan[2 * n + k];
            if (f < max_fix) {
                fix[3 * f] = (int)k;
                fix[3 * f + 1] = scan[n + k];
                fix[3 * f + 2] = nch;
            }
        }
    }
}

template <int MODE>
void launch_pass(const SortIn& in, long long n_items, long long n, int shift, long long n_tiles, int* tile_hist,
                 int* totals, int* valid_out, int* out_keys, int* out_pay, int* err, hipStream_t s) {
    const unsigned grid = grid_for(n_tiles, 1);
    hipLaunchKernelGGL(hist_kernel<MODE>, dim3(grid), dim3(THREADS), 0, s, in, n_items, n, shift, n_tiles, tile_hist, totals,
                       err);
    hipLaunchKernelGGL(digit_scan_kernel, dim3(RADIX), dim3(THREADS), 0, s, tile_hist, n_tiles, (const int*)totals, valid_out);
    hipLaunchKernelGGL(scatter_kernel<MODE>, dim3(grid), dim3(THREADS), 0, s, in, n_items, n, shift, n_tiles,
                       (const int*)tile_hist, out_keys, out_pay, err);
}

}  // namespace

extern "C" {

int32_t sgp_edge_sort_tile(void) { return TILE; }

int32_t sgp_edge_sort_passes(int64_t n_nodes) {
    if (n_nodes < 0 || n_nodes > MAX_ITEMS) return -1;
    return passes_for(n_nodes);
}

int64_t sgp_edge_sort_workspace_bytes(int64_t n_items) {
    if (n_items < 0 || n_items > MAX_ITEMS) return -1;
    return Layout(n_items, tiles_for(n_items)).bytes;
}

int sgp_edge_sort(const void* keys, int32_t keys64, int64_t n_keys, const int32_t* payload_in, int64_t n_items,
                  int64_t n_nodes, int32_t* order, int32_t* ptr, int32_t* err, void* ws, int64_t ws_bytes,
                  sgp_stream_t stream) {
    SGP_REQUIRE(n_items >= 0 && n_items <= MAX_ITEMS && n_keys >= 0 && n_keys <= MAX_ITEMS && n_nodes >= 0 &&
                n_nodes < MAX_ITEMS, "sgp_edge_sort: bad size");
    SGP_REQUIRE(keys64 == 0 || keys64 == 1, "sgp_edge_sort: keys64 is 0 or 1");
    SGP_REQUIRE(payload_in || n_keys == n_items, "sgp_edge_sort: %lld keys for %lld items", (long long)n_keys, (long long)n_items);
    SGP_REQUIRE(ptr && err, "sgp_edge_sort: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (!n_items) {
        e = hipMemsetAsync(ptr, 0, (size_t)(n_nodes + 1) * 4, s);
        if (e != hipSuccess) return sgp::fail((int)e, "sgp_edge_sort: %s", hipGetErrorString(e));
        return 0;
    }
    SGP_REQUIRE(keys && order && ws, "sgp_edge_sort: null pointer");
    const long long n_tiles = tiles_for(n_items);
    const Layout L(n_items, n_tiles);
    SGP_REQUIRE(ws_bytes >= L.bytes, "sgp_edge_sort: workspace of %lld bytes, %lld needed", (long long)ws_bytes, L.bytes);
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "sgp_edge_sort: misaligned workspace");
    char* base = static_cast<char*>(ws);
    int* bkeys[2] = {reinterpret_cast<int*>(base + L.keys[0]), reinterpret_cast<int*>(base + L.keys[1])};
    int* bpay[2] = {reinterpret_cast<int*>(base + L.pay[0]), reinterpret_cast<int*>(base + L.pay[1])};
    int* tile_hist = reinterpret_cast<int*>(base + L.hist);
    int* totals = reinterpret_cast<int*>(base + L.totals);
    int* valid = totals + MAX_PASSES * RADIX;
    e = hipMemsetAsync(totals, 0, 4 * (MAX_PASSES * RADIX + 1), s);
    if (e != hipSuccess) return sgp::fail((int)e, "sgp_edge_sort: %s", hipGetErrorString(e));
    const int passes = passes_for(n_nodes);
    for (int p = 0; p < passes; ++p) {
        int* out_pay = p == passes - 1 ? order : bpay[p & 1];
        if (p == 0) {
            const SortIn in{keys, payload_in, (long long)n_keys, nullptr, nullptr, nullptr};
            if (keys64) launch_pass<1>(in, n_items, n_nodes, 0, n_tiles, tile_hist, totals, valid, bkeys[0], out_pay, err, s);
            else launch_pass<0>(in, n_items, n_nodes, 0, n_tiles, tile_hist, totals, valid, bkeys[0], out_pay, err, s);
        } else {
            const SortIn in{nullptr, nullptr, 0, bkeys[(p - 1) & 1], bpay[(p - 1) & 1], valid};
            launch_pass<2>(in, n_items, n_nodes, 8 * p, n_tiles, tile_hist, totals + p * RADIX, nullptr, bkeys[p & 1], out_pay,
                           err, s);
        }
    }
    hipLaunchKernelGGL(ptr_kernel, dim3(grid_for(n_nodes + 1, 256)), dim3(256), 0, s, (const int*)bkeys[(passes - 1) & 1],
                       (const int*)valid, (long long)n_items, (long long)n_nodes, ptr);
    return sgp::check_launch("sgp_edge_sort");
}

int sgp_edge_segment_sum_f32(const int32_t* ptr, const int32_t* order, const float* weight, int64_t n_nodes,
                             int64_t n_items, float* deg, sgp_stream_t stream) {
    SGP_REQUIRE(n_nodes >= 0 && n_nodes < MAX_ITEMS && n_items >= 0 && n_items <= MAX_ITEMS, "sgp_edge_segment_sum_f32: bad size");
    if (!n_nodes) return 0;
    SGP_REQUIRE(ptr && deg && (order || !n_items), "sgp_edge_segment_sum_f32: null pointer");
    hipLaunchKernelGGL(segment_sum_kernel, dim3(grid_for(n_nodes, 256)), dim3(256), 0, (hipStream_t)stream, ptr, order, weight,
                       (long long)n_nodes, (long long)n_items, deg);
    return sgp::check_launch("sgp_edge_segment_sum_f32");
}

int sgp_edge_gather_f32(const int32_t* order, int64_t n_items, const void* other, int32_t other64, const float* weight,
                        const void* idx_a, const float* deg_a, const void* idx_b, const float* deg_b, int32_t idx64,
                        int64_t n_nodes, int32_t* col, float* val_a, float* val_b, sgp_stream_t stream) {
    SGP_REQUIRE(n_items >= 0 && n_items <= MAX_ITEMS && n_nodes >= 0 && n_nodes < MAX_ITEMS, "sgp_edge_gather_f32: bad size");
    SGP_REQUIRE((other64 == 0 || other64 == 1) && (idx64 == 0 || idx64 == 1), "sgp_edge_gather_f32: a 64-bit flag is 0 or 1");
    if (!n_items) return 0;
    SGP_REQUIRE(order && (col || val_a || val_b), "sgp_edge_gather_f32: null pointer");
    SGP_REQUIRE(!col || other, "sgp_edge_gather_f32: col without other");
    SGP_REQUIRE((!val_a || !deg_a || idx_a) && (!val_b || !deg_b || idx_b), "sgp_edge_gather_f32: deg without idx");
    hipLaunchKernelGGL(gather_kernel, dim3(grid_for(n_items, 256)), dim3(256), 0, (hipStream_t)stream, order,
                       (long long)n_items, other, (int)other64, weight, idx_a, deg_a, idx_b, deg_b, (int)idx64,
                       (long long)n_nodes, col, val_a, val_b);
    return sgp::check_launch("sgp_edge_gather_f32");
}

int sgp_edge_chunk_tables(const int32_t* ptr, int64_t n_nodes, int32_t chunk, int32_t* scan, int32_t* counts,
                          int32_t* chunks, int64_t max_chunks, int32_t* fix, int64_t max_fix, sgp_stream_t stream) {
    SGP_REQUIRE(n_nodes >= 0 && n_nodes < MAX_ITEMS && chunk >= 1 && max_chunks >= 0 && max_chunks <= MAX_ITEMS &&
                max_fix >= 0 && max_fix <= MAX_ITEMS, "sgp_edge_chunk_tables: bad size");
    SGP_REQUIRE(counts, "sgp_edge_chunk_tables: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!n_nodes) {
        hipError_t e = hipMemsetAsync(counts, 0, 12, s);
        if (e != hipSuccess) return sgp::fail((int)e, "sgp_edge_chunk_tables: %s", hipGetErrorString(e));
        return 0;
    }
    SGP_REQUIRE(ptr && scan && chunks && (fix || !max_fix), "sgp_edge_chunk_tables: null pointer");
    hipLaunchKernelGGL(chunk_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, ptr, (long long)n_nodes, (int)chunk, scan, counts);
    hipLaunchKernelGGL(chunk_emit_kernel, dim3(grid_for(max_chunks, 256)), dim3(256), 0, s, ptr, (long long)n_nodes, (int)chunk,
                       (const int*)scan, (const int*)counts, (long long)max_chunks, (long long)max_fix, chunks, fix);
    return sgp::check_launch("sgp_edge_chunk_tables");
}

}  // extern "C"
