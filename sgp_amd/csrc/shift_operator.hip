// The graph-shift operator of an edge list, built on the device: what ShiftOperator.from_edges /
// from_coo (sgp_amd/graph.py) build on the host, bit for bit, without a trip there.
//
//   prepare    item i -> (row, column) as int32 keys: the target and the source of edge i, swapped by `transpose`, and
//              for `undirected` the swapped list behind the original one.  An endpoint outside [0, n) (compared
//              unsigned, before it indexes anything) sets the error word and gives the item the key -1, which the sort
//              drops.
//   sort       two chained sgp_edge_sort passes: by column, then by row through the first order.  Stable: equal
//              (row, column) keep their list order.
//   gather     the sorted (row, column, weight) triples, contiguous.
//   count      kept run heads per tile of 4096 sorted items (a head: the first item of a run of equal (row, column);
//              kept: not on the diagonal when set_diag / remove_diag drop it)
//   scan       ONE workgroup: exclusive scan of the tile counts, the total, *nnz
//   emit       per tile: the scan of the head flags inside the tile; a kept head adds its run one weight after the
//              other from +0.0f (the host's zeros().index_add_) and writes the entry.  With set_diag row r's entries
//              sit r places further on, and one more behind its diagonal.
//   rows       one thread per row: rowptr, the diagonal entry of set_diag at its sorted place, the degree (the row's
//              values added in column order from +0.0f) and d = 1 / deg or 1 / sqrt(deg), +inf -> 0
//   normalise  one thread per entry: val = d[row] * val (* d[column])
// Integer arithmetic decides every position and every float sum has one order, so two runs give identical arrays.  No
// workgroup waits for another.  Every position read from the device (an order entry, a ptr entry, a scan value) is
// compared with the size of what it indexes first.
#include "wg.h"

#pragma clang fp contract(off)

namespace {
using sgp::grid_for;
using sgp::in_range;

constexpr int THREADS = 256;
constexpr int TILE = 4096;                        // sorted items per tile of the head scan (the sort's tile)
constexpr int SCAN_THREADS = 1024;
constexpr long long MAX_ITEMS = 2147483647ll;

inline long long align256(long long b) { return (b + 255) & ~255ll; }
inline long long tiles_for(long long items) { return items > 0 ? (items + TILE - 1) / TILE : 1; }

// workspace: the sort's | row keys (later: pos) | column keys | order by column | order by (row, column) | sorted rows |
// sorted columns | sorted weights | ptr [n + 1] | d [n] | tile counts [tiles + 1] (the last one: the total)
struct Layout {
    long long sort, rowk, colk, order1, order2, srow, scol, sw, ptr, d, tiles, bytes;
    Layout(long long n_items, long long n_nodes) {
        const long long per = align256(4 * (n_items > 0 ? n_items : 1));
        sort = 0;
        rowk = align256(sgp_edge_sort_workspace_bytes(n_items));
        colk = rowk + per; order1 = colk + per; order2 = order1 + per; srow = order2 + per; scol = srow + per;
        sw = scol + per;
        ptr = sw + per;
        d = ptr + align256(4 * (n_nodes + 1));
        tiles = d + align256(4 * (n_nodes > 0 ? n_nodes : 1));
        bytes = tiles + align256(4 * (tiles_for(n_items) + 1));
    }
};

__device__ __forceinline__ long long load_id(const void* p, int is64, long long at) {
    return is64 ? static_cast<const long long*>(p)[at] : (long long)static_cast<const int*>(p)[at];
}

__global__ __launch_bounds__(256) void prepare_kernel(const void* src, const void* dst, int idx64, long long n_edges,
                                                      long long n_items, long long n, int transpose,
                                                      int* __restrict__ rowk, int* __restrict__ colk, int* err) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n_items; i += (long long)gridDim.x * blockDim.x) {
        const bool second = i >= n_edges;                                       // the swapped half of `undirected`
        const long long e = second ? i - n_edges : i;
        const long long s = load_id(src, idx64, e), t = load_id(dst, idx64, e);
        const bool ok = in_range(s, n) && in_range(t, n);
        const bool swap = (transpose != 0) != second;
        if (!ok) *err = 1;
        rowk[i] = !ok ? -1 : (int)(swap ? s : t);
        colk[i] = !ok ? -1 : (int)(swap ? t : s);
    }
}

// the number of sorted items: what the second sort kept
__device__ __forceinline__ long long sorted_items(const int* __restrict__ ptr, long long n, long long n_items) {
    const long long t = ptr[n];
    return t < 0 ? 0 : (t > n_items ? n_items : t);
}

__global__ __launch_bounds__(256) void gather_kernel(const int* __restrict__ order1, const int* __restrict__ order2,
                                                     const int* __restrict__ rowk, const int* __restrict__ colk,
                                                     const float* __restrict__ w, long long n_edges, long long n_items,
                                                     long long n, const int* __restrict__ ptr, int* __restrict__ srow,
                                                     int* __restrict__ scol, float* __restrict__ sw) {
    const long long T = sorted_items(ptr, n, n_items);
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < T; p += (long long)gridDim.x * blockDim.x) {
        const int o2 = order2[p];
        const int o = in_range(o2, n_items) ? order1[o2] : -1;
        const bool ok = in_range(o, n_items);
        srow[p] = ok ? rowk[o] : -1;
        scol[p] = ok ? colk[o] : -1;
        sw[p] = !ok ? 0.f : (w ? w[o < n_edges ? o : o - n_edges] : 1.f);
    }
}

struct Sorted {
    const int* row;
    const int* col;
    long long T, n;
    int drop_diag;
};

// sorted item p starts a run of equal (row, column) that becomes an entry
__device__ __forceinline__ bool kept_head(const Sorted& s, long long p) {
    const int r = s.row[p], c = s.col[p];
    if (!in_range(r, s.n) || !in_range(c, s.n)) return false;
    if (s.drop_diag && r == c) return false;
    return p == 0 || s.row[p - 1] != r || s.col[p - 1] != c;
}

__global__ __launch_bounds__(THREADS) void count_kernel(const int* __restrict__ srow, const int* __restrict__ scol,
                                                        long long n_items, long long n, const int* __restrict__ ptr,
                                                        int drop_diag, long long n_tiles, int* __restrict__ tile_count) {
    __shared__ int sh[THREADS];
    const Sorted s{srow, scol, sorted_items(ptr, n, n_items), n, drop_diag};
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // block-uniform
        int mine = 0;
        for (int r = 0; r < TILE / THREADS; ++r) {
            const long long p = tile * TILE + r * THREADS + threadIdx.x;
            if (p < s.T && kept_head(s, p)) ++mine;
        }
        const int total = sgp::wg_reduce<THREADS>(mine, sh, [](int a, int b) { return a + b; });
        if (threadIdx.x == 0) tile_count[tile] = total;
    }
}

// ONE workgroup: tile_count -> the kept heads of the tiles before (in place), tile_count[n_tiles] = all of them
__global__ __launch_bounds__(SCAN_THREADS) void tile_scan_kernel(int* tile_count, long long n_tiles, long long n, int set_diag,
                                                                 int* nnz) {
    __shared__ int sums[1][SCAN_THREADS];
    int tot[1];
    sgp::wg_exclusive_scan<SCAN_THREADS, 1>(
        n_tiles, sums, [=](long long i, int (&v)[1]) { v[0] = tile_count[i]; },
        [=](long long i, const int (&run)[1]) { tile_count[i] = run[0]; }, tot);
    if (threadIdx.x == 0) {
        tile_count[n_tiles] = tot[0];
        *nnz = (int)(tot[0] + (set_diag ? n : 0));
    }
}

__global__ __launch_bounds__(THREADS) void emit_kernel(const int* __restrict__ srow, const int* __restrict__ scol,
                                                       const float* __restrict__ sw, long long n_items, long long n,
                                                       const int* __restrict__ ptr, int drop_diag, int set_diag,
                                                       long long n_tiles, const int* __restrict__ tile_base,
                                                       int* __restrict__ pos, int* __restrict__ col, float* __restrict__ val,
                                                       long long capacity) {
    __shared__ int sums[1][THREADS];
    const Sorted s{srow, scol, sorted_items(ptr, n, n_items), n, drop_diag};
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // block-uniform
        const long long start = tile * TILE;
        const long long count = s.T - start < TILE ? s.T - start : TILE;
        if (count <= 0) break;                                                  // (block-uniform; later tiles hold nothing either)
        const int base = tile_base[tile];
        int tot[1];
        sgp::wg_exclusive_scan<THREADS, 1>(
            count, sums, [=](long long i, int (&v)[1]) { v[0] = kept_head(s, start + i) ? 1 : 0; },
            [=](long long i, const int (&run)[1]) {
                const long long p = start + i;
                pos[p] = base + run[0];
                if (!kept_head(s, p)) return;
                const int r = s.row[p], c = s.col[p];
                const long long at = (long long)base + run[0] + (set_diag ? (long long)r + (c > r ? 1 : 0) : 0);
                if (!in_range(at, capacity)) return;
                float sum = 0.f;                                                // the head adds its run, in list order
                for (long long q = p; q < s.T && s.row[q] == r && s.col[q] == c; ++q) sum += sw[q];
                col[at] = c;
                val[at] = sum;
            }, tot);
        __syncthreads();                                                        // `sums` before the next tile's scan
    }
}

// kept heads below sorted position p (p <= T)
__device__ __forceinline__ long long heads_below(const int* __restrict__ pos, const int* __restrict__ total, long long p,
                                                 long long T) {
    return p < T ? pos[p] : *total;
}

__global__ __launch_bounds__(256) void rows_kernel(const int* __restrict__ ptr, const int* __restrict__ scol,
                                                   const int* __restrict__ pos, const int* __restrict__ total,
                                                   long long n_items, long long n, int set_diag, int gcn_norm,
                                                   int* __restrict__ rowptr, int* col, float* val, long long capacity,
                                                   float* __restrict__ d) {
    const long long T = sorted_items(ptr, n, n_items);
    for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k <= n; k += (long long)gridDim.x * blockDim.x) {
        long long p0 = ptr[k];
        p0 = p0 < 0 ? 0 : (p0 > T ? T : p0);
        const long long h0 = heads_below(pos, total, p0, T);
        long long e0 = h0 + (set_diag ? k : 0);
        rowptr[k] = (int)e0;
        if (k == n) break;
        long long p1 = ptr[k + 1];
        p1 = p1 < p0 ? p0 : (p1 > T ? T : p1);
        long long e1 = heads_below(pos, total, p1, T) + (set_diag ? k + 1 : 0);
        if (set_diag) {                                                         // behind the row's entries left of the diagonal
            long long lo = p0, hi = p1;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if (scol[mid] < k) lo = mid + 1; else hi = mid;
            }
            const long long at = e0 + (heads_below(pos, total, lo, T) - h0);
            if (in_range(at, capacity)) { col[at] = (int)k; val[at] = 1.f; }
        }
        if (e0 < 0) e0 = 0;
        if (e1 > capacity) e1 = capacity;
        float deg = 0.f;
        for (long long e = e0; e < e1; ++e) deg += val[e];
        float inv = gcn_norm ? 1.f / sqrtf(deg) : 1.f / deg;                     // IEEE division and square root
        if (inv == __builtin_inff()) inv = 0.f;
        d[k] = inv;
    }
}

__global__ __launch_bounds__(256) void normalise_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                        float* __restrict__ val, const float* __restrict__ d, long long n,
                                                        long long capacity, int gcn_norm) {
    long long nnz = rowptr[n];
    if (nnz > capacity) nnz = capacity;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < nnz; e += (long long)gridDim.x * blockDim.x) {
        long long lo = 0, hi = n;                                               // the last row that starts at or before e
        while (lo < hi) {
            const long long mid = (lo + hi) >> 1;
            if (rowptr[mid + 1] <= e) lo = mid + 1; else hi = mid;
        }
        if (lo >= n) continue;
        float v = d[lo] * val[e];
        if (gcn_norm) {
            const int c = col[e];
            v = v * (in_range(c, n) ? d[c] : 0.f);
        }
        val[e] = v;
    }
}

}  // namespace

extern "C" {

int64_t sgp_shift_operator_workspace_bytes(int64_t n_items, int64_t n_nodes) {
    if (n_items < 0 || n_items > MAX_ITEMS || n_nodes < 0 || n_nodes >= MAX_ITEMS) return -1;
    return Layout(n_items, n_nodes).bytes;
}

int sgp_shift_operator_f32(const void* src, const void* dst, int32_t idx64, const float* weight, int64_t n_edges,
                           int64_t n_nodes, int32_t flags, int32_t* rowptr, int32_t* col, float* val, int64_t capacity,
                           int32_t* nnz, int32_t* err, void* ws, int64_t ws_bytes, sgp_stream_t stream) {
    SGP_REQUIRE(rowptr && col && val && nnz && err && ws, "sgp_shift_operator_f32: null pointer");
    SGP_REQUIRE(idx64 == 0 || idx64 == 1, "sgp_shift_operator_f32: idx64 is 0 or 1");
    SGP_REQUIRE(flags >= 0 && flags < 32, "sgp_shift_operator_f32: unknown flag bits %d", (int)flags);
    SGP_REQUIRE(n_edges >= 0 && n_edges <= MAX_ITEMS && n_nodes >= 0 && n_nodes < MAX_ITEMS,
                "sgp_shift_operator_f32: bad size");
    const int gcn_norm = (flags & SGP_SHIFT_GCN_NORM) != 0, set_diag = (flags & SGP_SHIFT_SET_DIAG) != 0;
    const int drop_diag = set_diag || (flags & SGP_SHIFT_REMOVE_DIAG) != 0;
    const int transpose = (flags & SGP_SHIFT_TRANSPOSE) != 0;
    const long long n_items = (flags & SGP_SHIFT_UNDIRECTED) ? 2 * (long long)n_edges : (long long)n_edges;
    const long long need = n_items + (set_diag ? (long long)n_nodes : 0);
    SGP_REQUIRE(n_items <= MAX_ITEMS && need <= MAX_ITEMS, "sgp_shift_operator_f32: %lld entries do not fit 32-bit positions", need);
    SGP_REQUIRE(capacity >= need && capacity >= 1 && capacity <= MAX_ITEMS,
                "sgp_shift_operator_f32: capacity %lld, %lld needed", (long long)capacity, need > 1 ? need : 1);
    SGP_REQUIRE(!n_edges || (src && dst), "sgp_shift_operator_f32: null pointer");
    const Layout L(n_items, n_nodes);
    SGP_REQUIRE(ws_bytes >= L.bytes, "sgp_shift_operator_f32: workspace of %lld bytes, %lld needed", (long long)ws_bytes, L.bytes);
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 3u) == 0, "sgp_shift_operator_f32: misaligned workspace");
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ws);
    auto ints = [&](long long off) { return reinterpret_cast<int*>(base + off); };
    int *rowk = ints(L.rowk), *colk = ints(L.colk), *order1 = ints(L.order1), *order2 = ints(L.order2);
    int *srow = ints(L.srow), *scol = ints(L.scol), *ptr = ints(L.ptr), *tile_count = ints(L.tiles);
    float* sw = reinterpret_cast<float*>(base + L.sw);
    float* d = reinterpret_cast<float*>(base + L.d);
    int* pos = rowk;                                                            // the row keys are dead once gathered
    const long long n = n_nodes, n_tiles = tiles_for(n_items);
    if (!n_items) {
        hipError_t e = hipMemsetAsync(ptr, 0, (size_t)(n + 1) * 4, s);
        if (e != hipSuccess) return sgp::fail((int)e, "sgp_shift_operator_f32: %s", hipGetErrorString(e));
    } else {
        hipLaunchKernelGGL(prepare_kernel, dim3(grid_for(n_items, 256)), dim3(256), 0, s, src, dst, (int)idx64,
                           (long long)n_edges, n_items, n, transpose, rowk, colk, err);
        const int64_t sort_bytes = sgp_edge_sort_workspace_bytes(n_items);
        int rc = sgp_edge_sort(colk, 0, n_items, nullptr, n_items, n_nodes, order1, ptr, err, base + L.sort, sort_bytes, stream);
        if (rc) return rc;
        rc = sgp_edge_sort(rowk, 0, n_items, order1, n_items, n_nodes, order2, ptr, err, base + L.sort, sort_bytes, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(gather_kernel, dim3(grid_for(n_items, 256)), dim3(256), 0, s, (const int*)order1, (const int*)order2,
                           (const int*)rowk, (const int*)colk, weight, (long long)n_edges, n_items, n, (const int*)ptr, srow,
                           scol, sw);
    }
    hipLaunchKernelGGL(count_kernel, dim3(grid_for(n_tiles, 1)), dim3(THREADS), 0, s, (const int*)srow, (const int*)scol, n_items,
                       n, (const int*)ptr, drop_diag, n_tiles, tile_count);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, tile_count, n_tiles, n, set_diag, nnz);
    hipLaunchKernelGGL(emit_kernel, dim3(grid_for(n_tiles, 1)), dim3(THREADS), 0, s, (const int*)srow, (const int*)scol,
                       (const float*)sw, n_items, n, (const int*)ptr, drop_diag, set_diag, n_tiles, (const int*)tile_count, pos,
                       col, val, (long long)capacity);
    hipLaunchKernelGGL(rows_kernel, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, (const int*)ptr, (const int*)scol,
                       (const int*)pos, (const int*)(tile_count + n_tiles), n_items, n, set_diag, gcn_norm, rowptr, col, val,
                       (long long)capacity, d);
    hipLaunchKernelGGL(normalise_kernel, dim3(grid_for(capacity, 256)), dim3(256), 0, s, (const int*)rowptr, (const int*)col, val,
                       (const float*)d, n, (long long)capacity, gcn_norm);
    return sgp::check_launch("sgp_shift_operator_f32");
}

}  // extern "C"
