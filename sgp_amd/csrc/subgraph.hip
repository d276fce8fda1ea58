// k-hop subgraph extraction on the device: the reference's SubgraphLoader.collate
// (lib/dataloader/subgraph_dataloader.py:145-198) walks the whole edge list on the host once per hop with boolean
// masks, takes a `unique`, masks and relabels the edges and draws a `randperm` over them, for every batch.  Here the
// edge list stays in HBM as int32 and a batch is: mark the roots in a bit mask, one pass over the edges per hop
// (mask_in -> mask_out, two buffers), an ordered compaction of the node mask (sorted node ids + the relabel table), a
// pass that writes one flag BIT per edge, an ordered compaction of those flags, and a scatter of the relabelled
// endpoints.
//
// Ordered compaction = three launches on one stream, no workgroup waits for another:
//   count    one tile of 256 mask words (16 384 flags) per workgroup -> tile_counts[tile]
//   scan     ONE workgroup: exclusive scan of the tile counts in place, total to a device word
//   scatter  per tile: wave scan of the words' popcounts, then every word of a wave is broadcast in turn and lane l
//            takes bit l: rank = tile offset + words before + popcll(word & lanes below).  Consecutive lanes touch
//            consecutive indices, so the edge pass reads the edge list coalesced.
// Every flag array is a bit array in 64-bit words (the node mask itself is one); bits at and beyond n are ignored.
#include "wg.h"

namespace {
using sgp::grid_for;
using sgp::in_range;

typedef unsigned long long u64;

constexpr int TILE_WORDS = 256;          // words of one compaction tile = threads of its workgroup (4 waves)
constexpr int SCAN_THREADS = 1024;

__device__ __forceinline__ bool in_mask(const u64* __restrict__ mask, int v, long long n) {
    return in_range(v, n) && ((mask[(unsigned)v >> 6] >> (v & 63)) & 1ull);
}

// word w of an n-bit array with the bits at and beyond n cleared
__device__ __forceinline__ u64 load_word(const u64* __restrict__ bits, long long w, long long n_words, long long n) {
    if (w >= n_words) return 0ull;
    u64 x = bits[w];
    if (w == n_words - 1 && (n & 63)) x &= (1ull << (n & 63)) - 1ull;
    return x;
}

__global__ __launch_bounds__(256) void mark_kernel(const int* __restrict__ ids, long long n_ids, u64* mask, long long n,
                                                   int* err) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n_ids;
         i += (long long)gridDim.x * blockDim.x) {
        const int v = ids[i];
        if (in_range(v, n)) atomicOr(&mask[(unsigned)v >> 6], 1ull << (v & 63));
        else if (err) *err = 1;
    }
}

// mask_out |= { dst[e] : src[e] in mask_in }.  mask_in is only read and mask_out only OR-ed, so a node reached in this
// hop cannot expand in it.  The plain read of mask_out in front of the atomic drops the adds whose bit is already
// there (after the first few edges of a neighbourhood: most of them); a stale read only costs an atomic.
__global__ __launch_bounds__(256) void expand_kernel(const int* __restrict__ src, const int* __restrict__ dst,
                                                     long long n_edges, const u64* __restrict__ mask_in, u64* mask_out,
                                                     long long n) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n_edges;
         e += (long long)gridDim.x * blockDim.x) {
        if (!in_mask(mask_in, src[e], n)) continue;
        const int v = dst[e];
        if (!in_range(v, n)) continue;
        const u64 bit = 1ull << (v & 63);
        u64* word = &mask_out[(unsigned)v >> 6];
        if (!(*word & bit)) atomicOr(word, bit);
    }
}

// flags bit e = mask[src[e]] & mask[dst[e]]: one ballot and one 8-byte store per wave and 64 edges
__global__ __launch_bounds__(256) void edge_flags_kernel(const int* __restrict__ src, const int* __restrict__ dst,
                                                         long long n_edges, const u64* __restrict__ mask, long long n,
                                                         u64* __restrict__ flags, unsigned char* __restrict__ edge_mask) {
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long n_words = (n_edges + 63) >> 6;
    for (long long w = wave; w < n_words; w += n_waves) {                       // wave-uniform
        const long long e = w * 64 + lane;
        const bool keep = e < n_edges && in_mask(mask, src[e], n) && in_mask(mask, dst[e], n);
        const u64 word = __ballot(keep);
        if (lane == 0) flags[w] = word;
        if (edge_mask && e < n_edges) edge_mask[e] = keep ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void pack_u8_kernel(const unsigned char* __restrict__ f, long long n, u64* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const long long wave = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long n_words = (n + 63) >> 6;
    for (long long w = wave; w < n_words; w += n_waves) {
        const long long i = w * 64 + lane;
        const u64 word = __ballot(i < n && f[i] != 0);
        if (lane == 0) bits[w] = word;
    }
}

__global__ __launch_bounds__(TILE_WORDS) void count_kernel(const u64* __restrict__ bits, long long n, long long n_tiles,
                                                           int* __restrict__ tile_counts) {
    __shared__ int part[TILE_WORDS / 64];
    const long long n_words = (n + 63) >> 6;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // block-uniform
        const int c = sgp::wave_sum(__popcll(load_word(bits, tile * TILE_WORDS + threadIdx.x, n_words, n)));
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_counts[tile] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// exclusive scan of counts[0 .. n) in place by ONE workgroup (wg.h), the total to a device word.  n <= 2^17 for 2^31
// flags: 128 entries per thread.
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(int* counts, long long n, int* total) {
    __shared__ long long sums[1][SCAN_THREADS];
    long long tot[1];
    sgp::wg_exclusive_scan<SCAN_THREADS, 1>(
        n, sums, [=](long long i, long long (&v)[1]) { v[0] = counts[i]; },
        [=](long long i, const long long (&run)[1]) { counts[i] = (int)run[0]; }, tot);
    if (threadIdx.x == 0) *total = (int)tot[0];
}

// emit(i, r) for every set bit i of `bits`, r its exclusive rank, in ascending i within each wave's words
template <class Emit>
__device__ __forceinline__ void scatter_tiles(const u64* __restrict__ bits, long long n, long long n_tiles,
                                              const int* __restrict__ tile_offsets, Emit emit) {
    __shared__ int wave_tot[TILE_WORDS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long n_words = (n + 63) >> 6;
    const u64 below = (1ull << lane) - 1ull;
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // block-uniform
        const long long w0 = tile * TILE_WORDS + wv * 64;
        const u64 word = load_word(bits, w0 + lane, n_words, n);
        const int cnt = __popcll(word);
        int incl = cnt;                                                         // inclusive scan over the wave's 64 words
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        long long base = tile_offsets[tile];
        for (int k = 0; k < wv; ++k) base += wave_tot[k];
        __syncthreads();
        const int excl = incl - cnt;
        if (__shfl(incl, 63) == 0) continue;                                    // nothing set in this wave's words
        for (int j = 0; j < 64; ++j) {                                          // wave-uniform
            const u64 wj = __shfl(word, j);
            const int bj = __shfl(excl, j);
            if (wj == 0ull) continue;
            if ((wj >> lane) & 1ull) emit((w0 + j) * 64 + lane, base + bj + __popcll(wj & below));
        }
    }
}

__global__ __launch_bounds__(TILE_WORDS) void scatter_index_kernel(const u64* __restrict__ bits, long long n, long long n_tiles,
                                                                   const int* __restrict__ tile_offsets, long long cap,
                                                                   int* __restrict__ idx32, long long* __restrict__ idx64,
                                                                   int* __restrict__ rank) {
    scatter_tiles(bits, n, n_tiles, tile_offsets, [=](long long i, long long r) {
        if (rank) rank[i] = (int)r;
        if (r < cap) {
            if (idx32) idx32[r] = (int)i;
            if (idx64) idx64[r] = i;
        }
    });
}

__global__ __launch_bounds__(TILE_WORDS) void scatter_edges_kernel(const u64* __restrict__ flags, long long n_edges, long long n_tiles,
                                                                   const int* __restrict__ tile_offsets, long long cap,
                                                                   const int* __restrict__ src, const int* __restrict__ dst,
                                                                   const float* __restrict__ w, const int* __restrict__ relabel,
                                                                   long long n, long long* __restrict__ out_src,
                                                                   long long* __restrict__ out_dst, float* __restrict__ out_w) {
    scatter_tiles(flags, n_edges, n_tiles, tile_offsets, [=](long long e, long long r) {
        if (r >= cap) return;
        const int s = src[e], d = dst[e];
        const bool ok = in_range(s, n) && in_range(d, n);
        out_src[r] = ok ? relabel[s] : -1;
        out_dst[r] = ok ? relabel[d] : -1;
        if (out_w) out_w[r] = w[e];
    });
}

// out[j] = edge pos[keep[j]] relabelled: the reference's edge_index[:, keep_edges] on the surviving edges, in keep's order
__global__ __launch_bounds__(256) void take_edges_kernel(const int* __restrict__ src, const int* __restrict__ dst,
                                                         const float* __restrict__ w, long long n_edges,
                                                         const int* __restrict__ pos, long long n_pos,
                                                         const long long* __restrict__ keep, long long n_keep,
                                                         const int* __restrict__ relabel, long long n,
                                                         long long* __restrict__ out_src, long long* __restrict__ out_dst,
                                                         float* __restrict__ out_w, int* err) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n_keep;
         j += (long long)gridDim.x * blockDim.x) {
        const long long r = keep ? keep[j] : j;
        long long e = -1;
        if (r >= 0 && r < n_pos) e = pos ? (long long)pos[r] : r;
        int s = -1, d = -1;
        if (e >= 0 && e < n_edges) { s = src[e]; d = dst[e]; }
        const bool ok = in_range(s, n) && in_range(d, n);
        out_src[j] = ok ? (relabel ? relabel[s] : s) : -1;
        out_dst[j] = ok ? (relabel ? relabel[d] : d) : -1;
        if (out_w) out_w[j] = ok ? w[e] : 0.f;
        if (!ok && err) *err = 1;
    }
}

constexpr long long MAX_N = 2147483647ll;

}  // namespace

extern "C" {

int64_t sgp_compact_tiles(int64_t n) {
    if (n < 0 || n > MAX_N) return -1;
    const int64_t words = (n + 63) / 64;
    return (words + TILE_WORDS - 1) / TILE_WORDS;
}

int sgp_subgraph_mark(const int32_t* ids, int64_t n_ids, uint64_t* mask, int64_t n_nodes, int32_t* err,
                      sgp_stream_t stream) {
    SGP_REQUIRE(n_ids >= 0 && n_nodes >= 0 && n_nodes <= MAX_N, "sgp_subgraph_mark: bad size");
    if (!n_ids) return 0;
    SGP_REQUIRE(ids && mask, "sgp_subgraph_mark: null pointer");
    hipLaunchKernelGGL(mark_kernel, dim3(grid_for(n_ids, 256)), dim3(256), 0, (hipStream_t)stream, ids,
                       (long long)n_ids, (u64*)mask, (long long)n_nodes, err);
    return sgp::check_launch("sgp_subgraph_mark");
}

int sgp_subgraph_expand(const int32_t* src, const int32_t* dst, int64_t n_edges, const uint64_t* mask_in,
                        uint64_t* mask_out, int64_t n_nodes, sgp_stream_t stream) {
    SGP_REQUIRE(n_edges >= 0 && n_edges <= MAX_N && n_nodes >= 0 && n_nodes <= MAX_N, "sgp_subgraph_expand: bad size");
    if (!n_nodes) return 0;
    SGP_REQUIRE(mask_in && mask_out, "sgp_subgraph_expand: null pointer");
    SGP_REQUIRE(mask_in != mask_out, "sgp_subgraph_expand: the two masks must be different buffers");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(mask_out, mask_in, (size_t)((n_nodes + 63) / 64) * 8, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return sgp::fail((int)e, "sgp_subgraph_expand: %s", hipGetErrorString(e));
    if (!n_edges) return 0;
    SGP_REQUIRE(src && dst, "sgp_subgraph_expand: null pointer");
    hipLaunchKernelGGL(expand_kernel, dim3(grid_for(n_edges, 256 * 4)), dim3(256), 0, s, src, dst, (long long)n_edges,
                       (const u64*)mask_in, (u64*)mask_out, (long long)n_nodes);
    return sgp::check_launch("sgp_subgraph_expand");
}

int sgp_subgraph_edge_flags(const int32_t* src, const int32_t* dst, int64_t n_edges, const uint64_t* mask,
                            int64_t n_nodes, uint64_t* flags, uint8_t* edge_mask, sgp_stream_t stream) {
    SGP_REQUIRE(n_edges >= 0 && n_edges <= MAX_N && n_nodes >= 0 && n_nodes <= MAX_N, "sgp_subgraph_edge_flags: bad size");
    if (!n_edges) return 0;
    SGP_REQUIRE(src && dst && mask && flags, "sgp_subgraph_edge_flags: null pointer");
    hipLaunchKernelGGL(edge_flags_kernel, dim3(grid_for(n_edges, 256 * 4)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       (long long)n_edges, (const u64*)mask, (long long)n_nodes, (u64*)flags, edge_mask);
    return sgp::check_launch("sgp_subgraph_edge_flags");
}

int sgp_compact_pack_u8(const uint8_t* flags, int64_t n, uint64_t* bits, sgp_stream_t stream) {
    SGP_REQUIRE(n >= 0 && n <= MAX_N, "sgp_compact_pack_u8: bad size");
    if (!n) return 0;
    SGP_REQUIRE(flags && bits, "sgp_compact_pack_u8: null pointer");
    hipLaunchKernelGGL(pack_u8_kernel, dim3(grid_for(n, 256 * 4)), dim3(256), 0, (hipStream_t)stream, flags, (long long)n,
                       (u64*)bits);
    return sgp::check_launch("sgp_compact_pack_u8");
}

int sgp_compact_count(const uint64_t* bits, int64_t n, int32_t* tile_offsets, int32_t* total, sgp_stream_t stream) {
    SGP_REQUIRE(n >= 0 && n <= MAX_N, "sgp_compact_count: bad size");
    SGP_REQUIRE(total, "sgp_compact_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (!n) {
        hipError_t e = hipMemsetAsync(total, 0, 4, s);
        if (e != hipSuccess) return sgp::fail((int)e, "sgp_compact_count: %s", hipGetErrorString(e));
        return 0;
    }
    SGP_REQUIRE(bits && tile_offsets, "sgp_compact_count: null pointer");
    const long long n_tiles = sgp_compact_tiles(n);
    hipLaunchKernelGGL(count_kernel, dim3(grid_for(n_tiles, 1)), dim3(TILE_WORDS), 0, s, (const u64*)bits, (long long)n,
                       n_tiles, tile_offsets);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, tile_offsets, n_tiles, total);
    return sgp::check_launch("sgp_compact_count");
}

int sgp_compact_scatter(const uint64_t* bits, int64_t n, const int32_t* tile_offsets, int64_t n_set, int32_t* idx32,
                        int64_t* idx64, int32_t* rank, sgp_stream_t stream) {
    SGP_REQUIRE(n >= 0 && n <= MAX_N && n_set >= 0 && n_set <= n, "sgp_compact_scatter: bad size");
    if (!n || !n_set) return 0;
    SGP_REQUIRE(bits && tile_offsets && (idx32 || idx64 || rank), "sgp_compact_scatter: null pointer");
    const long long n_tiles = sgp_compact_tiles(n);
    hipLaunchKernelGGL(scatter_index_kernel, dim3(grid_for(n_tiles, 1)), dim3(TILE_WORDS), 0, (hipStream_t)stream,
                       (const u64*)bits, (long long)n, n_tiles, tile_offsets, (long long)n_set, idx32, (long long*)idx64, rank);
    return sgp::check_launch("sgp_compact_scatter");
}

int sgp_subgraph_edges(const uint64_t* flags, int64_t n_edges, const int32_t* tile_offsets, int64_t n_set,
                       const int32_t* src, const int32_t* dst, const float* weight, const int32_t* relabel,
                       int64_t n_nodes, int64_t* out_src, int64_t* out_dst, float* out_weight, sgp_stream_t stream) {
    SGP_REQUIRE(n_edges >= 0 && n_edges <= MAX_N && n_set >= 0 && n_set <= n_edges && n_nodes >= 0 && n_nodes <= MAX_N,
                "sgp_subgraph_edges: bad size");
    if (!n_edges || !n_set) return 0;
    SGP_REQUIRE(flags && tile_offsets && src && dst && relabel && out_src && out_dst, "sgp_subgraph_edges: null pointer");
    SGP_REQUIRE(!out_weight || weight, "sgp_subgraph_edges: out_weight without weight");
    const long long n_tiles = sgp_compact_tiles(n_edges);
    hipLaunchKernelGGL(scatter_edges_kernel, dim3(grid_for(n_tiles, 1)), dim3(TILE_WORDS), 0, (hipStream_t)stream,
                       (const u64*)flags, (long long)n_edges, n_tiles, tile_offsets, (long long)n_set, src, dst, weight,
                       relabel, (long long)n_nodes, (long long*)out_src, (long long*)out_dst, out_weight);
    return sgp::check_launch("sgp_subgraph_edges");
}

int sgp_subgraph_take_edges(const int32_t* src, const int32_t* dst, const float* weight, int64_t n_edges,
                            const int32_t* pos, int64_t n_pos, const int64_t* keep, int64_t n_keep,
                            const int32_t* relabel, int64_t n_nodes, int64_t* out_src, int64_t* out_dst,
                            float* out_weight, int32_t* err, sgp_stream_t stream) {
    SGP_REQUIRE(n_edges >= 0 && n_edges <= MAX_N && n_pos >= 0 && n_pos <= n_edges && n_keep >= 0 && n_keep <= MAX_N &&
                n_nodes >= 0 && n_nodes <= MAX_N, "sgp_subgraph_take_edges: bad size");
    if (!n_keep) return 0;
    SGP_REQUIRE(src && dst && out_src && out_dst, "sgp_subgraph_take_edges: null pointer");
    SGP_REQUIRE(!out_weight || weight, "sgp_subgraph_take_edges: out_weight without weight");
    hipLaunchKernelGGL(take_edges_kernel, dim3(grid_for(n_keep, 256)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       weight, (long long)n_edges, pos, (long long)n_pos, (const long long*)keep, (long long)n_keep, relabel,
                       (long long)n_nodes, (long long*)out_src, (long long*)out_dst, out_weight, err);
    return sgp::check_launch("sgp_subgraph_take_edges");
}

}  // extern "C"
