// The window gather of the data module: ONE launch builds one registered tensor of a whole batch,
//   out[b, j, k, 0:feat] = T( X[start[b] + offset + lag * j, node(b, k), 0:feat] ),
// from a resident fp32 / bf16 / fp16 series, with the scaler's transform or the mask's `!= 0` applied on the way
// (tsl/data/spatiotemporal_dataset.py window / horizon indexing, lib/dataloader/subgraph_dataloader.py:31-34).  Pure
// data movement: no LDS, no workgroup waits for another, every loop is grid-stride.
//
// Mapping.  blockIdx.y walks the (b, j) rows, so the window start, its range check and the source step row are
// workgroup-uniform (scalar loads, one division per row).  Inside a row the lanes run over `pieces`: piece e is
// (k, c) = (e / per_node, e % per_node), c fastest.  Element path (V = 1): per_node = feat, so for the raw series'
// feat of 1 or 2 neighbouring lanes are neighbouring nodes -- contiguous in `out`, contiguous in X without a node
// index and nearly so with a sorted one.  Vector path (V = 4 fp32 / 8 halves): a lane moves 16 source bytes, lanes
// along feat, then k.
#include "wg.h"

using sgp::f32x4;

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

template <int FMT> struct Elem { typedef unsigned short type; };
template <> struct Elem<0> { typedef float type; };

// exact in both formats (as in embed_store.hip): bf16 is the upper half of the fp32 pattern, every fp16 value is an
// fp32 value
template <int FMT>
__device__ __forceinline__ float widen(unsigned h) {
    if constexpr (FMT == SGP_STORE_BF16) return __uint_as_float(h << 16);
    else return (float)__builtin_bit_cast(_Float16, (unsigned short)h);
}

template <int FMT, int V>
__device__ __forceinline__ void load_piece(const typename Elem<FMT>::type* p, float (&v)[V]) {
    if constexpr (FMT == 0 && V == 1) {
        v[0] = p[0];
    } else if constexpr (FMT == 0) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else if constexpr (V == 1) {
        v[0] = widen<FMT>(p[0]);
    } else {
        const u32x4 h = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v[2 * q] = widen<FMT>(h[q] & 0xFFFFu);
            v[2 * q + 1] = widen<FMT>(h[q] >> 16);
        }
    }
}

// V floats, or V bool bytes (x != 0; NaN counts as set) at element offset o of `out`
template <int V>
__device__ __forceinline__ void store_piece(void* out, long long o, const float (&v)[V], bool as_mask) {
    if (as_mask) {
        unsigned char* ob = static_cast<unsigned char*>(out) + o;
        if constexpr (V == 1) {
            ob[0] = v[0] != 0.0f;
        } else {
            unsigned w[V / 4];
#pragma unroll
            for (int q = 0; q < V / 4; ++q)
                w[q] = (unsigned)(v[4 * q] != 0.0f) | ((unsigned)(v[4 * q + 1] != 0.0f) << 8) |
                       ((unsigned)(v[4 * q + 2] != 0.0f) << 16) | ((unsigned)(v[4 * q + 3] != 0.0f) << 24);
            if constexpr (V == 4) *reinterpret_cast<unsigned*>(ob) = w[0];
            else *reinterpret_cast<u32x2*>(ob) = u32x2{w[0], w[1]};
        }
    } else {
        float* of = static_cast<float*>(out) + o;
        if constexpr (V == 1) {
            of[0] = v[0];
        } else {
#pragma unroll
            for (int q = 0; q < V / 4; ++q)
                *reinterpret_cast<f32x4*>(of + 4 * q) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
        }
    }
}

struct WindowArgs {
    const void* X; long long xss, xns, n_steps, n_nodes; int feat;
    const int* start; long long rows; int count; long long offset, lag;
    const int* node; long long n_out, nbs;
    int mode; const float* bias; const float* scale; long long pns; int pfs;
    void* out; int* err;
};

template <int FMT, int V>
__global__ __launch_bounds__(256) void window_gather_kernel(const WindowArgs a) {
    typedef typename Elem<FMT>::type E;
    const int per_node = a.feat / V;
    const long long pieces = a.n_out * per_node;
    for (long long r = blockIdx.y; r < a.rows; r += gridDim.y) {
        long long b; int j;                                     // workgroup-uniform
        if (a.rows <= 0x7FFFFFFFll) {
            const unsigned q = (unsigned)r / (unsigned)a.count;
            b = q;
            j = (int)((unsigned)r - q * (unsigned)a.count);
        } else {
            b = r / a.count;
            j = (int)(r - b * a.count);
        }
        // the whole sample is judged, not this row alone: a start is bad for every j or for none
        const long long first = (long long)a.start[b] + a.offset, last = first + a.lag * (a.count - 1);
        const bool row_ok = first >= 0 && last < a.n_steps;
        if (!row_ok && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.err, SGP_WINDOW_ERR_START);
        const E* xrow = static_cast<const E*>(a.X) + (row_ok ? (first + a.lag * j) * a.xss : 0ll);
        const int* nrow = a.node ? a.node + b * a.nbs : nullptr;
        for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < pieces;
             e += (long long)gridDim.x * blockDim.x) {
            long long k = e; int c = 0;
            if (per_node > 1) {
                if (pieces <= 0x7FFFFFFFll) {
                    const unsigned q = (unsigned)e / (unsigned)per_node;
                    k = q;
                    c = (int)((unsigned)e - q * (unsigned)per_node);
                } else {
                    k = e / per_node;
                    c = (int)(e - k * per_node);
                }
            }
            long long g = k;                                    // without an index k < n_out = n_nodes
            bool ok = row_ok;
            if (nrow) {
                const int id = nrow[k];
                g = id;
                if (!sgp::in_range(id, a.n_nodes)) {
                    atomicOr(a.err, SGP_WINDOW_ERR_NODE);
                    ok = false;
                }
            }
            float v[V];
#pragma unroll
            for (int q = 0; q < V; ++q) v[q] = 0.0f;
            if (ok) {
                load_piece<FMT, V>(xrow + g * a.xns + (long long)c * V, v);
                if (a.mode == SGP_WINDOW_SCALE) {
                    // Scaler.transform's expression as scalers.hip evaluates it: IEEE subtraction, IEEE division, the
                    // epsilon added last; there is no product here for the backend to contract
                    const long long p = g * a.pns + (long long)c * V * a.pfs;
#pragma unroll
                    for (int q = 0; q < V; ++q) v[q] = (v[q] - a.bias[p + q * a.pfs]) / a.scale[p + q * a.pfs] + 5e-8f;
                }
            }
            store_piece<V>(a.out, (r * a.n_out + k) * a.feat + (long long)c * V, v, a.mode == SGP_WINDOW_MASK);
        }
    }
}

template <int FMT>
void launch(bool vec, dim3 grid, dim3 block, hipStream_t s, const WindowArgs& a) {
    constexpr int V = FMT == 0 ? 4 : 8;
    if (vec) hipLaunchKernelGGL((window_gather_kernel<FMT, V>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((window_gather_kernel<FMT, 1>), grid, block, 0, s, a);
}

}  // namespace

extern "C" {

int sgp_window_gather(const void* X, int32_t src_fmt, int64_t x_step_stride, int64_t x_node_stride,
                      int32_t n_steps, int32_t n_nodes, int32_t feat,
                      const int32_t* start, int32_t batch, int32_t offset, int32_t count, int32_t lag,
                      const int32_t* node, int32_t n_out, int64_t node_batch_stride,
                      int32_t mode, const float* bias, const float* scale, int32_t param_nodes, int32_t param_feat,
                      void* out, int32_t* err, sgp_stream_t stream) {
    SGP_REQUIRE(src_fmt == 0 || src_fmt == SGP_STORE_BF16 || src_fmt == SGP_STORE_F16,
                "sgp_window_gather: src_fmt must be 0 (fp32), SGP_STORE_BF16 or SGP_STORE_F16");
    SGP_REQUIRE(mode == SGP_WINDOW_IDENTITY || mode == SGP_WINDOW_SCALE || mode == SGP_WINDOW_MASK,
                "sgp_window_gather: mode must be SGP_WINDOW_IDENTITY, _SCALE or _MASK");
    SGP_REQUIRE(n_steps >= 0 && n_nodes >= 0 && feat >= 0 && batch >= 0 && count >= 0 && n_out >= 0 && offset >= 0 &&
                lag >= 1 && x_step_stride >= 0 && x_node_stride >= 0,
                "sgp_window_gather: bad size (sizes, offset and strides must not be negative, lag at least 1)");
    if (!batch || !count || !n_out || !feat) return 0;          // (an empty tensor has no address)
    SGP_REQUIRE(X && start && out && err, "sgp_window_gather: null pointer");
    SGP_REQUIRE(node || n_out == n_nodes, "sgp_window_gather: without a node index n_out must be n_nodes");
    SGP_REQUIRE(!node || node_batch_stride == 0 || node_batch_stride == n_out,
                "sgp_window_gather: node_batch_stride must be 0 (shared index) or n_out (one per item)");
    const uintptr_t elem = src_fmt == 0 ? 4 : 2;
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(X) & (elem - 1)) == 0, "sgp_window_gather: X is not aligned to its elements");
    SGP_REQUIRE(mode == SGP_WINDOW_MASK || (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
                "sgp_window_gather: out must be 4-byte aligned");
    SGP_REQUIRE((reinterpret_cast<uintptr_t>(err) & 3u) == 0, "sgp_window_gather: err must be 4-byte aligned");
    if (mode == SGP_WINDOW_SCALE) {
        SGP_REQUIRE(bias && scale, "sgp_window_gather: SGP_WINDOW_SCALE needs bias and scale");
        SGP_REQUIRE((param_nodes == 1 || param_nodes == n_nodes) && (param_feat == 1 || param_feat == feat),
                    "sgp_window_gather: parameters must be [1 | n_nodes, 1 | feat] (got [%d, %d])", param_nodes, param_feat);
    }
    WindowArgs a;
    a.X = X; a.xss = x_step_stride; a.xns = x_node_stride; a.n_steps = n_steps; a.n_nodes = n_nodes; a.feat = feat;
    a.start = start; a.rows = (long long)batch * count; a.count = count; a.offset = offset; a.lag = lag;
    a.node = node; a.n_out = n_out; a.nbs = node ? node_batch_stride : 0;
    a.mode = mode; a.bias = bias; a.scale = scale;
    a.pns = param_nodes == 1 ? 0 : param_feat;                  // parameters are indexed by the GLOBAL node id
    a.pfs = param_feat == 1 ? 0 : 1;
    a.out = out; a.err = err;
    const int v = src_fmt == 0 ? 4 : 8;
    const bool vec = feat % v == 0 && x_step_stride % v == 0 && x_node_stride % v == 0 && sgp::aligned16(X) &&
                     sgp::aligned16(out);
    const long long pieces = (long long)n_out * (vec ? feat / v : feat);
    const unsigned threads = pieces <= 64 ? 64 : 256;
    const unsigned gx = sgp::grid_for(pieces, threads, 4096);
    const long long gy_cap = 16384 / gx < 1 ? 1 : 16384 / gx;
    const dim3 grid(gx, (unsigned)(a.rows < gy_cap ? a.rows : gy_cap)), block(threads);
    hipStream_t s = (hipStream_t)stream;
    if (src_fmt == 0) launch<0>(vec, grid, block, s, a);
    else if (src_fmt == SGP_STORE_BF16) launch<SGP_STORE_BF16>(vec, grid, block, s, a);
    else launch<SGP_STORE_F16>(vec, grid, block, s, a);
    return sgp::check_launch("window_gather");
}

}  // extern "C"
