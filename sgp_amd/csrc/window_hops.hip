// The hop block of SGPOnlineModel (reference call site lib/nn/models/sgp_online.py:55-61:
// rearrange 'b t n f -> b n (t f)', sgp_spatial_embedding, torch.cat).  ONE launch is one hop of one direction for
// the whole batch, from the raw window [b, t, n, f] where it lies or from an earlier block of the output, into a
// block of the one output buffer out[b, n, D], D = n_blocks * W, W = t * f.  The first forward hop also writes block 0
// (the flattened window) for its own rows, so the model needs K * dirs launches, no copy kernel and no cat.
//
// Summation order.  The result has to be the bits of today's composition, which runs the generic CSR kernels of
// spmm.hip on W-wide slots of a 16-byte aligned buffer; every form below therefore keeps that kernel's order for its W:
//   W % 4 != 0   spmm_csr_scalar: one fp32 chain over the row's entries in CSR order.
//   W % 4 == 0   spmm_csr_rows<LPR>, LPR = sgp_spmm_csr_form(W): G = 64 / LPR partial chains, chain g over the entries
//                e0 + g, e0 + g + G, ... in order, then a butterfly over g (bit 0 first).  fp32 addition commutes, so
//                the butterfly's value does not depend on which lane holds which partial.
// The product and the add of a chain step are one fused multiply-add here and there (-ffp-contract=fast on both files).
//
// Forms (sgp_window_hop_form):
//   DIRECT   the lane layout of the CSR kernels themselves (rows<LPR> with 16-byte loads from a block; a wave packs
//            several (batch item, feature) pairs of its row when W % 4 != 0).  A window source is gathered element by
//            element: element (t, c) of a neighbour sits on its own cache line, t * f lines per neighbour.
//   PLANES   window source with t > 1 whose [n, f] plane fits the LDS stage: a workgroup stages the planes (b, t) of up
//            to 4 batch items with coalesced loads, G lanes own a row and gather from LDS.  A row's (col, val) are
//            loaded once per staged feature and shared by the batch items.
#include "common.h"
#include "device_math.h"

using sgp::f32x4;
using sgp::ld4;
using sgp::st4;

namespace {

constexpr int kStageFloats = 16384;   // 64 KiB of LDS: the default dynamic limit, two workgroups per CU
constexpr int kPlaneBatch = 4;
constexpr int kPlaneThreads = 1024;

struct Hop {
    const int* rowptr; const int* col; const float* val;      // rowptr == nullptr: block 0 only (K = 0)
    const float* x; long long bs, ts, ns; int f;              // window element (b, t, c, k): x[b bs + t ts + c ns + k]
    float* out; long long D;                                  // out[b, i, D]
    int W, sblock, dblock, write0;
    int n, batch;
};

// ---------------------------------------------------------------- DIRECT, W % 4 == 0
template <int LPR, bool WIN>
__global__ __launch_bounds__(256) void window_hop_rows(Hop h) {
    constexpr int G = 64 / LPR, TB = 4;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= h.n) return;
    const int lane = threadIdx.x & 63;
    const int f0 = blockIdx.z * (4 * LPR) + (lane % LPR) * 4;
    const int g = lane / LPR;
    const bool fok = f0 < h.W;
    const int b0 = blockIdx.y * TB;
    const long long obs = (long long)h.n * h.D;

    long long woff[4] = {0, 0, 0, 0};
    if constexpr (WIN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = fok ? f0 + j : 0;
            woff[j] = (long long)(w / h.f) * h.ts + (w % h.f);
        }
    }
    auto window4 = [&](int b, int c) {
        const float* p = h.x + (long long)b * h.bs + (long long)c * h.ns;
        return f32x4{p[woff[0]], p[woff[1]], p[woff[2]], p[woff[3]]};
    };

    if (h.rowptr != nullptr) {
        f32x4 acc[TB];
#pragma unroll
        for (int i = 0; i < TB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* sblk = h.out + (long long)h.sblock * h.W + f0;
        const int e1 = h.rowptr[row + 1];
        for (int e = h.rowptr[row] + g; e < e1; e += G) {
            const int c = h.col[e];
            const float v = h.val[e];
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                if (fok && b0 + i < h.batch) {
                    f32x4 xv;
                    if constexpr (WIN) xv = window4(b0 + i, c);
                    else xv = ld4(sblk + (long long)(b0 + i) * obs + (long long)c * h.D);
                    acc[i] += v * xv;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TB; ++i) {
#pragma unroll
            for (int off = LPR; off < 64; off <<= 1) {
                acc[i].x += __shfl_xor(acc[i].x, off);
                acc[i].y += __shfl_xor(acc[i].y, off);
                acc[i].z += __shfl_xor(acc[i].z, off);
                acc[i].w += __shfl_xor(acc[i].w, off);
            }
        }
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            if (fok && b0 + i < h.batch && g == (i % G))
                st4(h.out + (long long)(b0 + i) * obs + (long long)row * h.D + (long long)h.dblock * h.W + f0, acc[i]);
        }
    }
    if constexpr (WIN) {
        if (h.write0) {
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                if (fok && b0 + i < h.batch && g == (i % G))
                    st4(h.out + (long long)(b0 + i) * obs + (long long)row * h.D + f0, window4(b0 + i, row));
            }
        }
    }
}

// ---------------------------------------------------------------- DIRECT, any W: one chain per element
// A wave owns a row and `bc` batch items; its lanes run over the (batch item, feature) pairs, so W = 10 fills a wave
// with six batch items of the row instead of ten lanes.
template <bool WIN>
__global__ __launch_bounds__(256) void window_hop_scalar(Hop h, int bc) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= h.n) return;
    const int lane = threadIdx.x & 63;
    const int b0 = blockIdx.y * bc;
    const int nb = min(bc, h.batch - b0);
    const long long obs = (long long)h.n * h.D;
    int e0 = 0, e1 = 0;
    if (h.rowptr != nullptr) { e0 = h.rowptr[row]; e1 = h.rowptr[row + 1]; }
    for (int idx = lane; idx < nb * h.W; idx += 64) {
        const int bi = idx / h.W, w = idx - bi * h.W, b = b0 + bi;
        const float* sp;
        long long stride;
        if constexpr (WIN) {
            sp = h.x + (long long)b * h.bs + (long long)(w / h.f) * h.ts + (w % h.f);
            stride = h.ns;
        } else {
            sp = h.out + (long long)b * obs + (long long)h.sblock * h.W + w;
            stride = h.D;
        }
        float* orow = h.out + (long long)b * obs + (long long)row * h.D;
        if (h.rowptr != nullptr) {
            float acc = 0.f;
            for (int e = e0; e < e1; ++e) acc += h.val[e] * sp[(long long)h.col[e] * stride];
            orow[(long long)h.dblock * h.W + w] = acc;
        }
        if constexpr (WIN) {
            if (h.write0) orow[w] = sp[(long long)row * stride];
        }
    }
}

// ---------------------------------------------------------------- PLANES: window source staged in LDS
// Workgroup (t, batch chunk, row chunk).  G lanes own a row: lane g runs chain g, the butterfly folds them.
template <int G>
__global__ __launch_bounds__(kPlaneThreads) void window_hop_planes(Hop h, int pb, int rows_per_wg) {
    extern __shared__ __attribute__((aligned(16))) float stage[];
    const int tid = threadIdx.x;
    const int t = blockIdx.x;
    const int b0 = blockIdx.y * pb;
    const int nb = min(pb, h.batch - b0);
    const int nf = h.n * h.f;

    for (int p = 0; p < nb; ++p) {
        const float* plane = h.x + (long long)(b0 + p) * h.bs + (long long)t * h.ts;
        for (int i = tid; i < nf; i += kPlaneThreads) {
            const int node = i / h.f, k = i - node * h.f;
            stage[p * nf + i] = plane[(long long)node * h.ns + k];
        }
    }
    __syncthreads();

    constexpr int kSlots = kPlaneThreads / G;
    const int g = tid % G, slot = tid / G;
    const int r_begin = blockIdx.z * rows_per_wg;
    const int r_end = min(h.n, r_begin + rows_per_wg);
    const long long obs = (long long)h.n * h.D;
    for (int r0 = r_begin; r0 < r_end; r0 += kSlots) {     // workgroup-uniform trip count: the butterfly needs every lane
        const int r = r0 + slot;
        const bool valid = r < r_end;
        int e0 = 0, e1 = 0;
        if (valid) { e0 = h.rowptr[r] + g; e1 = h.rowptr[r + 1]; }
        for (int k = 0; k < h.f; ++k) {
            float acc[kPlaneBatch];
#pragma unroll
            for (int p = 0; p < kPlaneBatch; ++p) acc[p] = 0.f;
            for (int e = e0; e < e1; e += G) {
                const int c = h.col[e] * h.f + k;
                const float v = h.val[e];
#pragma unroll
                for (int p = 0; p < kPlaneBatch; ++p)
                    if (p < nb) acc[p] += v * stage[p * nf + c];
            }
#pragma unroll
            for (int p = 0; p < kPlaneBatch; ++p) {
#pragma unroll
                for (int off = 1; off < G; off <<= 1) acc[p] += __shfl_xor(acc[p], off);
            }
#pragma unroll
            for (int p = 0; p < kPlaneBatch; ++p) {
                if (valid && p < nb && g == (p % G)) {
                    float* orow = h.out + (long long)(b0 + p) * obs + (long long)r * h.D + t * h.f + k;
                    orow[(long long)h.dblock * h.W] = acc[p];
                    if (h.write0) orow[0] = stage[p * nf + r * h.f + k];
                }
            }
        }
    }
}

int chain_lanes(int W) { return W % 4 == 0 ? sgp_spmm_csr_form(W, 1, 0) : 0; }

// The launch geometry of one hop: the one computation behind sgp_window_hop_f32 and sgp_window_hop_plan.
enum { kRows = 0, kScalar = 1, kPlanes = 2 };
struct HopPlan {
    int form, kernel, lanes;              // lanes: LPR (rows), G (planes), 0 (scalar)
    unsigned gx, gy, gz;                  // all 0: an empty shape, nothing to launch
    int chunk;                            // batch items per workgroup: 4 (rows), bc (scalar), pb (planes)
    int rows_per_wg, row_trips;           // planes; otherwise 0 and 1
    size_t lds;
};

int plan_hop(const char* what, bool win, bool hop, int batch, int steps, int n, int feat, int form, HopPlan& p) {
    SGP_REQUIRE(batch >= 0 && steps >= 0 && n >= 0 && feat >= 0, "%s: bad size", what);
    SGP_REQUIRE((long long)steps * feat < (1ll << 24), "%s: window too wide", what);
    SGP_REQUIRE(form == 0 || form == SGP_WINDOW_HOP_DIRECT || form == SGP_WINDOW_HOP_PLANES, "%s: unknown form", what);
    const int natural = sgp_window_hop_form(win, hop, steps, n, feat);
    const int W = steps * feat;
    p = HopPlan{form ? form : natural, kScalar, 0, 0, 0, 0, 0, 0, 1, 0};
    if (batch == 0 || n == 0 || W == 0) return 0;
    if (form == SGP_WINDOW_HOP_PLANES && natural != SGP_WINDOW_HOP_PLANES)
        return sgp::fail(SGP_EUNSUP, "%s: the staged form needs a window source of more than one step "
                                     "whose [n, f] plane holds at most %d floats", what, kStageFloats);
    const int lpr = chain_lanes(W);
    p.gx = (n + 3) / 4;

    if (p.form == SGP_WINDOW_HOP_PLANES) {
        const int G = lpr ? 64 / lpr : 1;
        const int nf = n * feat;
        int pb = kStageFloats / nf;
        pb = pb > kPlaneBatch ? kPlaneBatch : pb;
        pb = pb > batch ? batch : pb;
        const int gy = (batch + pb - 1) / pb;
        SGP_REQUIRE(gy <= 65535, "%s: batch too large for one launch (chunk it)", what);
        // a few workgroups per CU: every row chunk stages its planes again (coalesced, from L2)
        const int slots = kPlaneThreads / G;
        const long long wgs = (long long)steps * gy;
        long long rc = (1024 + wgs - 1) / wgs;
        const long long rc_max = (n + slots - 1) / slots;
        rc = rc < 1 ? 1 : (rc > rc_max ? rc_max : rc);
        int rows_per_wg = (int)((n + rc - 1) / rc);
        rows_per_wg = (rows_per_wg + slots - 1) / slots * slots;
        const int gz = (n + rows_per_wg - 1) / rows_per_wg;
        SGP_REQUIRE(gz <= 65535, "%s: too many row chunks", what);
        p.kernel = kPlanes;
        p.lanes = G;
        p.gx = steps; p.gy = gy; p.gz = gz;
        p.chunk = pb;
        p.rows_per_wg = rows_per_wg;
        p.row_trips = rows_per_wg / slots;
        p.lds = (size_t)pb * nf * sizeof(float);
        return 0;
    }
    if (lpr == 0) {
        int bc = 256 / W;
        bc = bc < 1 ? 1 : (bc > batch ? batch : bc);
        const int gy = (batch + bc - 1) / bc;
        SGP_REQUIRE(gy <= 65535, "%s: batch too large for one launch (chunk it)", what);
        p.gy = gy; p.gz = 1;
        p.chunk = bc;
        return 0;
    }
    const unsigned gy = (batch + 3) / 4;
    SGP_REQUIRE(gy <= 65535, "%s: batch too large for one launch (chunk it)", what);
    const int gz = (W + 4 * lpr - 1) / (4 * lpr);
    SGP_REQUIRE(gz <= 65535, "%s: window too wide for one launch", what);      // (the runtime refused this launch before)
    p.kernel = kRows;
    p.lanes = lpr;
    p.gy = gy; p.gz = gz;
    p.chunk = 4;
    return 0;
}

}  // namespace

extern "C" {

int32_t sgp_window_hop_form(int32_t from_window, int32_t has_operator, int32_t steps, int32_t n, int32_t feat) {
    if (!from_window || !has_operator || steps <= 1) return SGP_WINDOW_HOP_DIRECT;
    return (long long)n * feat <= kStageFloats ? SGP_WINDOW_HOP_PLANES : SGP_WINDOW_HOP_DIRECT;
}

int sgp_window_hop_plan(int32_t from_window, int32_t has_operator, int32_t batch, int32_t steps, int32_t n,
                        int32_t feat, int32_t form, int64_t* out) {
    const char* what = "sgp_window_hop_plan";
    SGP_REQUIRE(out, "%s: null pointer", what);
    SGP_REQUIRE(has_operator || from_window, "%s: nothing to do without an operator", what);
    HopPlan p;
    if (int rc = plan_hop(what, from_window != 0, has_operator != 0, batch, steps, n, feat, form, p)) return rc;
    out[0] = p.form; out[1] = p.kernel; out[2] = p.lanes;
    out[3] = p.gx; out[4] = p.gy; out[5] = p.gz;
    out[6] = p.chunk; out[7] = p.rows_per_wg; out[8] = p.row_trips;
    out[9] = (int64_t)p.lds;
    return 0;
}

int sgp_window_hop_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                       const float* x, int64_t x_bs, int64_t x_ts, int64_t x_ns,
                       float* out, int32_t src_block, int32_t dst_block, int32_t write_block0,
                       int32_t batch, int32_t steps, int32_t n, int32_t feat, int32_t n_blocks,
                       int32_t form, sgp_stream_t stream) {
    const char* what = "sgp_window_hop_f32";
    SGP_REQUIRE(batch >= 0 && steps >= 0 && n >= 0 && feat >= 0 && n_blocks >= 1, "sgp_window_hop_f32: bad size");
    SGP_REQUIRE((long long)steps * feat < (1ll << 24) && (long long)steps * feat * n_blocks < (1ll << 31),
                "sgp_window_hop_f32: window too wide");
    const bool win = src_block < 0;
    const bool hop = rowptr != nullptr;
    SGP_REQUIRE(out != nullptr && (!win || x != nullptr), "sgp_window_hop_f32: null pointer");
    SGP_REQUIRE(!hop || (col != nullptr && val != nullptr), "sgp_window_hop_f32: null pointer");
    SGP_REQUIRE(hop || (win && write_block0), "sgp_window_hop_f32: nothing to do without an operator");
    SGP_REQUIRE(win || !write_block0, "sgp_window_hop_f32: block 0 is written from the window only");
    SGP_REQUIRE(form == 0 || form == SGP_WINDOW_HOP_DIRECT || form == SGP_WINDOW_HOP_PLANES,
                "sgp_window_hop_f32: unknown form");
    if (hop) {
        SGP_REQUIRE(dst_block >= 1 && dst_block < n_blocks && src_block < n_blocks && src_block != dst_block,
                    "sgp_window_hop_f32: block out of range");
        SGP_REQUIRE(!(write_block0 && dst_block == 0), "sgp_window_hop_f32: block out of range");
    }
    const int W = steps * feat;
    if (batch == 0 || n == 0 || W == 0) return 0;
    if (chain_lanes(W) != 0)
        SGP_REQUIRE(((uintptr_t)out & 15) == 0, "sgp_window_hop_f32: out must be 16-byte aligned");
    HopPlan p;
    if (int rc = plan_hop(what, win, hop, batch, steps, n, feat, form, p)) return rc;
    Hop h{rowptr, col, val, x, x_bs, x_ts, x_ns, feat, out, (long long)W * n_blocks,
          W, src_block, dst_block, write_block0 ? 1 : 0, n, batch};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(p.gx, p.gy, p.gz);

    if (p.kernel == kPlanes) {
#define SGP_PLANES(GG) \
    hipLaunchKernelGGL((window_hop_planes<GG>), grid, dim3(kPlaneThreads), p.lds, s, h, p.chunk, p.rows_per_wg)
        switch (p.lanes) {
            case 16: SGP_PLANES(16); break;
            case 8: SGP_PLANES(8); break;
            case 4: SGP_PLANES(4); break;
            case 2: SGP_PLANES(2); break;
            default: SGP_PLANES(1); break;
        }
#undef SGP_PLANES
        return sgp::check_launch("window_hop_planes");
    }
    if (p.kernel == kScalar) {
        if (win) hipLaunchKernelGGL((window_hop_scalar<true>), grid, dim3(256), 0, s, h, p.chunk);
        else hipLaunchKernelGGL((window_hop_scalar<false>), grid, dim3(256), 0, s, h, p.chunk);
        return sgp::check_launch("window_hop_scalar");
    }
#define SGP_ROWS(LPR)                                                                                         \
    do {                                                                                                      \
        if (win) hipLaunchKernelGGL((window_hop_rows<LPR, true>), grid, dim3(256), 0, s, h);                  \
        else hipLaunchKernelGGL((window_hop_rows<LPR, false>), grid, dim3(256), 0, s, h);                     \
    } while (0)
    switch (p.lanes) {
        case 64: SGP_ROWS(64); break;
        case 32: SGP_ROWS(32); break;
        case 16: SGP_ROWS(16); break;
        case 8: SGP_ROWS(8); break;
        default: SGP_ROWS(4); break;
    }
#undef SGP_ROWS
    return sgp::check_launch("window_hop_rows");
}

}  // extern "C"
