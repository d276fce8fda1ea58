// GRIN: the two stages that surround the diffusion-GRU cells in one step of GRIL (reference:
// tsl/nn/layers/graph_convs/grin_cell.py:200-227 and SpatialDecoder.forward :82-104).  With hT the top layer's state
// entering the step, m the mask and R = b n rows,
//
//   stage 1   p1 = W_fs hT + b_fs,  x1 = m ? x : p1,  z = W_in [x1 | m | hT | u] + b_in            -> slot 0 of dec [R, 3 H]
//   (one sgp_diffuse_f32 launch fills slots 1 and 2 with A_f z and A_b z, self loops removed)
//   stage 2   g = W_f [A_f z | A_b z] + b_f,  o = PReLU(W_o [g | hT] + b_o),  repr = [o | hT],
//             p2 = W_ro repr + b_ro,  x2 = m ? x : p2,  [x2 | m | u]                                -> slot 0 of the cell input
//
// and their backward halves, time reversed.  The step's input depends on the state of the same step, so nothing of
// this leaves the time loop; one launch per stage replaces about twenty small products, selects and concatenations.
//
// Mapping: a workgroup of 4 waves owns ONE tile of 16 rows.  Every product is a v_mfma_f32_16x16x4_f32 with the packed
// weight as the A operand (rows = output features) and the rows' vector, read from LDS, as the B operand; the waves
// deal the output tiles of 16 features round robin, the products of a chain hand their result to the next through LDS
// with one barrier in between.  Vectors are zero padded in LDS to whole k-blocks of 16, the packed weights (fragment
// order, frag.h) likewise.
// Arithmetic: exact fp32 products, one k-ordered chain per output starting from the bias, no atomics: every kernel is
// bit-identical from run to run and independent of the tile a row falls into.  x is only ever selected by the mask,
// never multiplied: a value at a missing entry is not read into any result.
// Rows: x, mask, u, p1, p2, repr, dP1, dP2, dRepr, gx and gu lie in the window's own [b, S, n, .] order, row
// (r / n) S n + tt n + r % n for row r of step tt; `reverse` makes tt = S - 1 - t.  Everything else is [R, .] of the step.
// LDS (floats; the budget per kernel is in DESIGN.md 9u): at most 2 * 16 (2 H + 4) + 16 * 20, 34 KB at H = 128.
#include "common.h"
#include "frag.h"
#include "wg.h"

namespace {
using sgp::f32x4;
using sgp::ld4;
using sgp::st4;
using sgp::kPad;
using sgp::tile_prod;
using sgp::bias4;

constexpr int kThreads = 256, kWaves = 4;

struct Dims {
    int H, C, U, K1, JT, KT;                                // K1 = 2 C + H + U; JT = H / 16; KT = tiles of 16 along K1
    Dims(int h, int c, int u) : H(h), C(c), U(u), K1(2 * c + h + u), JT(h / 16), KT((2 * c + h + u + 15) / 16) {}
    // floats of the packed parts: W_fs, W_in, W_f, W_o, W_ro, then their transposes in the same order
    long long fs() const { return 256ll * JT; }
    long long in() const { return 256ll * JT * KT; }
    long long sq() const { return 256ll * JT * 2 * JT; }    // W_f and W_o [H, 2 H]
    long long ro() const { return 256ll * 2 * JT; }
    long long dir() const { return fs() + in() + 2 * sq() + ro(); }
};

struct Packed { const float *fs, *in, *f, *o, *ro; };
Packed parts(const float* p, const Dims& d, bool bwd) {
    if (bwd) p += d.dir();
    return Packed{p, p + d.fs(), p + d.fs() + d.in(), p + d.fs() + d.in() + d.sq(), p + d.fs() + d.in() + 2 * d.sq()};
}

struct Args {
    Packed w;
    const float *b0, *b1, *b2, *slope;                      // biases in the order their products run
    const float *hT, *x, *msk, *u;
    const float *dP, *dRepr, *dcell;
    float *p, *dec, *repr, *cell, *save_a, *save_b;         // forward outputs; backward: pre, dg
    float *carry, *gx, *gu, *dp, *partial;
    long long R, inner, ldh, ldd, ldr, ldc;
    int S, tt, H, C, U;
};

__device__ __forceinline__ long long win_row(long long r, long long inner, int S, int tt) {
    return (r / inner) * S * inner + (long long)tt * inner + r % inner;
}

// ------------------------------------------------------------------------------------------------------- stage 1
__global__ __launch_bounds__(kThreads) void grin_stage1(Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, C = a.C, U = a.U, K1 = 2 * C + H + U, JT = H / 16, KT = (K1 + 15) / 16;
    const int LDH = H + kPad, LDI = 16 * KT + kPad;
    float* hb = lds;                                        // [16][LDH]   hT
    float* ib = lds + 16 * LDH;                             // [16][LDI]   [x1 | m | hT | u], zero padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, q = lane >> 4;
    const long long r0 = (long long)blockIdx.x * 16;
    for (int i = threadIdx.x; i < 16 * LDI; i += kThreads) ib[i] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < 16 * H; i += kThreads) {
        const int r = i / H, c = i % H;
        const long long row = r0 + r < a.R ? r0 + r : a.R - 1;
        const float v = a.hT[row * a.ldh + c];
        hb[r * LDH + c] = v;
        ib[r * LDI + 2 * C + c] = v;
    }
    for (int i = threadIdx.x; i < 16 * (C + U); i += kThreads) {
        const int r = i / (C + U), c = i % (C + U);
        const long long row = r0 + r < a.R ? r0 + r : a.R - 1;
        const long long xr = win_row(row, a.inner, a.S, a.tt);
        if (c < C) ib[r * LDI + C + c] = a.msk[xr * C + c] != 0.f ? 1.f : 0.f;
        else ib[r * LDI + 2 * C + H + (c - C)] = a.u[xr * U + (c - C)];
    }
    __syncthreads();
    const long long m = r0 + n;
    const bool ok = m < a.R;
    const long long mc = ok ? m : a.R - 1;
    const long long xr = win_row(mc, a.inner, a.S, a.tt);
    if (wave == 0) {                                        // C <= 16: one tile
        const f32x4 acc = tile_prod(a.w.fs, 0, JT, hb + n * LDH + 4 * q, bias4(a.b0, 4 * q, C), lane);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int d = 4 * q + s;
            if (d < C) {
                const bool seen = ib[n * LDI + C + d] != 0.f;
                float xv = acc[s];
                if (seen) xv = a.x[xr * C + d];
                ib[n * LDI + d] = xv;
                if (ok) a.p[xr * C + d] = acc[s];
            }
        }
    }
    __syncthreads();
    for (int jt = wave; jt < JT; jt += kWaves) {
        const f32x4 z = tile_prod(a.w.in, jt, KT, ib + n * LDI + 4 * q, ld4(a.b1 + 16 * jt + 4 * q), lane);
        if (ok) st4(a.dec + m * a.ldd + 16 * jt + 4 * q, z);
    }
    if (a.save_a)
        for (int i = threadIdx.x; i < 16 * K1; i += kThreads) {
            const int r = i / K1, c = i % K1;
            if (r0 + r < a.R) a.save_a[(r0 + r) * K1 + c] = ib[r * LDI + c];
        }
}

// ------------------------------------------------------------------------------------------------------- stage 2
__global__ __launch_bounds__(kThreads) void grin_stage2(Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, C = a.C, U = a.U, JT = H / 16, LD = 2 * H + kPad;
    float* A = lds;                                         // [16][LD]   [A_f z | A_b z], later repr = [o | hT]
    float* B = lds + 16 * LD;                               // [16][LD]   [g | hT]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, q = lane >> 4;
    const long long r0 = (long long)blockIdx.x * 16;
    for (int i = threadIdx.x; i < 16 * 2 * H; i += kThreads) {
        const int r = i / (2 * H), c = i % (2 * H);
        const long long row = r0 + r < a.R ? r0 + r : a.R - 1;
        A[r * LD + c] = a.dec[row * a.ldd + H + c];
        if (c < H) B[r * LD + H + c] = a.hT[row * a.ldh + c];
    }
    __syncthreads();
    const long long m = r0 + n;
    const bool ok = m < a.R;
    const long long mc = ok ? m : a.R - 1;
    const long long xr = win_row(mc, a.inner, a.S, a.tt);
    for (int jt = wave; jt < JT; jt += kWaves) {
        const int col = 16 * jt + 4 * q;
        st4(B + n * LD + col, tile_prod(a.w.f, jt, 2 * JT, A + n * LD + 4 * q, ld4(a.b0 + col), lane));
    }
    __syncthreads();                                        // g complete, A fully consumed
    const float slope = a.slope[0];
    for (int jt = wave; jt < JT; jt += kWaves) {
        const int col = 16 * jt + 4 * q;
        const f32x4 pre = tile_prod(a.w.o, jt, 2 * JT, B + n * LD + 4 * q, ld4(a.b1 + col), lane);
        f32x4 o;
#pragma unroll
        for (int s = 0; s < 4; ++s) o[s] = pre[s] > 0.f ? pre[s] : slope * pre[s];
        const f32x4 g = ld4(B + n * LD + col), hv = ld4(B + n * LD + H + col);
        st4(A + n * LD + col, o);
        st4(A + n * LD + H + col, hv);
        if (a.save_a && ok) {
            st4(a.save_a + m * H + col, pre);
            st4(a.save_b + m * 2 * H + col, g);
            st4(a.save_b + m * 2 * H + H + col, hv);
        }
    }
    __syncthreads();                                        // repr complete
    for (int i = threadIdx.x; a.repr && i < 16 * 2 * H; i += kThreads) {
        const int r = i / (2 * H), c = i % (2 * H);
        if (r0 + r < a.R) a.repr[win_row(r0 + r, a.inner, a.S, a.tt) * a.ldr + c] = A[r * LD + c];
    }
    if (wave == 0) {
        const f32x4 acc = tile_prod(a.w.ro, 0, 2 * JT, A + n * LD + 4 * q, bias4(a.b2, 4 * q, C), lane);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int d = 4 * q + s;
            if (d < C && ok) {
                const bool seen = a.msk[xr * C + d] != 0.f;
                float xv = acc[s];
                if (seen) xv = a.x[xr * C + d];
                a.p[xr * C + d] = acc[s];
                a.cell[m * a.ldc + d] = xv;
                a.cell[m * a.ldc + C + d] = seen ? 1.f : 0.f;
            }
        }
    } else if (wave == 1) {
        for (int i = lane; i < 16 * U; i += 64) {
            const int r = i / U, c = i % U;
            if (r0 + r < a.R) a.cell[(r0 + r) * a.ldc + 2 * C + c] = a.u[win_row(r0 + r, a.inner, a.S, a.tt) * U + c];
        }
    }
}

// ---------------------------------------------------------------------------------------------- stage 2, backward
// dp2 = dP2 + (1 - m) dx2, gx = m dx2;  drepr = W_ro^T dp2 + dRepr;  dpre = do PReLU'(pre) (in place of pre);
// d[g | hT] = W_o^T dpre;  d slots 1, 2 of dec = W_f^T dg, slot 0 zeroed for the adjoint hop;  carry += dhT.
__global__ __launch_bounds__(kThreads) void grin_stage2_bwd(Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double red[kWaves];
    const int H = a.H, C = a.C, JT = H / 16, LD = 2 * H + kPad, LDP = 16 + kPad;
    float* D1 = lds;                                        // [16][LD]   [dpre | dhT from read_out]
    float* D2 = lds + 16 * LD;                              // [16][LD]   dg in the first H columns
    float* P = lds + 2 * 16 * LD;                           // [16][LDP]  dp2, zero padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, q = lane >> 4;
    const long long r0 = (long long)blockIdx.x * 16;
    {
        const int r = threadIdx.x >> 4, d = threadIdx.x & 15;
        const bool live = r0 + r < a.R;
        const long long row = live ? r0 + r : a.R - 1;
        const long long xr = win_row(row, a.inner, a.S, a.tt);
        float v = 0.f;
        if (d < C) {
            const bool seen = a.msk[xr * C + d] != 0.f;
            const float dx2 = a.dcell ? a.dcell[row * a.ldc + d] : 0.f;
            v = (a.dP ? a.dP[xr * C + d] : 0.f) + (seen ? 0.f : dx2);
            if (live) {
                a.dp[row * C + d] = v;
                if (a.gx) a.gx[xr * C + d] = seen ? dx2 : 0.f;
            }
        }
        P[r * LDP + d] = v;
    }
    __syncthreads();
    const long long m = r0 + n;
    const bool ok = m < a.R;
    const long long mc = ok ? m : a.R - 1;
    const long long xr = win_row(mc, a.inner, a.S, a.tt);
    const float slope = a.slope[0];
    double part[1] = {0.0};
    for (int jt = wave; jt < 2 * JT; jt += kWaves) {
        const int col = 16 * jt + 4 * q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (a.dRepr)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = a.dRepr[xr * a.ldr + col + s];
        acc = tile_prod(a.w.ro, jt, 1, P + n * LDP + 4 * q, acc, lane);
        if (jt < JT) {
            const f32x4 pre = ld4(a.save_a + mc * H + col);
            f32x4 dpre;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                dpre[s] = pre[s] > 0.f ? acc[s] : slope * acc[s];
                if (ok && !(pre[s] > 0.f)) part[0] += (double)(acc[s] * pre[s]);
            }
            if (ok) st4(a.save_a + m * H + col, dpre);
            st4(D1 + n * LD + col, dpre);
        } else {
            st4(D1 + n * LD + col, acc);
        }
    }
    __syncthreads();
    for (int jt = wave; jt < 2 * JT; jt += kWaves) {
        const int col = 16 * jt + 4 * q;
        f32x4 acc = tile_prod(a.w.o, jt, JT, D1 + n * LD + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f}, lane);
        if (jt < JT) {
            st4(D2 + n * LD + col, acc);
            if (ok) st4(a.save_b + m * H + col, acc);
        } else if (ok) {
            float* c = a.carry + m * H + (col - H);
            st4(c, ld4(c) + (acc + ld4(D1 + n * LD + col)));
        }
    }
    __syncthreads();
    for (int jt = wave; jt < 2 * JT; jt += kWaves) {
        const int col = 16 * jt + 4 * q;
        const f32x4 acc = tile_prod(a.w.f, jt, JT, D2 + n * LD + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f}, lane);
        if (ok) {
            st4(a.dec + m * a.ldd + H + col, acc);
            if (jt < JT) st4(a.dec + m * a.ldd + col, f32x4{0.f, 0.f, 0.f, 0.f});
        }
    }
    sgp::wg_sum_waves<kThreads, 1>(part, red);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = (float)part[0];
}

// ---------------------------------------------------------------------------------------------- stage 1, backward
// d[x1 | m | hT | u] = W_in^T dz (dz: slot 0 of the decoder buffer's cotangent after the adjoint hop);
// dp1 = dP1 + (1 - m) dx1, gx += m dx1, gu = du + the cell input's u columns, carry += W_fs^T dp1 + dhT.
__global__ __launch_bounds__(kThreads) void grin_stage1_bwd(Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = a.H, C = a.C, U = a.U, K1 = 2 * C + H + U, JT = H / 16, KT = (K1 + 15) / 16;
    const int LDH = H + kPad, LDI = 16 * KT + kPad, LDP = 16 + kPad;
    float* Z = lds;                                         // [16][LDH]  dz
    float* I = lds + 16 * LDH;                              // [16][LDI]  d[x1 | m | hT | u]
    float* P = I + 16 * LDI;                                // [16][LDP]  dp1, zero padded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, q = lane >> 4;
    const long long r0 = (long long)blockIdx.x * 16;
    for (int i = threadIdx.x; i < 16 * H; i += kThreads) {
        const int r = i / H, c = i % H;
        const long long row = r0 + r < a.R ? r0 + r : a.R - 1;
        Z[r * LDH + c] = a.dec[row * a.ldd + c];
    }
    __syncthreads();
    for (int jt = wave; jt < KT; jt += kWaves)
        st4(I + n * LDI + 16 * jt + 4 * q, tile_prod(a.w.in, jt, JT, Z + n * LDH + 4 * q, f32x4{0.f, 0.f, 0.f, 0.f}, lane));
    __syncthreads();
    {
        const int r = threadIdx.x >> 4, d = threadIdx.x & 15;
        const bool live = r0 + r < a.R;
        const long long row = live ? r0 + r : a.R - 1;
        const long long xr = win_row(row, a.inner, a.S, a.tt);
        float v = 0.f;
        if (d < C) {
            const bool seen = a.msk[xr * C + d] != 0.f;
            const float dx1 = I[r * LDI + d];
            v = (a.dP ? a.dP[xr * C + d] : 0.f) + (seen ? 0.f : dx1);
            if (live) {
                a.dp[row * C + d] = v;
                if (a.gx && seen) a.gx[xr * C + d] += dx1;
            }
        }
        P[r * LDP + d] = v;
    }
    if (a.gu)
        for (int i = threadIdx.x; i < 16 * U; i += kThreads) {
            const int r = i / U, c = i % U;
            if (r0 + r < a.R)
                a.gu[win_row(r0 + r, a.inner, a.S, a.tt) * U + c] =
                    I[r * LDI + 2 * C + H + c] + (a.dcell ? a.dcell[(r0 + r) * a.ldc + 2 * C + c] : 0.f);
        }
    __syncthreads();
    const long long m = r0 + n;
    const bool ok = m < a.R;
    for (int jt = wave; jt < JT; jt += kWaves) {
        const int col = 16 * jt + 4 * q;
        f32x4 acc;
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = I[n * LDI + 2 * C + col + s];
        acc = tile_prod(a.w.fs, jt, 1, P + n * LDP + 4 * q, acc, lane);
        if (ok) {
            float* c = a.carry + m * H + col;
            st4(c, ld4(c) + acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ host side
const char* domain_error(int H, int C, int U) {
    if (H < 16 || H > 128 || H % 16) return "hidden size must be a multiple of 16 in 16 .. 128";
    if (C < 1 || C > 16) return "input size must be in 1 .. 16";
    if (U < 0 || U > 64) return "exogenous size must be in 0 .. 64";
    return nullptr;
}

enum Kernel { kStage1, kStage2, kStage2Bwd, kStage1Bwd };
size_t lds_bytes(Kernel k, const Dims& d) {
    const size_t h = 16 * (d.H + kPad), i = 16 * (16 * d.KT + kPad), w = 16 * (2 * d.H + kPad), p = 16 * (16 + kPad);
    switch (k) {
        case kStage1: return (h + i) * 4;
        case kStage2: return 2 * w * 4;
        case kStage2Bwd: return (2 * w + p) * 4;
        default: return (h + i + p) * 4;
    }
}

int check_common(const char* what, int H, int C, int U, int64_t R, int64_t inner, int S, int t, const float* packed) {
    if (const char* e = domain_error(H, C, U)) return sgp::fail(SGP_EUNSUP, "%s: %s (H %d, C %d, U %d)", what, e, H, C, U);
    SGP_REQUIRE(R >= 1 && R <= 0x7fffffffll - 16, "%s: bad row count %lld", what, (long long)R);
    SGP_REQUIRE(inner >= 1 && R % inner == 0, "%s: R %lld is no multiple of the node count %lld", what, (long long)R, (long long)inner);
    SGP_REQUIRE(S >= 1 && t >= 0 && t < S, "%s: step %d outside a window of %d", what, t, S);
    SGP_REQUIRE(packed && sgp::aligned16(packed), "%s: packed is null or not 16-byte aligned", what);
    return 0;
}

void fill(Args& a, int H, int C, int U, int64_t R, int64_t inner, int S, int t, int reverse) {
    a.H = H; a.C = C; a.U = U; a.R = R; a.inner = inner; a.S = S; a.tt = reverse ? S - 1 - t : t;
}

template <class K>
int run(K kernel, Kernel which, const Args& a, hipStream_t s, const char* what) {
    const Dims d(a.H, a.C, a.U);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.R + 15) / 16)), dim3(kThreads), lds_bytes(which, d), s, a);
    return sgp::check_launch(what);
}

bool vec_ok(const float* p, int64_t stride) { return p && sgp::aligned16(p) && stride % 4 == 0; }

}  // namespace

extern "C" {

int32_t sgp_grin_supported(int32_t H, int32_t C, int32_t U, int32_t k) {
    if (const char* e = domain_error(H, C, U)) {
        sgp::fail(SGP_EUNSUP, "sgp_grin_supported: %s (H %d, C %d, U %d)", e, H, C, U);
        return 0;
    }
    if (!sgp_dcrnn_supported(H, k)) return 0;               // the cells' own reason is in sgp_last_error
    return 1;
}

int64_t sgp_grin_packed_floats(int32_t H, int32_t C, int32_t U) {
    if (domain_error(H, C, U)) return -1;
    return 2 * Dims(H, C, U).dir();
}

int sgp_grin_plan(int32_t H, int32_t C, int32_t U, int64_t R, int32_t* plan) {
    if (const char* e = domain_error(H, C, U)) return sgp::fail(SGP_EUNSUP, "sgp_grin_plan: %s (H %d, C %d, U %d)", e, H, C, U);
    SGP_REQUIRE(plan && R >= 1 && R <= 0x7fffffffll - 16, "sgp_grin_plan: null pointer or bad size (R %lld)", (long long)R);
    const Dims d(H, C, U);
    plan[0] = d.JT;
    plan[1] = (d.JT + kWaves - 1) / kWaves;
    plan[2] = d.KT;
    plan[3] = (int32_t)((R + 15) / 16);
    plan[4] = (int32_t)lds_bytes(kStage1, d);
    plan[5] = (int32_t)lds_bytes(kStage2, d);
    plan[6] = (int32_t)lds_bytes(kStage2Bwd, d);
    plan[7] = (int32_t)lds_bytes(kStage1Bwd, d);
    return 0;
}

int sgp_grin_pack_f32(const float* w_fs, const float* w_in, const float* w_f, const float* w_o, const float* w_ro,
                      int32_t H, int32_t C, int32_t U, float* packed, sgp_stream_t stream) {
    if (const char* e = domain_error(H, C, U)) return sgp::fail(SGP_EUNSUP, "sgp_grin_pack_f32: %s (H %d, C %d, U %d)", e, H, C, U);
    SGP_REQUIRE(w_fs && w_in && w_f && w_o && w_ro && packed, "sgp_grin_pack_f32: null pointer");
    SGP_REQUIRE(sgp::aligned16(packed), "sgp_grin_pack_f32: packed must be 16-byte aligned");
    const Dims d(H, C, U);
    hipStream_t s = (hipStream_t)stream;
    auto run = [&](const float* src, int R, int Cc, int trans) { sgp::frag_pack_to(packed, src, Cc, R, Cc, trans, s); };   // src [R, Cc] contiguous
    for (int trans = 0; trans < 2; ++trans) {
        run(w_fs, C, H, trans);
        run(w_in, H, d.K1, trans);
        run(w_f, H, 2 * H, trans);
        run(w_o, H, 2 * H, trans);
        run(w_ro, C, 2 * H, trans);
    }
    return sgp::check_launch("sgp_grin_pack_f32");
}

int sgp_grin_stage1_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t, int32_t reverse,
                        const float* packed, const float* b_fs, const float* b_in, const float* hT, int64_t h_row_stride,
                        const float* x, const float* mask, const float* u, float* p1, float* dec, int64_t dec_row_stride,
                        float* save_in, sgp_stream_t stream) {
    const char* what = "sgp_grin_stage1_f32";
    if (int rc = check_common(what, H, C, U, R, inner, S, t, packed)) return rc;
    SGP_REQUIRE(b_fs && b_in && hT && x && mask && p1 && dec && (U == 0 || u), "%s: null pointer", what);
    SGP_REQUIRE(h_row_stride >= H && dec_row_stride >= 3 * H, "%s: a row stride is too small", what);
    SGP_REQUIRE(vec_ok(dec, dec_row_stride) && sgp::aligned16(b_in), "%s: dec and b_in must be 16-byte aligned, rows whole float4s", what);
    Args a{};
    fill(a, H, C, U, R, inner, S, t, reverse);
    a.w = parts(packed, Dims(H, C, U), false);
    a.b0 = b_fs; a.b1 = b_in; a.hT = hT; a.ldh = h_row_stride; a.x = x; a.msk = mask; a.u = u; a.p = p1;
    a.dec = dec; a.ldd = dec_row_stride; a.save_a = save_in;
    return run(grin_stage1, kStage1, a, (hipStream_t)stream, what);
}

int sgp_grin_stage2_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t, int32_t reverse,
                        const float* packed, const float* b_f, const float* b_o, const float* b_ro, const float* slope,
                        const float* dec, int64_t dec_row_stride, const float* hT, int64_t h_row_stride, const float* x,
                        const float* mask, const float* u, float* p2, float* repr, int64_t repr_row_stride,
                        float* cell_in, int64_t cell_row_stride, float* save_pre, float* save_cat, sgp_stream_t stream) {
    const char* what = "sgp_grin_stage2_f32";
    if (int rc = check_common(what, H, C, U, R, inner, S, t, packed)) return rc;
    SGP_REQUIRE(b_f && b_o && b_ro && slope && dec && hT && x && mask && p2 && cell_in && (U == 0 || u),
                "%s: null pointer", what);
    SGP_REQUIRE(!save_pre == !save_cat, "%s: the two save buffers come together", what);
    SGP_REQUIRE(h_row_stride >= H && dec_row_stride >= 3 * H && (!repr || repr_row_stride >= 2 * H) && cell_row_stride >= 2 * C + U,
                "%s: a row stride is too small", what);
    SGP_REQUIRE(sgp::aligned16(b_f) && sgp::aligned16(b_o) && (!save_pre || (sgp::aligned16(save_pre) && sgp::aligned16(save_cat))),
                "%s: b_f, b_o and the save buffers must be 16-byte aligned", what);
    Args a{};
    fill(a, H, C, U, R, inner, S, t, reverse);
    a.w = parts(packed, Dims(H, C, U), false);
    a.b0 = b_f; a.b1 = b_o; a.b2 = b_ro; a.slope = slope; a.dec = const_cast<float*>(dec); a.ldd = dec_row_stride;
    a.hT = hT; a.ldh = h_row_stride; a.x = x; a.msk = mask; a.u = u; a.p = p2; a.repr = repr; a.ldr = repr_row_stride;
    a.cell = cell_in; a.ldc = cell_row_stride; a.save_a = save_pre; a.save_b = save_cat;
    return run(grin_stage2, kStage2, a, (hipStream_t)stream, what);
}

int sgp_grin_stage2_bwd_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t,
                            int32_t reverse, const float* packed, const float* slope, const float* mask, const float* dP2,
                            const float* dRepr, int64_t drepr_row_stride, const float* dcell, int64_t cell_row_stride,
                            float* pre, float* dg, float* ddec, int64_t ddec_row_stride, float* carry, float* gx,
                            float* dp2, float* slope_partial, sgp_stream_t stream) {
    const char* what = "sgp_grin_stage2_bwd_f32";
    if (int rc = check_common(what, H, C, U, R, inner, S, t, packed)) return rc;
    SGP_REQUIRE(slope && mask && pre && dg && ddec && carry && dp2 && slope_partial, "%s: null pointer", what);
    SGP_REQUIRE((!dRepr || drepr_row_stride >= 2 * H) && (!dcell || cell_row_stride >= 2 * C + U) && ddec_row_stride >= 3 * H,
                "%s: a row stride is too small", what);
    SGP_REQUIRE(sgp::aligned16(pre) && sgp::aligned16(dg) && sgp::aligned16(carry) && vec_ok(ddec, ddec_row_stride),
                "%s: pre, dg, carry and ddec must be 16-byte aligned, rows whole float4s", what);
    Args a{};
    fill(a, H, C, U, R, inner, S, t, reverse);
    a.w = parts(packed, Dims(H, C, U), true);
    a.slope = slope; a.msk = mask; a.dP = dP2; a.dRepr = dRepr; a.ldr = drepr_row_stride; a.dcell = dcell;
    a.ldc = cell_row_stride; a.save_a = pre; a.save_b = dg; a.dec = ddec; a.ldd = ddec_row_stride; a.carry = carry;
    a.gx = gx; a.dp = dp2; a.partial = slope_partial;
    return run(grin_stage2_bwd, kStage2Bwd, a, (hipStream_t)stream, what);
}

int sgp_grin_stage1_bwd_f32(int32_t H, int32_t C, int32_t U, int64_t R, int64_t inner, int32_t S, int32_t t,
                            int32_t reverse, const float* packed, const float* mask, const float* dP1, const float* dcell,
                            int64_t cell_row_stride, const float* ddec, int64_t ddec_row_stride, float* carry, float* gx,
                            float* dp1, float* gu, sgp_stream_t stream) {
    const char* what = "sgp_grin_stage1_bwd_f32";
    if (int rc = check_common(what, H, C, U, R, inner, S, t, packed)) return rc;
    SGP_REQUIRE(mask && ddec && carry && dp1, "%s: null pointer", what);
    SGP_REQUIRE((!dcell || cell_row_stride >= 2 * C + U) && ddec_row_stride >= H, "%s: a row stride is too small", what);
    SGP_REQUIRE(sgp::aligned16(carry), "%s: carry must be 16-byte aligned", what);
    Args a{};
    fill(a, H, C, U, R, inner, S, t, reverse);
    a.w = parts(packed, Dims(H, C, U), true);
    a.msk = mask; a.dP = dP1; a.dcell = dcell; a.ldc = cell_row_stride; a.dec = const_cast<float*>(ddec);
    a.ldd = ddec_row_stride; a.carry = carry; a.gx = gx; a.dp = dp1; a.gu = U ? gu : nullptr;
    return run(grin_stage1_bwd, kStage1Bwd, a, (hipStream_t)stream, what);
}

}  // extern "C"
