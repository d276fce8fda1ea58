// Scaler fits and the fused scaler transform (include/sgp_amd.h "scalers").
//
// x is a row-major [M, G] fp32 matrix: M reduced rows, G groups (one bias / scale each).  An element counts iff its mask
// byte is set (no mask: every element) and it is not NaN.  Two launch regimes, chosen by sgp_amd.scalers.launch_plan:
//   long  (G <= 8):  rows are dealt to workgroups; fp64 partial sums per workgroup, a second stage adds them in a fixed
//                    order; the select is a 4-pass radix select on 8-bit digits, per-workgroup LDS histograms merged
//                    into global integer histograms, one small scan kernel per digit.
//   many  (any G):   a workgroup owns `tile_cols` adjacent columns and walks down all rows (neighbouring lanes on
//                    neighbouring columns); everything stays in LDS: 8 passes on 4-bit digits, no global merge.
// Order-preserving keys: negatives have all bits flipped, the rest the sign bit.  Up to 6 ranks per group (floor and
// ceil of three quantiles); ranks that still share a prefix share a histogram slot.  No float atomics anywhere.
#include "wg.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int THREADS = 256;
constexpr int LONG_MAX_G = 8;
constexpr int NRANK = 6;
constexpr int MAX_TILE = 64;
// stats [6, G] fp64: count | mean | sum of squared deviations | min | max | NaN seen among the unmasked
enum { ST_COUNT = 0, ST_MEAN = 1, ST_M2 = 2, ST_MIN = 3, ST_MAX = 4, ST_NAN = 5, NSTAT = 6 };

struct SelState {                       // per group, long regime (global memory)
    unsigned pref[NRANK];               // distinct key prefixes still alive (slots 0 .. npref - 1)
    int slot[NRANK];                    // rank k looks in slot[k]
    int npref, pad;
    unsigned long long rem[NRANK];      // rank k inside its prefix
};

__device__ inline unsigned key_of(float v) {
    unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float val_of(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// numpy's linear method: virtual index q / 100 * (n - 1), its floor, the next rank and the fraction
__device__ inline void rank_of(long long n, double q, long long& lo, long long& hi, double& frac) {
    if (n <= 0) { lo = hi = 0; frac = 0.0; return; }
    double vi = q / 100.0 * (double)(n - 1);
    double f = floor(vi);
    if (!(f >= 0.0)) f = 0.0;
    if (f > (double)(n - 1)) f = (double)(n - 1);
    lo = (long long)f;
    hi = lo + 1 < n ? lo + 1 : n - 1;
    frac = vi - f;
    if (!(frac >= 0.0)) frac = 0.0;
    if (frac > 1.0) frac = 1.0;
}

// ---------------------------------------------------------------------------------------------- long: moments
// PASS 1: count, sum, min, max, NaN flag; PASS 2: sum of squared deviations from stats' mean.  part: per workgroup and
// group 5 (PASS 1) or 1 (PASS 2) doubles.
template <int PASS>
__global__ __launch_bounds__(THREADS) void moments_long_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                               int mask_div, long long m, int g, long long rows_per_wg,
                                                               const double* __restrict__ stats, double* __restrict__ part) {
    __shared__ double s_sum[THREADS];
    __shared__ float s_mn[THREADS], s_mx[THREADS];
    __shared__ unsigned s_cnt[THREADS], s_nan[THREADS];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * rows_per_wg;
    const long long r1 = r0 + rows_per_wg < m ? r0 + rows_per_wg : m;
    const int gm = g / mask_div;
    double sum[LONG_MAX_G], mean[LONG_MAX_G];
    float mn[LONG_MAX_G], mx[LONG_MAX_G];
    unsigned cnt[LONG_MAX_G], nanf = 0;
#pragma unroll
    for (int u = 0; u < LONG_MAX_G; ++u) {
        sum[u] = 0.0; mn[u] = INFINITY; mx[u] = -INFINITY; cnt[u] = 0;
        mean[u] = (PASS == 2 && u < g) ? stats[(long long)ST_MEAN * g + u] : 0.0;
    }
    for (long long row = r0 + tid; row < r1; row += THREADS) {
        const float* xr = x + row * g;
        const uint8_t* mr = mask ? mask + row * gm : nullptr;
#pragma unroll
        for (int u = 0; u < LONG_MAX_G; ++u) {
            if (u < g) {
                float v = xr[u];
                bool on = mr ? mr[u / mask_div] != 0 : true;
                if (on) {
                    if (v != v) nanf |= 1u << u;
                    else if (PASS == 1) { cnt[u] += 1; sum[u] += (double)v; mn[u] = fminf(mn[u], v); mx[u] = fmaxf(mx[u], v); }
                    else { double d = (double)v - mean[u]; sum[u] += d * d; }
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < LONG_MAX_G; ++u) {
        if (u < g) {                                             // (g is uniform: the barriers below are too)
            s_sum[tid] = sum[u];
            if (PASS == 1) { s_mn[tid] = mn[u]; s_mx[tid] = mx[u]; s_cnt[tid] = cnt[u]; s_nan[tid] = (nanf >> u) & 1u; }
            sgp::wg_reduce<THREADS>([&](int a, int b) {
                s_sum[a] += s_sum[b];
                if (PASS == 1) {
                    s_mn[a] = fminf(s_mn[a], s_mn[b]); s_mx[a] = fmaxf(s_mx[a], s_mx[b]);
                    s_cnt[a] += s_cnt[b]; s_nan[a] |= s_nan[b];
                }
            });
            if (tid == 0) {
                if (PASS == 1) {
                    double* p = part + ((long long)blockIdx.x * g + u) * 5;
                    p[0] = (double)s_cnt[0]; p[1] = s_sum[0]; p[2] = (double)s_mn[0]; p[3] = (double)s_mx[0]; p[4] = (double)s_nan[0];
                } else {
                    part[(long long)blockIdx.x * g + u] = s_sum[0];
                }
            }
            __syncthreads();
        }
    }
}

// second stage: block u adds the workgroups' partials of group u, every thread a fixed subset in ascending order
template <int PASS>
__global__ __launch_bounds__(THREADS) void moments_reduce_kernel(const double* __restrict__ part, long long nwg, int g,
                                                                 double* __restrict__ stats) {
    __shared__ double s_a[THREADS], s_b[THREADS], s_mn[THREADS], s_mx[THREADS], s_nan[THREADS];
    const int tid = threadIdx.x, u = blockIdx.x;
    double a = 0.0, b = 0.0, mn = INFINITY, mx = -INFINITY, nf = 0.0;
    for (long long w = tid; w < nwg; w += THREADS) {
        if (PASS == 1) {
            const double* p = part + (w * g + u) * 5;
            a += p[0]; b += p[1]; mn = fmin(mn, p[2]); mx = fmax(mx, p[3]); nf = fmax(nf, p[4]);
        } else {
            b += part[w * g + u];
        }
    }
    s_a[tid] = a; s_b[tid] = b; s_mn[tid] = mn; s_mx[tid] = mx; s_nan[tid] = nf;
    sgp::wg_reduce<THREADS>([&](int a, int b) {
        s_a[a] += s_a[b]; s_b[a] += s_b[b];
        s_mn[a] = fmin(s_mn[a], s_mn[b]); s_mx[a] = fmax(s_mx[a], s_mx[b]);
        s_nan[a] = fmax(s_nan[a], s_nan[b]);
    });
    if (tid == 0) {
        const long long G = g;
        if (PASS == 1) {
            stats[ST_COUNT * G + u] = s_a[0];
            stats[ST_MEAN * G + u] = s_a[0] > 0.0 ? s_b[0] / s_a[0] : (double)NAN;
            stats[ST_M2 * G + u] = 0.0;
            stats[ST_MIN * G + u] = s_mn[0]; stats[ST_MAX * G + u] = s_mx[0]; stats[ST_NAN * G + u] = s_nan[0];
        } else {
            stats[ST_M2 * G + u] = s_b[0];
        }
    }
}

// ---------------------------------------------------------------------------------------------- many: moments
// thread = (row lane rl, column c) of the tile; both passes in one launch, the row lanes' partials added in lane order
__global__ __launch_bounds__(THREADS) void moments_many_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                               long long mask_div, long long m, long long g, int tc,
                                                               int want_var, double* __restrict__ stats) {
    __shared__ double s_sum[THREADS], s_mean[MAX_TILE];
    __shared__ float s_mn[THREADS], s_mx[THREADS];
    __shared__ unsigned s_cnt[THREADS], s_nan[THREADS];
    const int tid = threadIdx.x, rl = tid / tc, c = tid % tc, nrl = THREADS / tc;
    const long long col = (long long)blockIdx.x * tc + c;
    const bool live = col < g;
    const long long gm = g / mask_div, mcol = col / mask_div;
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    unsigned cnt = 0, nanf = 0;
    if (live) {
#pragma unroll 4
        for (long long row = rl; row < m; row += nrl) {
            float v = x[row * g + col];
            bool on = mask ? mask[row * gm + mcol] != 0 : true;
            if (on) {
                if (v != v) nanf = 1;
                else { cnt += 1; sum += (double)v; mn = fminf(mn, v); mx = fmaxf(mx, v); }
            }
        }
    }
    s_sum[tid] = sum; s_mn[tid] = mn; s_mx[tid] = mx; s_cnt[tid] = cnt; s_nan[tid] = nanf;
    __syncthreads();
    if (rl == 0) {
        double n = (double)cnt;
        for (int k = 1; k < nrl; ++k) {
            int j = k * tc + c;
            sum += s_sum[j]; n += (double)s_cnt[j]; mn = fminf(mn, s_mn[j]); mx = fmaxf(mx, s_mx[j]); nanf |= s_nan[j];
        }
        double mean = n > 0.0 ? sum / n : (double)NAN;
        s_mean[c] = mean;
        if (live) {
            stats[ST_COUNT * g + col] = n; stats[ST_MEAN * g + col] = mean; stats[ST_M2 * g + col] = 0.0;
            stats[ST_MIN * g + col] = (double)mn; stats[ST_MAX * g + col] = (double)mx; stats[ST_NAN * g + col] = (double)nanf;
        }
    }
    if (!want_var) return;                                       // (uniform)
    __syncthreads();
    const double mean = s_mean[c];
    sum = 0.0;
    if (live) {
#pragma unroll 4
        for (long long row = rl; row < m; row += nrl) {
            float v = x[row * g + col];
            bool on = mask ? mask[row * gm + mcol] != 0 : true;
            if (on && v == v) { double d = (double)v - mean; sum += d * d; }
        }
    }
    __syncthreads();                                             // (s_sum of pass 1 has been read)
    s_sum[tid] = sum;
    __syncthreads();
    if (rl == 0 && live) {
        for (int k = 1; k < nrl; ++k) sum += s_sum[k * tc + c];
        stats[ST_M2 * g + col] = sum;
    }
}

// ---------------------------------------------------------------------------------------------- long: select
__global__ void select_init_kernel(const double* __restrict__ stats, int g, double q0, double q1, double q2,
                                   SelState* __restrict__ state) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= g) return;
    const long long n = (long long)stats[(long long)ST_COUNT * g + u];
    SelState st;
    const double q[3] = {q0, q1, q2};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        long long lo, hi; double frac;
        rank_of(n, q[j], lo, hi, frac);
        st.rem[2 * j] = (unsigned long long)lo; st.rem[2 * j + 1] = (unsigned long long)hi;
    }
#pragma unroll
    for (int k = 0; k < NRANK; ++k) { st.pref[k] = 0; st.slot[k] = 0; }
    st.npref = 1; st.pad = 0;
    state[u] = st;
}

// one LDS increment per lane, the lanes that agree with the first valid lane's bin folded into one add (a value that
// fills half a group would otherwise serialise the wave on one LDS word)
__device__ inline void lds_add_folded(unsigned* lh, int addr) {
    const unsigned long long valid = __ballot(addr >= 0);
    if (valid == 0) return;
    const int leader = __builtin_ctzll(valid);
    const int cand = __shfl(addr, leader);
    const unsigned long long same = __ballot(addr == cand);
    const int lane = threadIdx.x & 63;
    if (lane == leader) atomicAdd(&lh[cand], (unsigned)__popcll(same));
    else if (addr >= 0 && addr != cand) atomicAdd(&lh[addr], 1u);
}

// digit d (0 = most significant byte): LDS histograms [g][slot][256] of the elements whose key prefix is alive, merged
// into hist (same layout, 64-bit) with integer atomics
__global__ __launch_bounds__(THREADS) void select_hist_long_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                                   int mask_div, long long m, int g, long long rows_per_wg,
                                                                   const SelState* __restrict__ state,
                                                                   unsigned long long* __restrict__ hist, int d) {
    extern __shared__ unsigned lh[];                             // g * NRANK * 256
    __shared__ unsigned s_pref[LONG_MAX_G * NRANK];
    __shared__ int s_np[LONG_MAX_G];
    const int tid = threadIdx.x;
    const int nbins = g * NRANK * 256;
    if (tid < g * NRANK) s_pref[tid] = state[tid / NRANK].pref[tid % NRANK];
    if (tid < g) s_np[tid] = state[tid].npref;
    for (int i = tid; i < nbins; i += THREADS) lh[i] = 0;
    __syncthreads();
    const long long r0 = (long long)blockIdx.x * rows_per_wg;
    const long long r1 = r0 + rows_per_wg < m ? r0 + rows_per_wg : m;
    const int gm = g / mask_div;
    const int shift = 24 - 8 * d;
    for (long long base = r0; base < r1; base += THREADS) {      // (uniform trip count: the folded add uses ballots)
        const long long row = base + tid;
        const bool active = row < r1;
        const float* xr = x + (active ? row : r0) * g;
        const uint8_t* mr = mask ? mask + (active ? row : r0) * gm : nullptr;
#pragma unroll
        for (int u = 0; u < LONG_MAX_G; ++u) {
            if (u < g) {
                int addr = -1;
                float v = xr[u];
                bool on = active && (mr ? mr[u / mask_div] != 0 : true);
                if (on && v == v) {
                    const unsigned key = key_of(v);
                    const unsigned hi = d ? key >> (shift + 8) : 0u;
                    const int dg = (int)((key >> shift) & 255u);
                    const int np = s_np[u];
#pragma unroll
                    for (int p = 0; p < NRANK; ++p)
                        if (p < np && s_pref[u * NRANK + p] == hi) addr = (u * NRANK + p) * 256 + dg;
                }
                lds_add_folded(lh, addr);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < nbins; i += THREADS) {
        const unsigned v = lh[i];
        if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
}

// block u: every rank of group u finds its bin in its slot's histogram; thread 0 regroups the new prefixes into slots
__global__ void select_scan_kernel(SelState* __restrict__ state, const unsigned long long* __restrict__ hist, int d,
                                   float* __restrict__ ostat) {
    __shared__ unsigned s_newp[NRANK];
    __shared__ unsigned long long s_rem[NRANK];
    const int u = blockIdx.x, k = threadIdx.x;
    SelState* st = state + u;
    if (k < NRANK) {
        const int s = st->slot[k];
        const unsigned long long rem = st->rem[k];
        const unsigned long long* h = hist + (long long)(u * NRANK + s) * 256;
        unsigned long long cum = 0;
        int b = 0;
        for (; b < 256; ++b) {
            const unsigned long long hv = h[b];
            if (cum + hv > rem) break;
            cum += hv;
        }
        if (b == 256) { b = 255; cum = rem; }                    // (an empty group: nothing to find)
        s_newp[k] = (st->pref[s] << 8) | (unsigned)b;
        s_rem[k] = rem - cum;
    }
    __syncthreads();
    if (k == 0) {
        unsigned prefs[NRANK];
        int np = 0;
        for (int r = 0; r < NRANK; ++r) {
            int j = 0;
            for (; j < np; ++j) if (prefs[j] == s_newp[r]) break;
            if (j == np) { prefs[np] = s_newp[r]; st->pref[np] = s_newp[r]; ++np; }
            st->slot[r] = j;
            st->rem[r] = s_rem[r];
            if (d == 3) ostat[(long long)u * NRANK + r] = val_of(s_newp[r]);
        }
        st->npref = np;
    }
}

// ---------------------------------------------------------------------------------------------- many: select
__global__ __launch_bounds__(THREADS) void select_many_kernel(const float* __restrict__ x, const uint8_t* __restrict__ mask,
                                                              long long mask_div, long long m, long long g, int tc,
                                                              const double* __restrict__ stats, double q0, double q1, double q2,
                                                              float* __restrict__ ostat) {
    __shared__ unsigned hist[MAX_TILE * NRANK * 16];             // [column][slot][16]
    __shared__ unsigned pref[MAX_TILE * NRANK], newp[MAX_TILE * NRANK], rem[MAX_TILE * NRANK];
    __shared__ int slot[MAX_TILE * NRANK], np[MAX_TILE];
    const int tid = threadIdx.x, rl = tid / tc, c = tid % tc, nrl = THREADS / tc;
    const long long col0 = (long long)blockIdx.x * tc, col = col0 + c;
    const bool live = col < g;
    const long long gm = g / mask_div, mcol = col / mask_div;
    for (int i = tid; i < tc * NRANK; i += THREADS) {
        const int cc = i / NRANK, k = i % NRANK;
        const long long n = col0 + cc < g ? (long long)stats[ST_COUNT * g + col0 + cc] : 0;
        long long lo, hi; double frac;
        rank_of(n, k < 2 ? q0 : k < 4 ? q1 : q2, lo, hi, frac);
        rem[i] = (unsigned)((k & 1) ? hi : lo);
        slot[i] = 0; pref[i] = 0;
    }
    for (int i = tid; i < tc; i += THREADS) np[i] = 1;
    __syncthreads();
    for (int d = 0; d < 8; ++d) {
        const int shift = 28 - 4 * d;
        for (int i = tid; i < tc * NRANK * 16; i += THREADS) hist[i] = 0;
        __syncthreads();
        const int npc = np[c];
        unsigned pr[NRANK];
#pragma unroll
        for (int p = 0; p < NRANK; ++p) pr[p] = pref[c * NRANK + p];
        if (live) {
#pragma unroll 4
            for (long long row = rl; row < m; row += nrl) {
                float v = x[row * g + col];
                bool on = mask ? mask[row * gm + mcol] != 0 : true;
                if (on && v == v) {
                    const unsigned key = key_of(v);
                    const unsigned hi = d ? key >> (shift + 4) : 0u;
                    const int dg = (int)((key >> shift) & 15u);
#pragma unroll
                    for (int p = 0; p < NRANK; ++p)
                        if (p < npc && pr[p] == hi) atomicAdd(&hist[(c * NRANK + p) * 16 + dg], 1u);
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < tc * NRANK; i += THREADS) {
            const int cc = i / NRANK, s = slot[i];
            const unsigned r = rem[i];
            const unsigned* h = &hist[(cc * NRANK + s) * 16];
            unsigned cum = 0;
            int b = 0;
            for (; b < 16; ++b) {
                const unsigned hv = h[b];
                if (cum + hv > r) break;
                cum += hv;
            }
            if (b == 16) { b = 15; cum = r; }
            newp[i] = (pref[cc * NRANK + s] << 4) | (unsigned)b;
            rem[i] = r - cum;
        }
        __syncthreads();
        for (int cc = tid; cc < tc; cc += THREADS) {
            int n_new = 0;
            for (int r = 0; r < NRANK; ++r) {
                const unsigned want = newp[cc * NRANK + r];
                int j = 0;
                for (; j < n_new; ++j) if (pref[cc * NRANK + j] == want) break;
                if (j == n_new) { pref[cc * NRANK + n_new] = want; ++n_new; }
                slot[cc * NRANK + r] = j;
            }
            np[cc] = n_new;
        }
        __syncthreads();
    }
    for (int i = tid; i < tc * NRANK; i += THREADS) {
        const int cc = i / NRANK;
        if (col0 + cc < g) ostat[(col0 + cc) * NRANK + i % NRANK] = val_of(pref[cc * NRANK + slot[i]]);
    }
}

// ---------------------------------------------------------------------------------------------- finish
__device__ inline double lerp_np(double a, double b, double t) {          // numpy's _lerp
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// kind 0 standard (mean, population std), 1 min-max (p0, p1 = output range), 2 robust (p0, p1 = quantile range in
// percent, adjust: 0 or the unit-variance divisor); fp64 throughout, one rounding to fp32
__global__ void finish_kernel(int kind, const double* __restrict__ stats, const float* __restrict__ ostat, long long g,
                              int has_mask, double p0, double p1, double adjust, float* __restrict__ bias,
                              float* __restrict__ scale) {
    const long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= g) return;
    const double n = stats[ST_COUNT * g + u];
    const bool bad = !(n > 0.0) || (!has_mask && stats[ST_NAN * g + u] != 0.0);
    double b = 0.0, s = 1.0;
    if (kind == 0) {
        b = stats[ST_MEAN * g + u];
        s = sqrt(stats[ST_M2 * g + u] / n);
    } else if (kind == 1) {
        b = stats[ST_MIN * g + u];
        s = (stats[ST_MAX * g + u] - b) / (p1 - p0);
    } else {
        const float* o = ostat + u * NRANK;
        const double q[3] = {p0, 50.0, p1};
        double v[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            long long lo, hi; double frac;
            rank_of((long long)n, q[j], lo, hi, frac);
            v[j] = lerp_np((double)o[2 * j], (double)o[2 * j + 1], frac);
        }
        b = v[1];
        s = v[2] - v[0];
    }
    float sf = (float)s;
    if (fabsf(sf) <= 10.0f * 1.1920928955078125e-7f) { sf = 1.0f; s = 1.0; }      // zeros_to_one_ (NaN stays NaN)
    if (kind == 1) b = b - p0 * s;
    if (kind == 2 && adjust != 0.0) sf = (float)(s / adjust);
    float bf = (float)b;
    if (bad) { bf = NAN; sf = NAN; }
    bias[u] = bf;
    scale[u] = sf;
}

// ---------------------------------------------------------------------------------------------- apply
__device__ inline float apply_one(float x, float b, float s, int inverse) {
    // torch's unfused fp32 evaluation: IEEE division, and no FMA.  The build contracts in the backend
    // (-ffp-contract=fast), where neither the _rn intrinsics (plain operators to the compiler) nor a contract pragma
    // hold it back: the product goes through an empty asm, which the combiner cannot see through.
    if (inverse) {
        float t = x * (s + 5e-8f);
        asm volatile("" : "+v"(t));
        return t + b;
    }
    return (x - b) / s + 5e-8f;
}

template <typename I>
__global__ __launch_bounds__(THREADS) void apply_kernel(const float* x, float* out, const float* __restrict__ bias,
                                                        const float* __restrict__ scale, I n, I np, int inverse, int vec) {
    const I i0 = ((I)blockIdx.x * THREADS + threadIdx.x) * 4;
    if (i0 >= n) return;
    I p = i0 % np;
    if (vec && n - i0 >= 4) {
        sgp::f32x4 v = *reinterpret_cast<const sgp::f32x4*>(x + i0), r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            r[j] = apply_one(v[j], bias[p], scale[p], inverse);
            p = p + 1 == np ? 0 : p + 1;
        }
        *reinterpret_cast<sgp::f32x4*>(out + i0) = r;
    } else {
        float v[4];
        const int cnt = n - i0 >= 4 ? 4 : (int)(n - i0);
        for (int j = 0; j < cnt; ++j) v[j] = x[i0 + j];          // (all reads before the writes: out may be x)
        for (int j = 0; j < cnt; ++j) {
            out[i0 + j] = apply_one(v[j], bias[p], scale[p], inverse);
            p = p + 1 == np ? 0 : p + 1;
        }
    }
}

// ---------------------------------------------------------------------------------------------- host
struct LongLayout { long long nwg, part1, part2, state, hist, total; };

bool long_layout(long long m, long long g, long long rows_per_wg, LongLayout& L) {
    if (m <= 0 || g <= 0 || g > LONG_MAX_G || rows_per_wg <= 0 || rows_per_wg > INT_MAX) return false;
    L.nwg = (m + rows_per_wg - 1) / rows_per_wg;
    if (L.nwg > (1ll << 22)) return false;
    auto up = [](long long b) { return (b + 255) / 256 * 256; };
    L.part1 = 0;
    L.part2 = L.part1 + up(L.nwg * g * 5 * 8);
    L.state = L.part2 + up(L.nwg * g * 8);
    L.hist = L.state + up(g * (long long)sizeof(SelState));
    L.total = L.hist + up(4ll * g * NRANK * 256 * 8);
    return true;
}

bool tile_ok(int tc) { return tc == 16 || tc == 32 || tc == 64; }

int check_common(const char* what, long long mask_div, long long m, long long g, int regime, long long rows_per_wg, int tile_cols) {
    SGP_REQUIRE(m > 0 && g > 0, "%s: sizes must be positive (m=%lld, g=%lld)", what, m, g);
    SGP_REQUIRE(m <= (1ll << 40) / g, "%s: %lld x %lld elements are out of range", what, m, g);
    SGP_REQUIRE(mask_div >= 1 && g % mask_div == 0, "%s: mask_div %lld does not divide g=%lld", what, mask_div, g);
    SGP_REQUIRE(regime == 0 || regime == 1, "%s: regime must be 0 (long) or 1 (many)", what);
    if (regime == 0) {
        SGP_REQUIRE(g <= LONG_MAX_G, "%s: the long regime serves g <= %d (got %lld)", what, LONG_MAX_G, g);
        LongLayout L;
        SGP_REQUIRE(long_layout(m, g, rows_per_wg, L), "%s: bad rows_per_wg %lld for m=%lld", what, rows_per_wg, m);
    } else {
        SGP_REQUIRE(tile_ok(tile_cols), "%s: tile_cols must be 16, 32 or 64 (got %d)", what, tile_cols);
        SGP_REQUIRE((g + tile_cols - 1) / tile_cols <= INT_MAX && m <= INT_MAX, "%s: m=%lld, g=%lld exceed the many regime", what, m, g);
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t sgp_scaler_workspace_bytes(int64_t m, int64_t g, int32_t regime, int64_t rows_per_wg) {
    if (regime == 1) return m > 0 && g > 0 ? 256 : -1;
    LongLayout L;
    if (regime != 0 || !long_layout(m, g, rows_per_wg, L)) return -1;
    return L.total;
}

int sgp_scaler_moments_f32(const float* x, const uint8_t* mask, int64_t mask_div, int64_t m, int64_t g, int32_t want_var,
                           int32_t regime, int64_t rows_per_wg, int32_t tile_cols, double* stats, void* ws,
                           int64_t ws_bytes, sgp_stream_t stream) {
    SGP_REQUIRE(x && stats, "sgp_scaler_moments_f32: null pointer");
    if (int rc = check_common("sgp_scaler_moments_f32", mask_div, m, g, regime, rows_per_wg, tile_cols)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (regime == 1) {
        const unsigned grid = (unsigned)((g + tile_cols - 1) / tile_cols);
        hipLaunchKernelGGL(moments_many_kernel, dim3(grid), dim3(THREADS), 0, s, x, mask, (long long)mask_div, (long long)m,
                           (long long)g, (int)tile_cols, (int)(want_var != 0), stats);
        return sgp::check_launch("sgp_scaler_moments_f32");
    }
    LongLayout L;
    long_layout(m, g, rows_per_wg, L);
    SGP_REQUIRE(ws && ws_bytes >= L.total, "sgp_scaler_moments_f32: workspace of %lld bytes needed", L.total);
    char* w = (char*)ws;
    double* part1 = (double*)(w + L.part1);
    double* part2 = (double*)(w + L.part2);
    hipLaunchKernelGGL(moments_long_kernel<1>, dim3((unsigned)L.nwg), dim3(THREADS), 0, s, x, mask, (int)mask_div, (long long)m,
                       (int)g, (long long)rows_per_wg, (const double*)stats, part1);
    hipLaunchKernelGGL(moments_reduce_kernel<1>, dim3((unsigned)g), dim3(THREADS), 0, s, (const double*)part1, L.nwg, (int)g, stats);
    if (want_var) {
        hipLaunchKernelGGL(moments_long_kernel<2>, dim3((unsigned)L.nwg), dim3(THREADS), 0, s, x, mask, (int)mask_div,
                           (long long)m, (int)g, (long long)rows_per_wg, (const double*)stats, part2);
        hipLaunchKernelGGL(moments_reduce_kernel<2>, dim3((unsigned)g), dim3(THREADS), 0, s, (const double*)part2, L.nwg, (int)g, stats);
    }
    return sgp::check_launch("sgp_scaler_moments_f32");
}

int sgp_scaler_select_f32(const float* x, const uint8_t* mask, int64_t mask_div, int64_t m, int64_t g, const double* stats,
                          double q_lo, double q_mid, double q_hi, int32_t regime, int64_t rows_per_wg, int32_t tile_cols,
                          float* ostat, void* ws, int64_t ws_bytes, sgp_stream_t stream) {
    SGP_REQUIRE(x && stats && ostat, "sgp_scaler_select_f32: null pointer");
    if (int rc = check_common("sgp_scaler_select_f32", mask_div, m, g, regime, rows_per_wg, tile_cols)) return rc;
    SGP_REQUIRE(q_lo >= 0.0 && q_lo <= 100.0 && q_mid >= 0.0 && q_mid <= 100.0 && q_hi >= 0.0 && q_hi <= 100.0,
                "sgp_scaler_select_f32: quantiles must lie in [0, 100]");
    hipStream_t s = (hipStream_t)stream;
    if (regime == 1) {
        const unsigned grid = (unsigned)((g + tile_cols - 1) / tile_cols);
        hipLaunchKernelGGL(select_many_kernel, dim3(grid), dim3(THREADS), 0, s, x, mask, (long long)mask_div, (long long)m,
                           (long long)g, (int)tile_cols, stats, q_lo, q_mid, q_hi, ostat);
        return sgp::check_launch("sgp_scaler_select_f32");
    }
    LongLayout L;
    long_layout(m, g, rows_per_wg, L);
    SGP_REQUIRE(ws && ws_bytes >= L.total, "sgp_scaler_select_f32: workspace of %lld bytes needed", L.total);
    char* w = (char*)ws;
    SelState* state = (SelState*)(w + L.state);
    unsigned long long* hist = (unsigned long long*)(w + L.hist);
    const long long per_digit = (long long)g * NRANK * 256;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)(4 * per_digit * 8), s);
    if (e != hipSuccess) return sgp::fail((int)e, "sgp_scaler_select_f32: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(64), 0, s, stats, (int)g, q_lo, q_mid, q_hi, state);
    const size_t lds = (size_t)per_digit * sizeof(unsigned);
    for (int d = 0; d < 4; ++d) {
        hipLaunchKernelGGL(select_hist_long_kernel, dim3((unsigned)L.nwg), dim3(THREADS), lds, s, x, mask, (int)mask_div,
                           (long long)m, (int)g, (long long)rows_per_wg, (const SelState*)state, hist + d * per_digit, d);
        hipLaunchKernelGGL(select_scan_kernel, dim3((unsigned)g), dim3(64), 0, s, state,
                           (const unsigned long long*)(hist + d * per_digit), d, ostat);
    }
    return sgp::check_launch("sgp_scaler_select_f32");
}

int sgp_scaler_finish_f32(int32_t kind, const double* stats, const float* ostat, int64_t g, int32_t has_mask, double p0,
                          double p1, double adjust, float* bias, float* scale, sgp_stream_t stream) {
    SGP_REQUIRE(stats && bias && scale && (kind != 2 || ostat), "sgp_scaler_finish_f32: null pointer");
    SGP_REQUIRE(g > 0 && g <= (1ll << 40), "sgp_scaler_finish_f32: g must be positive (got %lld)", (long long)g);
    SGP_REQUIRE(kind >= 0 && kind <= 2, "sgp_scaler_finish_f32: kind must be 0, 1 or 2");
    SGP_REQUIRE(kind != 1 || p0 < p1, "sgp_scaler_finish_f32: empty output range");
    const unsigned grid = (unsigned)((g + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(finish_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, (int)kind, stats, ostat, (long long)g,
                       (int)(has_mask != 0), p0, p1, adjust, bias, scale);
    return sgp::check_launch("sgp_scaler_finish_f32");
}

int sgp_scaler_apply_f32(const float* x, float* out, const float* bias, const float* scale, int64_t n, int64_t n_params,
                         int32_t inverse, sgp_stream_t stream) {
    SGP_REQUIRE(x && out && bias && scale, "sgp_scaler_apply_f32: null pointer");
    SGP_REQUIRE(n > 0 && n_params > 0 && n_params <= n && n <= (1ll << 40),
                "sgp_scaler_apply_f32: bad sizes (n=%lld, n_params=%lld)", (long long)n, (long long)n_params);
    const int vec = sgp::aligned16(x) && sgp::aligned16(out);
    const long long grid = (n + 4 * THREADS - 1) / (4 * THREADS);
    SGP_REQUIRE(grid <= INT_MAX, "sgp_scaler_apply_f32: n=%lld is out of range", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    if (n < (1ll << 31))
        hipLaunchKernelGGL(apply_kernel<unsigned>, dim3((unsigned)grid), dim3(THREADS), 0, s, x, out, bias, scale, (unsigned)n,
                           (unsigned)n_params, (int)(inverse != 0), vec);
    else
        hipLaunchKernelGGL(apply_kernel<long long>, dim3((unsigned)grid), dim3(THREADS), 0, s, x, out, bias, scale, (long long)n,
                           (long long)n_params, (int)(inverse != 0), vec);
    return sgp::check_launch("sgp_scaler_apply_f32");
}

}  // extern "C"
