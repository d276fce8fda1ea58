// C ABI of the windowed last-state reservoir (kernel: reservoir_window_impl.h) + its weight packing, and the
// instances for R <= 32 (the wider ones: reservoir_window_mid.hip, reservoir_window_mid_stream.hip, reservoir_window_wide.hip).
#include "reservoir_window_impl.h"

namespace sgp_win {
WinKernel resolve_narrow(int jt, int L) {
    const auto ls = std::make_integer_sequence<int, 8>{};
    return jt == 1 ? pick_layers<1, true>(L, ls) : jt == 2 ? pick_layers<2, true>(L, ls) : nullptr;
}
}  // namespace sgp_win

namespace {
using namespace sgp_win;

// one layer into the layout at the head of reservoir_window_impl.h: w_ih [R, Fin], w_hh [R, R], b [R]
__global__ void pack_window_layer(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b,
                                  float* __restrict__ out, int Fin, int R, int JT, int NK) {
    const long long n_bias = (long long)JT * 16, n_wx = (long long)JT * NK * 256, total = layer_floats(JT, NK);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i < n_bias) {
            v = i < R ? b[i] : 0.f;
        } else {
            const bool in = i < n_bias + n_wx;
            const long long o = i - n_bias - (in ? 0 : n_wx);
            const int nk = in ? NK : JT, width = in ? Fin : R;
            const int s = (int)(o & 3), l = (int)((o >> 2) & 63);
            const int kb = (int)((o >> 8) % nk), jt = (int)((o >> 8) / nk);
            const int j = 16 * jt + (l & 15), k = 16 * kb + 4 * (l >> 4) + s;
            v = (j < R && k < width) ? (in ? w_ih : w_hh)[(long long)j * width + k] : 0.f;
        }
        out[i] = v;
    }
}

struct WinPlan {
    int mode;            // 0: unsupported, 1: all layers in one launch, 2: layer by layer over one [S, M, R] intermediate
    int jt, nk0, nkd;    // register tiles per layer; 16-feature input chunks of layer 0 / of a deeper layer
    bool lds;            // weights in LDS (else streamed from the packed buffer through L2)
    long long pack_bytes;
};

WinPlan plan_window(int F, int R, int L) {
    WinPlan p{};
    if (F < 1 || F > 256 || R < 1 || R > 256 || L < 1 || L > kMaxLayers) return p;
    p.jt = pad_jt(R);
    p.nk0 = (F + 15) / 16;
    p.lds = p.jt <= 4;
    const long long one = pack_floats(p.jt, p.nk0, L) * 4;
    if (L == 1 || L * p.jt <= kMaxStateTiles) {
        p.mode = 1; p.nkd = p.jt; p.pack_bytes = one;
        // a pack beyond the LDS (32 < R <= 64, deep, wide input): the streamed twin; R <= 32 packs always fit
        if (p.lds && one > kLdsLimit) p.lds = false;
    } else {
        p.mode = 2; p.nkd = (R + 15) / 16;
        p.pack_bytes = (layer_floats(p.jt, p.nk0) + (L - 1) * layer_floats(p.jt, p.nkd)) * 4;
    }
    p.pack_bytes = (p.pack_bytes + 255) / 256 * 256;
    return p;
}

WinKernel resolve(int jt, int L, bool lds) {
    return jt <= 2 ? resolve_narrow(jt, L) : jt <= 4 ? (lds ? resolve_mid(jt, L) : resolve_mid_stream(jt, L)) : resolve_wide(jt, L);
}

int launch(WinKernel kern, const WinArgs& a, int layers, const WinPlan& p, hipStream_t s) {
    if (!kern) return sgp::fail(SGP_EUNSUP, "sgp_reservoir_window_f32: planned a kernel that is not built");
    const long long tiles = (a.M + 15) / 16;
    const long long lds = p.lds ? (layer_floats(p.jt, a.nk0) + (layers - 1) * layer_floats(p.jt, p.jt)) * 4 : 0;
    // four waves share one copy of the weights; small problems spread over more compute units instead
    const int waves = (tiles >= 1024 || lds > 64 * 1024) ? 4 : (tiles >= 512 ? 2 : 1);
    if (lds > 0) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return sgp::fail((int)e, "reservoir_window: LDS opt-in: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((tiles + waves - 1) / waves)), dim3(64 * waves), (size_t)lds, s, a);
    return sgp::check_launch("reservoir_window");
}
}  // namespace

extern "C" {

int32_t sgp_reservoir_window_supported(int32_t F, int32_t R, int32_t L) { return plan_window(F, R, L).mode; }

int64_t sgp_reservoir_window_workspace_bytes(int32_t F, int32_t R, int32_t L, int32_t S, int64_t M) {
    const WinPlan p = plan_window(F, R, L);
    if (!p.mode || S < 0 || M < 0) return -1;
    return p.pack_bytes + (p.mode == 2 ? ((int64_t)S * M * R * 4 + 255) / 256 * 256 : 0);
}

int sgp_reservoir_window_f32(const float* x, int64_t xbs, int64_t xss, int64_t xns, int32_t Fx,
                             const float* u, int64_t ubs, int64_t uss, int64_t uns, int32_t Fu,
                             const int32_t* step_start,
                             const float* const* w_ih, const float* const* w_hh, const float* const* b,
                             const double* alpha, int32_t act,
                             const float* h0, float* out, int64_t out_row_stride,
                             void* workspace, int32_t packed,
                             int32_t B, int32_t N, int32_t S, int32_t R, int32_t L, sgp_stream_t stream) {
    SGP_REQUIRE(x && out && workspace && alpha, "sgp_reservoir_window_f32: null pointer");
    SGP_REQUIRE(B >= 0 && N >= 0 && S >= 1 && Fx >= 1 && Fu >= 0, "sgp_reservoir_window_f32: bad size");
    SGP_REQUIRE((u != nullptr) == (Fu > 0), "sgp_reservoir_window_f32: u and its width go together");
    SGP_REQUIRE(act >= SGP_ACT_TANH && act <= SGP_ACT_TANH_REL, "sgp_reservoir_window_f32: unknown activation %d", act);
    SGP_REQUIRE(sgp::aligned16(workspace), "sgp_reservoir_window_f32: workspace must be 16-byte aligned");
    const int F = Fx + Fu;
    const WinPlan p = plan_window(F, R, L);
    if (!p.mode)
        return sgp::fail(SGP_EUNSUP, "sgp_reservoir_window_f32: built for Fx + Fu <= 256, R <= 256, L <= %d (got %d, %d, %d)",
                         kMaxLayers, F, R, L);
    SGP_REQUIRE(out_row_stride >= (int64_t)L * R, "sgp_reservoir_window_f32: out rows hold L * R values");
    SGP_REQUIRE(packed || (w_ih && w_hh && b), "sgp_reservoir_window_f32: null weight table");
    const long long M = (long long)B * N;
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    float* const ws = (float*)workspace;

    long long off[kMaxLayers];                            // floats from the start of the pack
    for (int l = 0, at = 0; l < L; ++l) {
        off[l] = at;
        at += (int)layer_floats(p.jt, l == 0 ? p.nk0 : p.nkd);
    }
    if (!packed) {
        for (int l = 0; l < L; ++l) {
            SGP_REQUIRE(w_ih[l] && w_hh[l] && b[l], "sgp_reservoir_window_f32: null weights of layer %d", l);
            const int nk = l == 0 ? p.nk0 : p.nkd;
            const long long blocks = (layer_floats(p.jt, nk) + 255) / 256;
            hipLaunchKernelGGL(pack_window_layer, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, s,
                               w_ih[l], w_hh[l], b[l], ws + off[l], l == 0 ? F : R, R, p.jt, nk);
        }
        int rc = sgp::check_launch("pack_window_layer");
        if (rc) return rc;
    }

    WinArgs a{};
    a.x = x; a.xbs = xbs; a.xss = xss; a.xns = xns; a.Fx = Fx;
    a.u = u; a.ubs = ubs; a.uss = uss; a.uns = uns; a.Fu = Fu;
    a.step_start = step_start;
    a.wp = ws;
    a.h0 = h0; a.h0_layer = M * R;
    a.out = out; a.ors = out_row_stride;
    a.act = act; a.S = S; a.N = N; a.R = R; a.nk0 = p.nk0; a.M = M;
    a.ovec = (R % 4 == 0 && out_row_stride % 4 == 0 && sgp::aligned16(out)) ? 1 : 0;
    for (int l = 0; l < L; ++l) {
        a.alpha[l] = (float)alpha[l];                      // rounded to fp32 as torch does for `(1 - alpha) * h`
        a.one_minus_alpha[l] = (float)(1.0 - alpha[l]);    // (reservoir.py:80)
    }
    if (p.mode == 1) return launch(resolve(p.jt, L, p.lds), a, L, p, s);

    // layer by layer: layer l leaves its sequence in `seq`, layer l + 1 reads a row and overwrites it with its own
    // (a sequence's rows belong to one wave, which has consumed a row before it stores to it); the last stores none
    float* const seq = ws + p.pack_bytes / 4;
    WinKernel kern = resolve(p.jt, 1, p.lds);
    for (int l = 0; l < L; ++l) {
        WinArgs m = a;
        if (l > 0) {
            m.x = seq; m.xbs = 0; m.xss = M * R; m.xns = R; m.Fx = R;
            m.u = nullptr; m.Fu = 0; m.step_start = nullptr;
            m.N = (int)(M < 0x7fffffff ? M : 0);
            m.nk0 = p.nkd;
        }
        if (l > 0 && M >= 0x7fffffff) return sgp::fail(SGP_EUNSUP, "sgp_reservoir_window_f32: too many sequences");
        m.wp = ws + off[l];
        m.h0 = h0 ? h0 + l * M * R : nullptr;
        m.out = out + (long long)l * R;
        m.ovec = a.ovec;
        m.alpha[0] = a.alpha[l]; m.one_minus_alpha[0] = a.one_minus_alpha[l];
        m.seq = l + 1 < L ? seq : nullptr;
        int rc = launch(kern, m, 1, p, s);
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
