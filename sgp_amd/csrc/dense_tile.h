// The stage loop of the dense kernels: sgp_dense_f32 (decoder_mlp.hip), the DCRNN gates / update steps (dcrnn.hip) and
// the Graph WaveNet temporal convolution (gwnet.hip) are this loop with their own row loader, column-tile map and
// epilogue.  v_mfma_f32_16x16x4_f32 (exact fp32 products); a workgroup = 4 waves x RT row tiles of 16 rows x DT_TILES
// packed column tiles; the weight slab of a 64-wide k chunk is staged in LDS once and serves all the workgroup's rows.
//
// Why a kernel built on it computes the same bits whatever its launch form: every output element is ONE accumulator
// fed by one fmaf chain in k order -- kb ascending, s = 0 .. 3 inside a k block -- starting from zero; the stage
// depth, the tile a column lands in and the rows that share a workgroup change nothing in that chain.  What the loop
// itself must keep:
//   - two __syncthreads() per stage (the previous stage fully consumed, this one fully staged), the row pieces loaded
//     before the first so that they are in flight across it;
//   - the break at kb0 + u >= KB is wave-uniform, and a k block or column tile past the end is staged as zeros;
//   - rows past the end stay in the loop with zero row pieces, because they take part in the barriers: they leave
//     in the caller's epilogue only.
#pragma once
#include "common.h"

namespace sgp_dense {
using sgp::f32x4;

// The packed M[N, K] (wp below) is in the fragment order of frag.h: sgp_dense_pack_f32, sgp::frag_floats(N, K) floats.

constexpr int DT_KCH = 4;                          // k blocks of 16 per LDS stage
constexpr int DT_TILES = 4;                        // packed 16-column tiles per workgroup
constexpr int DT_LDS = DT_TILES * DT_KCH * 64;     // f32x4 elements of the caller's __shared__ slab: 16 KB

// acc[t][c] = sum over k of Mp[tile_of(c)] . (row tile t), for a workgroup of 256 threads.
//   load_x(t, kb)  the lane's 16-byte piece (columns 16 kb + 4 (lane >> 4) ..) of its row of row tile t; zeros past the
//                  end of the row and for a row that does not exist
//   tile_of(c)     packed column tile of LDS tile c, negative: a zero tile
// The packed weight holds fewer than 2^31 tiles of 1 KB (the callers' domain checks), so a tile's index is an int: as a
// 64-bit product it cost every kernel two VGPRs (profiles/dense_tile/).
// D[col, row]: lane (q, b), register r of acc[t][c] -> column 4 q + r of tile_of(c), row b of row tile t.
template <int RT, class LoadX, class TileOf>
__device__ __forceinline__ void dense_tile_loop(f32x4* wl, const float* wp, int KB, LoadX load_x, TileOf tile_of,
                                                f32x4 (&acc)[RT][DT_TILES]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int c = 0; c < DT_TILES; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb0 = 0; kb0 < KB; kb0 += DT_KCH) {
        f32x4 xv[RT][DT_KCH];                                        // row pieces first: in flight across the barrier
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int u = 0; u < DT_KCH; ++u) xv[t][u] = load_x(t, kb0 + u);
        __syncthreads();                                             // previous stage fully consumed
        for (int i = threadIdx.x; i < DT_LDS; i += 256) {
            const int l = i & 63, u = (i >> 6) % DT_KCH, c = i / (64 * DT_KCH);
            const int jt = tile_of(c);
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (jt >= 0 && kb0 + u < KB)
                v = *reinterpret_cast<const f32x4*>(wp + ((long long)(jt * KB + kb0 + u) * 64 + l) * 4);
            wl[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < DT_KCH; ++u) {
            if (kb0 + u >= KB) break;                                // wave-uniform
#pragma unroll
            for (int c = 0; c < DT_TILES; ++c) {
                const f32x4 wf = wl[(c * DT_KCH + u) * 64 + lane];
#pragma unroll
                for (int t = 0; t < RT; ++t)
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s], xv[t][u][s], acc[t][c], 0, 0, 0);
            }
        }
    }
}

}  // namespace sgp_dense
