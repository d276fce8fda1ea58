// Stand-alone driver of the hop entries' operand checks for the host-ASan build (no Python, no preload):
//   make -C sgp_amd/csrc -f Makefile.asan
//   hipcc -Xarch_host -fsanitize=address -Iinclude tools/hop_operands_asan.cpp -Lsgp_amd/csrc/build_asan -lsgp_amd_asan \
//         -Wl,-rpath,$PWD/sgp_amd/csrc/build_asan -o /tmp/hop_operands_asan && /tmp/hop_operands_asan
// Every one of the nine entries gets every class of bad operand block of tests/test_hop_operands.py (same plan scalars:
// an accepted block is refused by the entry afterwards, nothing is launched); prints the codes, exits 0 when each bad
// block was refused with a message that names its entry.
#include <stdio.h>
#include <string.h>
#include "sgp_amd.h"

struct Block {
    const float* X; int64_t xrs, xbs; const float* Xh; int64_t xhrs, xhbs; int32_t n_own;
    float* Y; int64_t yrs, ybs; int32_t n_rows, n_cols, batch, feat;
};
#define BLOCK(o) o.X, o.xrs, o.xbs, o.Xh, o.xhrs, o.xhbs, o.n_own, o.Y, o.yrs, o.ybs, o.n_rows, o.n_cols, o.batch, o.feat

alignas(64) static float mem[256];
static const int32_t* const P = reinterpret_cast<const int32_t*>(mem + 192);     // every plan array: never read

static int call(int e, const Block& o) {
    const float* F = reinterpret_cast<const float*>(P);
    switch (e) {
        case 0: return sgp_spmm_csr_f32(P, P, F, BLOCK(o), nullptr, 0, nullptr);
        case 1: return sgp_spmm_tiled_f32(P, P, P, P, reinterpret_cast<const uint16_t*>(P), F,
                                          sgp_spmm_tiled_max_tile_rows() / 6 + 1, 8, 0, 64, BLOCK(o), nullptr, 0, nullptr);
        case 2: return sgp_spmm_res_f32(P, P, P, P, P, P, F, P, 0, 0, 0, BLOCK(o), nullptr, 0, nullptr);
        case 3: return sgp_spmm_mix_f32(P, P, P, P, P, P, F, P, P, P, F, 0, 0, 0, BLOCK(o), nullptr, 0, nullptr);
        case 4: return sgp_spmm_colblock_f32(P, P, P, 1, 1, BLOCK(o), nullptr, 0, nullptr);
        case 5: return sgp_spmm_split_f32(P, P, P, P, P, F, 1 << 28, BLOCK(o), F, 0, 8, nullptr, 0, nullptr);
        case 6: return sgp_spmm_split_wide_f32(P, P, P, P, P, F, 1 << 28, BLOCK(o), F, 0, 8, nullptr, 0, nullptr);
        case 7: return sgp_spmm_split_banded_f32(P, P, P, P, P, F, 1 << 28, BLOCK(o), F, 0, 8, 0, nullptr, 0, nullptr, 0, nullptr);
        default: return sgp_spmm_split_wide_banded_f32(P, P, P, P, P, F, 1 << 28, BLOCK(o), F, 0, 8, 0, nullptr, 0, nullptr, 0, nullptr);
    }
}

int main() {
    static const char* const names[9] = {"sgp_spmm_csr_f32", "sgp_spmm_tiled_f32", "sgp_spmm_res_f32", "sgp_spmm_mix_f32",
                                         "sgp_spmm_colblock_f32", "sgp_spmm_split_f32", "sgp_spmm_split_wide_f32",
                                         "sgp_spmm_split_banded_f32", "sgp_spmm_split_wide_banded_f32"};
    static const int64_t own_limit[9] = {0, 1ll << 31, 1ll << 30, 1ll << 30, 1ll << 40, 1ll << 29, 1ll << 29, 1ll << 29, 1ll << 29};
    int bad = 0;
    for (int e = 0; e < 9; ++e) {
        Block b{mem, 64, 4096, nullptr, 0, 0, 0, mem + 64, 64, 4096, 8, 8, 1, 64};
        if (e == 0) { b.n_own = 8; b.batch = 4 * 65535 + 1; }
        if (e == 4) b.feat = 64 * 65536;
        Block h = b; h.Xh = mem + 128; h.xhrs = 64; h.xhbs = 4096; h.n_own = 4;
        struct { const char* what; Block o; } cases[9] = {
            {"null_x", b}, {"null_y", b}, {"negative_batch", b}, {"n_own_beyond_cols", h}, {"row_stride_not_x4", b},
            {"base_not_aligned", b}, {"halo_stride_not_x4", h}, {"own_offset_at_limit", b}, {"feat_not_admissible", b}};
        cases[0].o.X = nullptr; cases[1].o.Y = nullptr; cases[2].o.batch = -1; cases[3].o.n_own = 9; cases[4].o.xrs = 66;
        cases[5].o.X = mem + 1; cases[6].o.xhrs = 65; cases[7].o.n_cols = 1 << 20; cases[7].o.xrs = own_limit[e] >> 20;
        cases[8].o.feat = e >= 5 ? 24 : 32;
        for (int c = 0; c < (e == 0 ? 4 : 9); ++c) {            // (csr: 64-bit addressing, a scalar kernel: the first four only)
            const int rc = call(e, cases[c].o);
            const bool named = strstr(sgp_last_error(), names[e]) == sgp_last_error();
            printf("%-32s %-20s %3d %s\n", names[e], cases[c].what, rc, sgp_last_error());
            if (rc >= 0 || !named) ++bad;
        }
    }
    printf("%d bad operand blocks were not refused by name\n", bad);
    return bad != 0;
}
