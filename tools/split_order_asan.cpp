// Stand-alone driver of the split hop's row-ordering pass and deal for a host sanitizer build (no Python, no preload,
// no GPU: the planner is host code):
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/split_order_asan.cpp sgp_amd/csrc/plan_split.hip -o /tmp/split_order_asan && /tmp/split_order_asan
// Builds ring lattices (every node joined to its k nearest on a ring, numbering plain and shuffled, one with an
// isolated row and an over-long row) in memory, orders them, deals both orders and checks: the order is a permutation,
// two calls agree, every wave and tile of the deal keeps the three caps, malformed CSRs are refused.  Exits 0 when all
// hold.  (sgp::fail lives in api.hip with the device code; the few lines below stand in for it.)
#include <stdarg.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <set>
#include <vector>
#include "../include/sgp_amd.h"

static char g_err[512];
namespace sgp {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace sgp

struct Csr { int64_t n; std::vector<int64_t> rowptr, col; };

static Csr ring(int64_t n, int k, bool shuffle, bool odd_rows) {
    std::vector<int64_t> name(n);
    for (int64_t i = 0; i < n; ++i) name[i] = i;
    if (shuffle) {
        uint64_t s = 12345;
        for (int64_t i = n - 1; i > 0; --i) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(name[i], name[(int64_t)((s >> 33) % (uint64_t)(i + 1))]);
        }
    }
    std::vector<std::vector<int64_t>> rows(n);
    for (int64_t i = 0; i < n; ++i)
        for (int d = 1; d <= k / 2; ++d) {
            rows[name[i]].push_back(name[(i + d) % n]);
            rows[name[i]].push_back(name[(i + n - d) % n]);
        }
    if (odd_rows) {
        rows[5].clear();                                           // isolated (as a row)
        rows[9].clear();
        for (int64_t c = 0; c < 300 && c < n; ++c) rows[9].push_back((c * 7) % n);   // beyond 224 columns
    }
    Csr g{n, {0}, {}};
    for (auto& r : rows) { g.col.insert(g.col.end(), r.begin(), r.end()); g.rowptr.push_back((int64_t)g.col.size()); }
    return g;
}

static int check(const char* what, const Csr& g, int waves, int chunks, int max_union, int rpw) {
    const int64_t n = g.n, nnz = (int64_t)g.col.size();
    std::vector<int64_t> o1(n, -1), o2(n, -2);
    if (sgp_split_plan_order(g.rowptr.data(), g.col.data(), nnz, n, n, waves, chunks, max_union, rpw, o1.data()) != 0 ||
        sgp_split_plan_order(g.rowptr.data(), g.col.data(), nnz, n, n, waves, chunks, max_union, rpw, o2.data()) != 0) {
        printf("%s: order failed: %s\n", what, g_err);
        return 1;
    }
    std::vector<int64_t> sorted(o1);
    std::sort(sorted.begin(), sorted.end());
    for (int64_t i = 0; i < n; ++i) if (sorted[i] != i) { printf("%s: not a permutation\n", what); return 1; }
    if (o1 != o2) { printf("%s: two calls differ\n", what); return 1; }
    int64_t tiles[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int64_t> wave_of_row(n), slot_of_row(n), tile_of_wave(n), rows_of_wave(n);
        const int64_t nw = sgp_split_plan_deal(g.rowptr.data(), g.col.data(), nnz, n, n, pass ? o1.data() : nullptr, pass ? n : 0,
                                               waves, chunks, max_union, rpw, wave_of_row.data(), slot_of_row.data(),
                                               tile_of_wave.data(), rows_of_wave.data());
        if (nw == -2) { tiles[pass] = -2; continue; }
        if (nw <= 0) { printf("%s: deal failed: %s\n", what, g_err); return 1; }
        tiles[pass] = tile_of_wave[nw - 1] + 1;
        std::vector<std::set<int64_t>> wcols(nw), tcols(tiles[pass]);
        std::vector<int64_t> wpt(tiles[pass], 0);
        for (int64_t w = 0; w < nw; ++w) ++wpt[tile_of_wave[w]];
        for (int64_t r = 0; r < n; ++r)
            for (int64_t e = g.rowptr[r]; e < g.rowptr[r + 1]; ++e) {
                wcols[wave_of_row[r]].insert(g.col[e]);
                tcols[tile_of_wave[wave_of_row[r]]].insert(g.col[e]);
            }
        for (int64_t w = 0; w < nw; ++w)
            if (rows_of_wave[w] > rpw || (int64_t)wcols[w].size() > 32 * chunks) { printf("%s: wave %lld over a cap\n", what, (long long)w); return 1; }
        for (int64_t t = 0; t < tiles[pass]; ++t)
            if (wpt[t] > waves || (int64_t)tcols[t].size() > max_union) { printf("%s: tile %lld over a cap\n", what, (long long)t); return 1; }
    }
    printf("%-28s n = %6lld  tiles in numbering order %lld, in the new order %lld\n", what, (long long)n, (long long)tiles[0], (long long)tiles[1]);
    return 0;
}

int main() {
    int bad = 0;
    bad += check("ring 40", ring(5000, 40, false, false), 16, 7, 768, 16);
    bad += check("ring 40 shuffled", ring(3000, 40, true, false), 16, 7, 768, 16);
    bad += check("ring 20 odd rows", ring(700, 20, false, true), 16, 7, 768, 16);
    bad += check("ring 20 odd rows, wide", ring(700, 20, true, true), 8, 14, 768, 16);
    bad += check("ring 6 tiny caps", ring(200, 6, true, false), 2, 1, 40, 4);
    // malformed CSRs: refused with a code, nothing read out of bounds
    Csr g = ring(64, 6, false, false);
    std::vector<int64_t> o(64);
    const int64_t nnz = (int64_t)g.col.size();
    Csr dec = g; dec.rowptr[10] = dec.rowptr[11] + 3;
    Csr off = g; off.rowptr[0] = 1;
    Csr far = g; far.rowptr[64] = nnz + 5;
    Csr oob = g; oob.col[7] = 64;
    for (const Csr* c : {&dec, &off, &far, &oob}) {
        const int rc = sgp_split_plan_order(c->rowptr.data(), c->col.data(), nnz, 64, 64, 16, 7, 768, 16, o.data());
        printf("malformed: %d %s\n", rc, g_err);
        bad += rc >= 0;
    }
    bad += sgp_split_plan_order(nullptr, g.col.data(), nnz, 64, 64, 16, 7, 768, 16, o.data()) >= 0;
    bad += sgp_split_plan_order(g.rowptr.data(), g.col.data(), nnz, 64, 64, 0, 7, 768, 16, o.data()) >= 0;
    printf("%d checks failed\n", bad);
    return bad != 0;
}
