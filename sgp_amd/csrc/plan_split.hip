// Host-side planner of sgp_spmm_split_f32 (kernel: spmm_split.hip; array formats: sgp_amd/splitplan.py, whose numpy
// planner this file restates -- tests/test_splitplan.py holds the two to the same bytes).  No device code: the
// functions below take HOST pointers and run on the caller's cores.
//
// Why native: the plan of the target graph (N = 100 000, 100-NN) cost 22 s of single-threaded numpy in front of an
// 80 ms encoder pass (round-5 review); the encoder is called once per experiment (reference: lib/utils.py:27-32), so
// its wall time is what a user sees.  Here: one O(nnz log) dealing pass + a per-tile fill on all cores.
#include "common.h"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

namespace {

// k-slots of the four 8-row sets a chunk's two transpose reads serve together (splitplan._SET_SLOTS)
constexpr int SET_SLOTS[4][8] = {{0, 1, 2, 3, 8, 9, 10, 11}, {4, 5, 6, 7, 12, 13, 14, 15},
                                 {16, 17, 18, 19, 24, 25, 26, 27}, {20, 21, 22, 23, 28, 29, 30, 31}};

inline uint16_t half_bits(_Float16 h) { uint16_t b; memcpy(&b, &h, 2); return b; }

// v (already scaled) -> hi + lo fp16 pieces: hi = v truncated to 10 explicit mantissa bits (rounded in the fp16
// subnormal range), lo = the rounded remainder (splitplan.split_fp16)
inline void split_fp16(float v, uint16_t& hi, uint16_t& lo) {
    uint32_t bits;
    memcpy(&bits, &v, 4);
    bits &= 0xFFFFE000u;
    float hi32;
    memcpy(&hi32, &bits, 4);
    if (fabsf(v) < 6.103515625e-05f) hi32 = (float)(_Float16)v;
    const _Float16 h = (_Float16)hi32;
    const _Float16 l = (_Float16)(v - (float)h);
    hi = half_bits(h);
    lo = half_bits(l);
}

// floor(log2(16384 / rmax)) clipped to [-126, 126] (exact: exponent extraction, not a rounded logarithm)
inline int row_exponent(float rmax) {
    if (!(rmax > 0.0f)) return 0;
    const float q = 16384.0f / rmax;
    int e;
    if (isinf(q)) e = 126;
    else { int ex; (void)frexpf(q, &ex); e = ex - 1; }
    return std::min(126, std::max(-126, e));
}

struct FillArgs {
    const int64_t* rowptr; const int64_t* col; const float* val;
    int64_t n_rows, n_cols;
    const int64_t* wave_of_row; const int64_t* slot_of_row; const int64_t* tile_of_wave; const int64_t* rows_of_wave;
    int64_t n_waves, n_tiles;
    int waves, chunks, max_union;
    int32_t* hdr; int32_t* rowid; int32_t* ucol; uint16_t* afr; int32_t* adr; float* rinv;
};

struct Scratch {
    std::vector<int32_t> stage_of_col, kpos_of_col;
    std::vector<int64_t> cols;
    std::vector<float> dense;
    explicit Scratch(const FillArgs& a) : stage_of_col(a.n_cols, -1), kpos_of_col(a.n_cols, -1), dense((size_t)a.chunks * 512) {}
};

// one tile: staged rows, per-wave k-slots (bank-aware), transpose-read addresses, A fragments.  Returns the number of
// (wave, column) keys, -1 on a plan that breaks the kernel's limits.
int64_t fill_tile(const FillArgs& a, int64_t t, const int64_t* first_wave, const int64_t* row_list, const int64_t* row_first,
                  Scratch& s, int64_t& union_out) {
    const int W = a.waves, C = a.chunks;
    const int64_t w0 = first_wave[t], w1 = first_wave[t + 1];
    // staged rows: the tile's sorted distinct columns
    s.cols.clear();
    for (int64_t w = w0; w < w1; ++w)
        for (int64_t i = row_first[w]; i < row_first[w + 1]; ++i) {
            const int64_t r = row_list[i];
            s.cols.insert(s.cols.end(), a.col + a.rowptr[r], a.col + a.rowptr[r + 1]);
        }
    std::sort(s.cols.begin(), s.cols.end());
    s.cols.erase(std::unique(s.cols.begin(), s.cols.end()), s.cols.end());
    if (s.cols.empty()) s.cols.push_back(0);                 // a tile of empty rows still stages one (finite) row: its padding reads
    const int64_t U = (int64_t)s.cols.size();
    if (U > a.max_union) return -1;
    union_out = U;
    std::vector<int64_t> tile_cols(s.cols);
    for (int64_t i = 0; i < U; ++i) {
        s.stage_of_col[tile_cols[i]] = (int32_t)i;
        a.ucol[t * a.max_union + i] = (int32_t)tile_cols[i];
    }
    a.hdr[t * 64 + 2 * W] = (int32_t)U;
    int64_t keys = 0;
    for (int64_t w = w0; w < w1; ++w) {
        const int win = (int)(w - w0);
        const int nrows = (int)a.rows_of_wave[w];
        a.hdr[t * 64 + W + win] = nrows;
        // the wave's sorted distinct columns; position p -> chunk p / 32
        s.cols.clear();
        for (int64_t i = row_first[w]; i < row_first[w + 1]; ++i) {
            const int64_t r = row_list[i];
            a.rowid[(t * W + win) * 16 + a.slot_of_row[r]] = (int32_t)r;
            s.cols.insert(s.cols.end(), a.col + a.rowptr[r], a.col + a.rowptr[r + 1]);
        }
        std::sort(s.cols.begin(), s.cols.end());
        s.cols.erase(std::unique(s.cols.begin(), s.cols.end()), s.cols.end());
        const int nk = (int)s.cols.size();
        if (nk > 32 * C) return -1;
        keys += nk;
        int32_t* adr = a.adr + ((t * W + win) * C) * 64;
        for (int c = 0; c < C; ++c) {
            // k-slots of the chunk: the j-th row of a bank residue (stage & 7) goes to set j, in residue order inside
            // the set; rows beyond four of a residue take the free slots in order
            int srow[32];
            for (int k = 0; k < 32; ++k) srow[k] = -1;
            const int k0 = 32 * c, k1 = std::min(nk, 32 * c + 32);
            int cnt_res[8] = {0, 0, 0, 0, 0, 0, 0, 0}, in_set[4] = {0, 0, 0, 0};
            int rank[32], slot[32];
            for (int k = k0; k < k1; ++k) rank[k - k0] = cnt_res[s.stage_of_col[s.cols[k]] & 7]++;
            // primaries: for rank r, keys in residue order (at most one per residue)
            for (int r = 0; r < 4; ++r)
                for (int res = 0; res < 8; ++res)
                    for (int k = k0; k < k1; ++k)
                        if (rank[k - k0] == r && (s.stage_of_col[s.cols[k]] & 7) == res) slot[k - k0] = SET_SLOTS[r][in_set[r]++];
            bool occ[32] = {};
            for (int k = k0; k < k1; ++k) if (rank[k - k0] < 4) occ[slot[k - k0]] = true;
            int free_at = 0;
            for (int res = 0; res < 8; ++res)               // extras in (residue, stage) order
                for (int k = k0; k < k1; ++k)
                    if (rank[k - k0] >= 4 && (s.stage_of_col[s.cols[k]] & 7) == res) {
                        while (occ[free_at]) ++free_at;
                        slot[k - k0] = free_at;
                        occ[free_at] = true;
                    }
            for (int k = k0; k < k1; ++k) {
                srow[slot[k - k0]] = s.stage_of_col[s.cols[k]];
                s.kpos_of_col[s.cols[k]] = 32 * c + slot[k - k0];
            }
            // padding slots repeat a row of their own set (same address = broadcast); an empty set reads staged row 0
            for (int q = 0; q < 4; ++q) {
                int rep = -1;
                for (int i = 0; i < 8; ++i) { const int v = srow[SET_SLOTS[q][i]]; if (v >= 0 && (rep < 0 || v < rep)) rep = v; }
                if (rep < 0) rep = 0;
                for (int i = 0; i < 8; ++i) if (srow[SET_SLOTS[q][i]] < 0) srow[SET_SLOTS[q][i]] = rep;
            }
            for (int g = 0; g < 4; ++g)
                for (int li = 0; li < 16; ++li) {
                    unsigned av[2];
                    for (int j = 0; j < 2; ++j) {
                        const int sl = srow[8 * g + 4 * j + (li >> 2)];
                        av[j] = (unsigned)((sl >> 3) * 512 + (sl & 7) * 32 + 8 * (li & 3));
                    }
                    if (av[0] >= 65536u || av[1] >= 65536u) return -1;
                    adr[c * 64 + 16 * g + li] = (int32_t)(av[0] | (av[1] << 16));
                }
        }
        // A fragments: duplicates added in fp32 in edge order, every row scaled by its own power of two, split
        std::fill(s.dense.begin(), s.dense.end(), 0.0f);
        for (int64_t i = row_first[w]; i < row_first[w + 1]; ++i) {
            const int64_t r = row_list[i];
            const int sl = (int)a.slot_of_row[r];
            for (int64_t e = a.rowptr[r]; e < a.rowptr[r + 1]; ++e) {
                const int pos = s.kpos_of_col[a.col[e]];
                const int k = pos & 31;
                s.dense[(size_t)(pos >> 5) * 512 + (sl + 16 * (k >> 3)) * 8 + (k & 7)] += a.val[e];
            }
        }
        uint16_t* afr = a.afr + ((size_t)(t * W + win) * C) * 2 * 512;
        for (int sl = 0; sl < 16; ++sl) {
            float rmax = 0.0f;
            for (int c = 0; c < C; ++c)
                for (int g = 0; g < 4; ++g)
                    for (int e = 0; e < 8; ++e) rmax = std::max(rmax, fabsf(s.dense[(size_t)c * 512 + (sl + 16 * g) * 8 + e]));
            const int er = row_exponent(rmax);
            const float scale = ldexpf(1.0f, er);
            for (int c = 0; c < C; ++c)
                for (int g = 0; g < 4; ++g)
                    for (int e = 0; e < 8; ++e) {
                        const size_t at = (size_t)(sl + 16 * g) * 8 + e;
                        uint16_t hi, lo;
                        split_fp16(s.dense[(size_t)c * 512 + at] * scale, hi, lo);
                        afr[((size_t)c * 2 + 0) * 512 + at] = hi;
                        afr[((size_t)c * 2 + 1) * 512 + at] = lo;
                    }
            a.rinv[(t * W + win) * 16 + sl] = sl < nrows ? ldexpf(1.0f, -er) : 0.0f;
        }
    }
    return keys;
}

// rowptr of a CSR with nnz stored entries: starts at 0, never decreases, ends within the arrays
const char* rowptr_fault(const int64_t* rowptr, int64_t n_rows, int64_t nnz) {
    if (nnz < 0) return "negative nnz";
    if (n_rows > 0 && rowptr[0] != 0) return "rowptr[0] != 0";
    for (int64_t r = 0; r < n_rows; ++r)
        if (rowptr[r + 1] < rowptr[r]) return "rowptr decreases";
    if (n_rows > 0 && rowptr[n_rows] > nnz) return "rowptr[n_rows] > nnz";
    return nullptr;
}

// the entries below are called through a C ABI: nothing may leave them as an exception (std::bad_alloc from the
// vectors, std::system_error from std::thread)
template <class R, class F> R guarded(const char* what, F&& body) {
    try { return body(); }
    catch (const std::bad_alloc&) { return (R)sgp::fail(SGP_ENOMEM, "%s: out of host memory", what); }
    catch (const std::exception& e) { return (R)sgp::fail(SGP_EINVAL, "%s: %s", what, e.what()); }
    catch (...) { return (R)sgp::fail(SGP_EINVAL, "%s: unknown exception", what); }
}

}  // namespace

extern "C" int64_t sgp_split_plan_deal(const int64_t* rowptr, const int64_t* col, int64_t nnz, int64_t n_rows, int64_t n_cols,
                                       const int64_t* order, int64_t n_order,
                                       int32_t waves, int32_t chunks, int32_t max_union, int32_t rows_per_wave,
                                       int64_t* wave_of_row, int64_t* slot_of_row, int64_t* tile_of_wave, int64_t* rows_of_wave) {
  return guarded<int64_t>("sgp_split_plan_deal", [&]() -> int64_t {
    if (!rowptr || (!col && nnz > 0) || !wave_of_row || !slot_of_row || !tile_of_wave || !rows_of_wave ||
        n_rows < 0 || n_cols < 0 || waves < 1 || chunks < 1 || max_union < 1 || rows_per_wave < 1 || (order && n_order < 0))
        return sgp::fail(SGP_EINVAL, "sgp_split_plan_deal: bad argument");
    if (const char* f = rowptr_fault(rowptr, n_rows, nnz)) return sgp::fail(SGP_EINVAL, "sgp_split_plan_deal: malformed CSR: %s", f);
    const int64_t cap = 32ll * chunks;
    std::vector<int64_t> wmark(n_cols, -1), tmark(n_cols, -1), c;
    for (int64_t r = 0; r < n_rows; ++r) wave_of_row[r] = slot_of_row[r] = -1;
    int64_t wave = -1, tile = -1, w_rows = 0, w_cols = 0, t_cols = 0, t_waves = 0;
    auto open_wave = [&](bool new_tile) {
        ++wave;
        if (new_tile) { ++tile; t_cols = t_waves = 0; }
        ++t_waves;
        w_rows = w_cols = 0;
        tile_of_wave[wave] = tile;
        rows_of_wave[wave] = 0;
    };
    const int64_t n_seq = order ? n_order : n_rows;
    for (int64_t i = 0; i < n_seq; ++i) {
        const int64_t r = order ? order[i] : i;
        if (r < 0 || r >= n_rows) return sgp::fail(SGP_EINVAL, "sgp_split_plan_deal: order entry out of range");
        if (wave_of_row[r] >= 0) return sgp::fail(SGP_EINVAL, "sgp_split_plan_deal: row %lld appears twice in the order", (long long)r);
        c.assign(col + rowptr[r], col + rowptr[r + 1]);
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        const int64_t nc = (int64_t)c.size();
        if (nc > cap || nc > max_union) return -2;             // a row beyond a wave's column budget: no single-pass plan
        if (nc && (c.front() < 0 || c.back() >= n_cols)) return sgp::fail(SGP_EINVAL, "sgp_split_plan_deal: column out of range");
        if (wave < 0) open_wave(true);
        int64_t new_w = 0, new_t = 0;
        for (int64_t v : c) { new_w += wmark[v] != wave; new_t += tmark[v] != tile; }
        const bool need_wave = w_rows == rows_per_wave || w_cols + new_w > cap;
        if (t_cols + new_t > max_union || (need_wave && t_waves == waves)) { open_wave(true); new_w = new_t = nc; }
        else if (need_wave) { open_wave(false); new_w = nc; }
        for (int64_t v : c) { wmark[v] = wave; tmark[v] = tile; }
        w_cols += new_w;
        t_cols += new_t;
        wave_of_row[r] = wave;
        slot_of_row[r] = w_rows;
        rows_of_wave[wave] = ++w_rows;
    }
    return wave + 1;
  });
}

namespace {

// The graph as the ordering pass sees it: the sorted DISTINCT columns of every row, and the rows of every column.
struct OrderGraph {
    std::vector<int64_t> rp, cp;           // rp[n_rows + 1] into rc, cp[n_cols + 1] into cr
    std::vector<int32_t> rc, cr;
    int32_t deg(int64_t r) const { return (int32_t)(rp[r + 1] - rp[r]); }
};

// 0, or the message of what is wrong with a column
const char* order_graph(const int64_t* rowptr, const int64_t* col, int64_t n_rows, int64_t n_cols, OrderGraph& g) {
    g.rp.assign(n_rows + 1, 0);
    g.rc.reserve((size_t)rowptr[n_rows]);
    std::vector<int64_t> c;
    for (int64_t r = 0; r < n_rows; ++r) {
        c.assign(col + rowptr[r], col + rowptr[r + 1]);
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        if (!c.empty() && (c.front() < 0 || c.back() >= n_cols)) return "column out of range";
        for (int64_t v : c) g.rc.push_back((int32_t)v);
        g.rp[r + 1] = (int64_t)g.rc.size();
    }
    g.cp.assign(n_cols + 1, 0);
    for (int32_t v : g.rc) ++g.cp[v + 1];
    for (int64_t v = 0; v < n_cols; ++v) g.cp[v + 1] += g.cp[v];
    g.cr.resize(g.rc.size());
    std::vector<int64_t> at(g.cp.begin(), g.cp.end() - 1);
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t e = g.rp[r]; e < g.rp[r + 1]; ++e) g.cr[at[g.rc[e]]++] = (int32_t)r;
    return nullptr;
}

// The greedy of sgp_split_plan_order.  One instance grows tiles (level 0: candidates come from a frontier bucketed by
// the number of new columns) and, inside a finished tile, waves (level 1: candidates are the tile's own rows).  Both
// keep, per row, the number of its columns already in the current union -- counted incrementally: a column that
// joins the union bumps the rows that hold it.
struct Orderer {
    const OrderGraph& g;
    const int64_t n_rows;
    const int32_t waves, wave_cols, max_union, rows_per_wave;
    std::vector<uint8_t> placed;
    std::vector<int32_t> t_mark, t_cnt, t_cnt_at, t_cand;         // tile level: stamps are tile numbers
    std::vector<int32_t> w_mark, w_cnt, w_cnt_at, in_tile;        // wave level: stamps are wave numbers
    std::vector<std::vector<int32_t>> bucket;                     // frontier rows by new-column count (lazily updated)
    std::vector<int32_t> rows, rest, wave_rows, wave_first;
    int32_t tile = -1, wave = -1, lo = 0;
    int64_t t_union = 0, w_union = 0, next_row = 0;

    Orderer(const OrderGraph& g_, int64_t n_rows_, int64_t n_cols, int32_t waves_, int32_t chunks, int32_t max_union_, int32_t rpw)
        : g(g_), n_rows(n_rows_), waves(waves_), wave_cols(32 * chunks), max_union(max_union_), rows_per_wave(rpw),
          placed(n_rows_, 0), t_mark(n_cols, -1), t_cnt(n_rows_, 0), t_cnt_at(n_rows_, -1), t_cand(n_rows_, -1),
          w_mark(n_cols, -1), w_cnt(n_rows_, 0), w_cnt_at(n_rows_, -1), in_tile(n_rows_, -1) {
        int32_t dmax = 0;
        for (int64_t r = 0; r < n_rows; ++r) dmax = std::max(dmax, g.deg(r));
        bucket.resize((size_t)dmax + 1);
    }
    int32_t t_have(int32_t r) const { return t_cnt_at[r] == tile ? t_cnt[r] : 0; }
    int32_t w_have(int32_t r) const { return w_cnt_at[r] == wave ? w_cnt[r] : 0; }
    void t_push(int32_t r) {
        const int32_t k = g.deg(r) - t_have(r);
        bucket[k].push_back(r);
        lo = std::min(lo, k);
    }
    void tile_take(int32_t r) {
        placed[r] = 1;
        rows.push_back(r);
        for (int64_t e = g.rp[r]; e < g.rp[r + 1]; ++e) {
            const int32_t c = g.rc[e];
            if (t_mark[c] == tile) continue;
            t_mark[c] = tile;
            ++t_union;
            for (int64_t i = g.cp[c]; i < g.cp[c + 1]; ++i) {
                const int32_t q = g.cr[i];
                if (placed[q]) continue;
                if (t_cnt_at[q] != tile) { t_cnt_at[q] = tile; t_cnt[q] = 0; }
                ++t_cnt[q];
                if (t_cand[q] == tile) t_push(q);
            }
            if (c < n_rows && !placed[c] && t_cand[c] != tile) { t_cand[c] = tile; t_push(c); }    // square: column c names row c
        }
    }
    // best frontier row: fewest new columns, then most columns in the union, then lowest number; -1: none
    int32_t tile_best() {
        for (; lo < (int32_t)bucket.size(); ++lo) {
            std::vector<int32_t>& b = bucket[lo];
            size_t keep = 0;
            int32_t best = -1;
            for (int32_t q : b) {
                if (placed[q] || t_cand[q] != tile || g.deg(q) - t_have(q) != lo) continue;       // stale entry
                b[keep++] = q;
                if (best < 0 || t_have(q) > t_have(best) || (t_have(q) == t_have(best) && q < best)) best = q;
            }
            b.resize(keep);
            if (best >= 0) return best;
        }
        return -1;
    }
    void grow_tile() {
        ++tile;
        rows.clear();
        t_union = 0;
        for (auto& b : bucket) b.clear();
        lo = (int32_t)bucket.size();
        while (placed[next_row]) ++next_row;
        tile_take((int32_t)next_row);                              // the seed, whatever its size
        const size_t cap_rows = (size_t)waves * rows_per_wave;
        while (rows.size() < cap_rows) {
            int32_t r = tile_best();
            if (r < 0) {                                           // nothing on the frontier: the numbering's next row
                while (next_row < n_rows && placed[next_row]) ++next_row;
                if (next_row == n_rows) break;
                r = (int32_t)next_row;
            }
            if (t_union + g.deg(r) - t_have(r) > max_union) break;
            tile_take(r);
        }
    }
    void wave_take(int32_t r) {
        in_tile[r] = -1;
        wave_rows.push_back(r);
        for (int64_t e = g.rp[r]; e < g.rp[r + 1]; ++e) {
            const int32_t c = g.rc[e];
            if (w_mark[c] == wave) continue;
            w_mark[c] = wave;
            ++w_union;
            for (int64_t i = g.cp[c]; i < g.cp[c + 1]; ++i) {
                const int32_t q = g.cr[i];
                if (in_tile[q] != tile) continue;
                if (w_cnt_at[q] != wave) { w_cnt_at[q] = wave; w_cnt[q] = 0; }
                ++w_cnt[q];
            }
        }
    }
    // cuts rows[] into waves (wave_rows / wave_first); returns their number
    int32_t cut_waves() {
        rest.assign(rows.begin(), rows.end());
        std::sort(rest.begin(), rest.end());
        for (int32_t r : rest) in_tile[r] = tile;
        wave_rows.clear();
        wave_first.assign(1, 0);
        while (!rest.empty()) {
            ++wave;
            w_union = 0;
            int32_t n_in = 0;
            size_t at = 0;                                         // the seed: the lowest-numbered row left
            for (;;) {
                const int32_t r = rest[at];
                rest.erase(rest.begin() + (int64_t)at);
                wave_take(r);
                if (++n_in == rows_per_wave || rest.empty()) break;
                at = 0;
                for (size_t i = 1; i < rest.size(); ++i) {         // (rest is sorted: the first of equals has the lowest number)
                    const int32_t q = rest[i], b = rest[at];
                    const int32_t nq = g.deg(q) - w_have(q), nb = g.deg(b) - w_have(b);
                    if (nq < nb || (nq == nb && w_have(q) > w_have(b))) at = i;
                }
                if (w_union + g.deg(rest[at]) - w_have(rest[at]) > wave_cols) break;
            }
            wave_first.push_back((int32_t)wave_rows.size());
        }
        return (int32_t)wave_first.size() - 1;
    }
    void run(int64_t* order) {
        int64_t n_out = 0;
        while (n_out < n_rows) {
            grow_tile();
            const int32_t n_waves = cut_waves();
            const int32_t kept = std::min(n_waves, waves);
            for (int32_t i = 0; i < wave_first[kept]; ++i) order[n_out++] = wave_rows[i];
            for (int32_t i = wave_first[kept]; i < wave_first[n_waves]; ++i) {     // waves beyond the tile's: unplaced again
                placed[wave_rows[i]] = 0;
                next_row = std::min<int64_t>(next_row, wave_rows[i]);
            }
        }
    }
};

}  // namespace

extern "C" int sgp_split_plan_order(const int64_t* rowptr, const int64_t* col, int64_t nnz, int64_t n_rows, int64_t n_cols,
                                    int32_t waves, int32_t chunks, int32_t max_union, int32_t rows_per_wave, int64_t* order) {
  return guarded<int>("sgp_split_plan_order", [&]() -> int {
    SGP_REQUIRE(rowptr && (col || nnz <= 0) && order, "sgp_split_plan_order: null pointer");
    SGP_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_rows < (1ll << 31) - 1 && n_cols < (1ll << 31) - 1 && waves >= 1 && chunks >= 1 &&
                chunks <= (1 << 24) && max_union >= 1 && rows_per_wave >= 1 && (int64_t)waves * rows_per_wave < (1ll << 31),
                "sgp_split_plan_order: bad size");
    if (const char* f = rowptr_fault(rowptr, n_rows, nnz)) return sgp::fail(SGP_EINVAL, "sgp_split_plan_order: malformed CSR: %s", f);
    if (n_rows == 0) return 0;
    OrderGraph g;
    if (const char* f = order_graph(rowptr, col, n_rows, n_cols, g)) return sgp::fail(SGP_EINVAL, "sgp_split_plan_order: %s", f);
    Orderer(g, n_rows, n_cols, waves, chunks, max_union, rows_per_wave).run(order);
    return 0;
  });
}

extern "C" int sgp_split_plan_fill(const int64_t* rowptr, const int64_t* col, const float* val, int64_t nnz, int64_t n_rows, int64_t n_cols,
                                   const int64_t* wave_of_row, const int64_t* slot_of_row, const int64_t* tile_of_wave,
                                   const int64_t* rows_of_wave, int64_t n_waves, int64_t n_tiles,
                                   int32_t waves, int32_t chunks, int32_t max_union,
                                   int32_t* hdr, int32_t* rowid, int32_t* ucol, void* afr, int32_t* adr, float* rinv,
                                   double* stats, int32_t threads) {
  return guarded<int>("sgp_split_plan_fill", [&]() -> int {
    SGP_REQUIRE(rowptr && col && val && wave_of_row && slot_of_row && tile_of_wave && rows_of_wave && hdr && rowid && ucol &&
                afr && adr && rinv && stats, "sgp_split_plan_fill: null pointer");
    SGP_REQUIRE(n_rows > 0 && n_cols > 0 && n_waves > 0 && n_tiles > 0 && waves >= 1 && 2 * waves < 64 && chunks >= 1 &&
                max_union >= 1 && max_union <= 65536 / 64 * 8, "sgp_split_plan_fill: bad size");
    if (const char* f = rowptr_fault(rowptr, n_rows, nnz)) return sgp::fail(SGP_EINVAL, "sgp_split_plan_fill: malformed CSR: %s", f);
    for (int64_t e = 0; e < rowptr[n_rows]; ++e)
        SGP_REQUIRE(col[e] >= 0 && col[e] < n_cols, "sgp_split_plan_fill: column out of range");
    FillArgs a{rowptr, col, val, n_rows, n_cols, wave_of_row, slot_of_row, tile_of_wave, rows_of_wave, n_waves, n_tiles,
               waves, chunks, max_union, hdr, rowid, ucol, (uint16_t*)afr, adr, rinv};
    memset(hdr, 0, sizeof(int32_t) * 64 * n_tiles);
    std::fill(rowid, rowid + n_tiles * waves * 16, -1);
    std::fill(ucol, ucol + n_tiles * (int64_t)max_union, -1);
    memset(afr, 0, sizeof(uint16_t) * (size_t)n_tiles * waves * chunks * 2 * 512);
    memset(adr, 0, sizeof(int32_t) * (size_t)n_tiles * waves * chunks * 64);
    memset(rinv, 0, sizeof(float) * (size_t)n_tiles * waves * 16);
    // waves of every tile (contiguous), rows of every wave in slot order
    std::vector<int64_t> first_wave(n_tiles + 1, 0), row_first(n_waves + 1, 0);
    for (int64_t w = 0; w < n_waves; ++w) {
        const int64_t t = tile_of_wave[w];
        SGP_REQUIRE(t >= 0 && t < n_tiles && (w == 0 || t == tile_of_wave[w - 1] || t == tile_of_wave[w - 1] + 1),
                    "sgp_split_plan_fill: tile_of_wave is not a non-decreasing run");
        SGP_REQUIRE(rows_of_wave[w] >= 0 && rows_of_wave[w] <= 16, "sgp_split_plan_fill: a wave holds at most 16 rows");
        ++first_wave[t + 1];
        row_first[w + 1] = row_first[w] + rows_of_wave[w];
    }
    for (int64_t t = 0; t < n_tiles; ++t) {
        SGP_REQUIRE(first_wave[t + 1] >= 1 && first_wave[t + 1] <= waves, "sgp_split_plan_fill: a tile holds 1 .. waves waves");
        first_wave[t + 1] += first_wave[t];
    }
    const int64_t n_dealt = row_first[n_waves];
    std::vector<int64_t> row_list(std::max<int64_t>(n_dealt, 1), -1);
    int64_t seen = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t w = wave_of_row[r];
        if (w < 0) continue;
        SGP_REQUIRE(w < n_waves && slot_of_row[r] >= 0 && slot_of_row[r] < rows_of_wave[w] && row_list[row_first[w] + slot_of_row[r]] < 0,
                    "sgp_split_plan_fill: wave / slot of row %lld inconsistent", (long long)r);
        row_list[row_first[w] + slot_of_row[r]] = r;
        ++seen;
    }
    SGP_REQUIRE(seen == n_dealt, "sgp_split_plan_fill: rows_of_wave does not match wave_of_row");

    int nthr = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    nthr = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(nthr, 64), n_tiles));
    // every thread's scratch takes 8 bytes per column: at most 1 GiB of it in all
    nthr = (int)std::max<int64_t>(1, std::min<int64_t>(nthr, (1ll << 30) / (8 * n_cols)));
    std::atomic<int64_t> next(0), keys(0), usum(0), umax(0);
    std::atomic<int> bad(0);                               // 1: the deal breaks the kernel's limits, 2: out of memory
    auto work = [&]() {
        try {
            Scratch s(a);
            int64_t k_local = 0, u_local = 0, u_max = 0;
            for (;;) {
                const int64_t t = next.fetch_add(1);
                if (t >= n_tiles || bad.load()) break;
                int64_t U = 0;
                const int64_t k = fill_tile(a, t, first_wave.data(), row_list.data(), row_first.data(), s, U);
                if (k < 0) { bad.store(1); break; }
                k_local += k; u_local += U; u_max = std::max(u_max, U);
            }
            keys += k_local; usum += u_local;
            int64_t cur = umax.load();
            while (u_max > cur && !umax.compare_exchange_weak(cur, u_max)) {}
        } catch (...) { bad.store(2); }                    // (a thread's exception must not leave the thread)
    };
    if (nthr == 1) work();
    else {
        std::vector<std::thread> pool;
        pool.reserve(nthr);
        try {
            for (int i = 0; i < nthr; ++i) pool.emplace_back(work);
        } catch (const std::system_error&) {               // no more threads to be had: the ones started do the work
            if (pool.empty()) work();
        }
        for (auto& th : pool) th.join();
    }
    if (bad.load() == 2) return sgp::fail(SGP_ENOMEM, "sgp_split_plan_fill: out of host memory");
    if (bad.load()) return sgp::fail(SGP_EUNSUP, "sgp_split_plan_fill: the dealt rows break the kernel's limits");
    double norm_inf = 0.0;
    for (int64_t r = 0; r < n_rows; ++r) {
        double sum = 0.0;
        for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) sum += fabs((double)val[e]);
        norm_inf = std::max(norm_inf, sum);
    }
    const double dealt = (double)std::max<int64_t>(1, n_dealt);
    stats[0] = (double)n_tiles; stats[1] = (double)n_waves; stats[2] = (double)n_dealt / (double)n_waves;
    stats[3] = dealt / (double)n_tiles; stats[4] = (double)usum.load() / dealt;
    stats[5] = (double)keys.load() / ((double)n_waves * chunks * 32); stats[6] = (double)umax.load(); stats[7] = norm_inf;
    return 0;
  });
}

extern "C" int64_t sgp_split_plan_bands(const int32_t* ucol, int64_t n_tiles, int32_t max_union, int64_t n_cols,
                                        int64_t col_budget, int32_t* band_first) {
  return guarded<int64_t>("sgp_split_plan_bands", [&]() -> int64_t {
    if (!ucol || !band_first || n_tiles < 1 || n_tiles >= (1ll << 31) || max_union < 1 || n_cols < 1 || col_budget < 1)
        return sgp::fail(SGP_EINVAL, "sgp_split_plan_bands: bad argument");
    // the deal's bookkeeping one level up: mark[c] = band that last staged column c
    std::vector<int64_t> mark(n_cols, -1);
    int64_t band = 0, b_cols = 0;
    band_first[0] = 0;
    for (int64_t t = 0; t < n_tiles; ++t) {
        const int32_t* u = ucol + t * max_union;
        int64_t fresh = 0, U = 0;
        for (; U < max_union && u[U] >= 0; ++U) {
            if (u[U] >= n_cols) return sgp::fail(SGP_EINVAL, "sgp_split_plan_bands: column out of range");
            fresh += mark[u[U]] != band;
        }
        if (t > band_first[band] && b_cols + fresh > col_budget) {      // (a tile beyond the budget on its own: a band of one)
            band_first[++band] = (int32_t)t;
            b_cols = 0;
            fresh = U;
        }
        for (int64_t i = 0; i < U; ++i) mark[u[i]] = band;
        b_cols += fresh;
    }
    band_first[band + 1] = (int32_t)n_tiles;
    return band + 1;
  });
}
