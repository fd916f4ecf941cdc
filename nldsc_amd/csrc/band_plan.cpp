// band_plan.cpp — host-side window replay and band schedule of the engine (no HIP: also built with
// g++ -fsanitize=address,undefined for the CPU sanitizer run, tests/native/plan_tsv_check.cpp).
#include "band_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/nldsc_ld.h"

namespace nldsc {

// Replay of ChunkwiseReader's pointers (stream.h:131-155,182-197) from positions and MAF-pass
// flags.  For every SNP j the reference computes, N(j) = { i in [L_j, R_j] : pass_i,
// |pos_i - pos_j| <= w, i != j }; L_j = -1 marks a SNP it does not compute (unused, MAF-failed).
void replay_windows(const double* pos, const uint8_t* flags, int n, double w, int* L, int* R) {
    auto used = [&](int i) { return 0 <= i && i < n && pos[i] >= 0; };
    auto inwin = [&](int a, int b) { return used(a) && used(b) && std::fabs(pos[b] - pos[a]) <= w; };
    int left = 0, right = -1;
    for (int j = 0; j < n; ++j) {
        L[j] = -1;
        R[j] = -2;
        if (!used(j)) continue;                       // pass_chunk
        do {                                          // extend_cache
            if (right + 1 >= n) break;
            ++right;
        } while (inwin(j, right));
        if (!(j <= right && (flags[j] & 1))) continue;  // initialize_next_chunk() == false
        // chunk_indices: evict failing SNPs at the left edge
        while (left < j && !((flags[left] & 1) && inwin(j, left))) ++left;
        L[j] = left;
        R[j] = right;
    }
}

// Positions non-decreasing over the used SNPs (pos >= 0)?
// every position >= 0 (no NaN) and non-decreasing: one branch-free pass (the GPU schedule's condition)
bool positions_nonneg_sorted(const double* pos, int M) {
    int bad = M > 0 && !(pos[0] >= 0.0);
    for (int j = 1; j < M; ++j) bad |= !(pos[j] >= 0.0) | (pos[j] < pos[j - 1]);
    return !bad;
}

bool positions_sorted(const double* pos, int M) {
    double last = -1.0;
    for (int j = 0; j < M; ++j)
        if (pos[j] >= 0) {
            if (pos[j] < last) return false;
            last = pos[j];
        }
    return true;
}

// Tile schedule of the band kernel.  A block pair (I <= J) is needed when it holds a pair (i < j)
// with j in N(i) or i in N(j) and one of i, j is owned.  Rows need columns up to the last
// in-window neighbour: R_i is the reference's (loose) cache bound — its extend_cache advances at
// least one SNP per SNP, so R_i drifts past the window — so for sorted positions the bound is
// tightened to the last index with pos <= pos_i + w (the kernel still masks with the exact
// predicate).  Columns j need rows down to L_j (exact).
void plan_items(const double* pos, const uint8_t* flags, int M, double w, const int* L, const int* R, int own_begin,
                int own_end, int max_nc, std::vector<PlanItem>& out) {
    constexpr int B = 32;
    const int nblk = (M + B - 1) / B;
    std::vector<int> blk_pass(nblk, 0), blk_own(nblk, 0);
    for (int j = 0; j < M; ++j) {
        if (flags[j] & 1) blk_pass[j / B] = 1;
        if (j >= own_begin && j < own_end) blk_own[j / B] = 1;
    }
    // sorted (non-decreasing over used SNPs)?  then the window's right edge is a binary search
    std::vector<int> used_idx;
    used_idx.reserve(M);
    bool sorted = true;
    for (int j = 0; j < M; ++j)
        if (pos[j] >= 0) {
            if (!used_idx.empty() && pos[j] < pos[used_idx.back()]) sorted = false;
            used_idx.push_back(j);
        }
    // sorted: last used index with pos <= pos_i + w (ties inclusive, tools.h:41-49) by a two-pointer sweep
    std::vector<int> hi_of;
    if (sorted) {
        hi_of.assign(M, -1);
        size_t k = 0;
        for (size_t u = 0; u < used_idx.size(); ++u) {
            const double lim = pos[used_idx[u]] + w;
            if (k < u) k = u;
            while (k + 1 < used_idx.size() && pos[used_idx[k + 1]] <= lim) ++k;
            hi_of[used_idx[u]] = used_idx[k];
        }
    }
    auto row_bound = [&](int i) { return sorted ? std::min(R[i], hi_of[i]) : R[i]; };
    std::vector<int> comp;
    comp.reserve(M);
    for (int j = 0; j < M; ++j) if (L[j] >= 0) comp.push_back(j);
    int lo_row = own_begin;  // first row an owned SNP needs: min L_j over owned computed j
    for (int j : comp) if (j >= own_begin && j < own_end) lo_row = std::min(lo_row, L[j]);
    size_t cp = 0;
    int run_rmax = -1;  // largest computed j with L_j <= current row (L non-decreasing over computed)
    out.clear();
    std::vector<PlanItem> ones;
    for (int I = std::max(0, lo_row / B); I < nblk && I * B < own_end; ++I) {
        const int i_end = std::min(M, (I + 1) * B) - 1;
        int jmax = -1;
        for (int i = I * B; i <= i_end; ++i) if (L[i] >= 0) jmax = std::max(jmax, row_bound(i));
        while (cp < comp.size() && L[comp[cp]] <= i_end) { run_rmax = comp[cp]; ++cp; }
        jmax = std::max(jmax, run_rmax);
        if (!blk_pass[I] || jmax < I * B) continue;
        const int Jmax = std::min(nblk - 1, jmax / B);
        auto useful = [&](int JJ) { return blk_pass[JJ] && (blk_own[I] || blk_own[JJ]); };
        int J = I;
        while (J <= Jmax) {
            if (!useful(J)) { ++J; continue; }
            if (max_nc == 2 && J + 1 <= Jmax && useful(J + 1)) {
                out.push_back(PlanItem{I, J, 2, 0});
                J += 2;
            } else {
                ones.push_back(PlanItem{I, J, 1, 0});
                J += 1;
            }
        }
    }
    out.insert(out.end(), ones.begin(), ones.end());
}

// Reorder single-block-pair items (row-major by I, then J) into tiles of R row blocks x C diagonal
// offsets d = J - I: tile (I / R, d / C), then I, then J.  The launch hands each XCD a contiguous
// run of the list, so the waves resident on one XCD at a time work on about R row strips and R + C
// column strips, each reused ~R or ~C times from that XCD's L2.  Row-major order (R = 1) is as good
// for narrow bands (C3: d <= 10) and poor for wide ones (C5: d <= ~220, a column strip is read by
// ~2 resident waves): 16 x 16 tiles cut the C5 band kernel by 8.5 % (profiles/r01_ab_tiles_c5.json).
void order_items_tiled(std::vector<PlanItem>& items, int nblk, int R, int C, std::vector<PlanItem>& scratch) {
    if (R <= 1 || items.empty()) return;
    std::vector<int> first(nblk + 1, 0);  // items of row block I: [first[I], first[I+1])
    int dmax = 0;
    for (const PlanItem& it : items) {
        ++first[it.x + 1];
        dmax = std::max(dmax, it.y - it.x);
    }
    if (dmax < 2 * C) return;  // narrow band: row-major is as good (C3, profiles/r01_ab_tiles_c3.json)
    for (int I = 0; I < nblk; ++I) first[I + 1] += first[I];
    std::vector<int> cur(first.begin(), first.end() - 1);  // next unread item of each row block
    scratch.clear();
    scratch.reserve(items.size());
    for (int t0 = 0; t0 < nblk; t0 += R)
        for (int c0 = 0; c0 <= dmax; c0 += C)
            for (int I = t0; I < std::min(nblk, t0 + R); ++I)
                for (int& k = cur[I]; k < first[I + 1] && items[k].y - I < c0 + C; ++k) scratch.push_back(items[k]);
    items.swap(scratch);
}

// K-split (f4, unsegmented rows) when the items fill the wave slots (2 per SIMD) in few, partly empty
// rounds — a rank's shard of one chromosome — and splitting the K loop in P pieces fills them better
// Model: a round of items takes ~0.67 us per K chunk (C3: 2 466 chunks, 1.65 ms per round, 12.7 rounds in
// 20.9 ms); the split adds ~64 KiB of partial-tile traffic per piece at ~3 TB/s effective (measured: a 1/8
// shard of C3, 3 300 items, band 3.35 -> 3.01 ms; a 1/2 shard, 13 000 items, P = 5 made it 7.5 % slower).
int choose_ksplit(int n_items, int n_it, int n_cu, bool enabled) {
    int ksplit = 1;
    if (enabled && n_items > 0 && n_it <= F4_SEG_CHUNKS) {
        const double slots = 8.0 * (double)n_cu, t_round = 0.67e-6 * n_it;
        auto cost = [&](int P) {
            return std::ceil((double)n_items * P / slots) / P * t_round +
                   (P > 1 ? n_items * P * 65536.0 / 3e12 : 0.0);
        };
        double best = cost(1);
        for (int P = 2; P <= 8 && 2 * P <= n_it; ++P)
            if (cost(P) < 0.97 * best && (size_t)n_items * P * 32768 <= ((size_t)3 << 30)) {
                best = cost(P);
                ksplit = P;
            }
    }
    return ksplit;
}

// single-block fp4 items in launches of one round of the wave slots (2 per SIMD): long unsegmented rows, at least
// BAND_ROUND_MIN rounds of items
static bool round_launches(int n_items, int n_it, int n_cu, bool use_f4, bool band_rounds) {
    return band_rounds && use_f4 && n_it >= 1024 && n_it <= F4_SEG_CHUNKS && n_items >= BAND_ROUND_MIN * 8 * n_cu;
}

BandChoice choose_band(int n_items, int n_it, int n_cu, bool use_f4, bool ksplit_enabled, bool band_rounds,
                       bool t2_cand) {
    int ksplit = choose_ksplit(n_items, n_it, n_cu, ksplit_enabled);
    // long rows: bands of at least BAND_ROUND_MIN rounds of wave slots go in round launches (the last, partial round
    // K-split), not K-split whole — a 1/8 shard of C3 (1.6 rounds) band 2.70-2.76 -> 2.61-2.64 ms, a 1/4 shard
    // (3.2 rounds) 5.21-5.26 -> 4.87-4.89 ms (profiles/r03_ab_round_min.txt; was from 4 rounds on)
    // — in the single-block kernel, as the K-split it replaces: a shard's few super-items leave most CUs of the
    // 4 x 4 kernel idle (a missing-free 1/8 shard of C3: 2.88 ms with it, 1.93-1.99 K-split whole)
    bool rounds_forced = false;
    if (round_launches(n_items, n_it, n_cu, use_f4, band_rounds)) {
        rounds_forced = ksplit > 1;
        ksplit = 1;
    }
    return {ksplit, t2_cand && ksplit == 1 && n_items > 0 && !rounds_forced};
}

// Unsegmented single-block fp4 items go in launches of one round of the wave slots each (2 per SIMD): the items
// of a launch start together and, all of equal length, stay at nearby K offsets, so the waves on one XCD that
// share a strip (the plan's 16 x 16 tiles) read it from that XCD's L2.  In one launch of all items the waves
// drift apart and most strip bytes come from beyond L2 again (C3: 68 -> 14 GB per band, the clock 1.90 -> 2.02
// GHz; band -2 to -4 % after the launch tails).  From one round of items on (BAND_ROUND_MIN), only for long rows: the
// waves of a round also reach their epilogues together, which then no longer overlap another wave's products —
// at N = 50 000 (strips of 0.4 MB, L2-resident anyway; epilogue ~1/3 of an item) round launches made the band
// 2.8 -> 5.1 ms.  The last, partial round leaves wave slots idle for a whole item length (C3: 1 458 items in
// 2 048 slots); those items are K-split instead when the cost model finds it cheaper (C3: P = 4, 3 rounds of 1/4
// of an item).
// rare-variant items of the single-block fp4 kernel run their K loops in the main launch (Gram tiles kept), their
// epilogues after the replay (launch_band_f4 rep): unsegmented rows, no K-split of the whole band (whose
// partial kernel already runs every item)
SingleShape shape_single(int n_single, int n_it, int n_cu, bool use_f4, int ksplit, bool band_rounds, bool nc2,
                         bool ksplit_ok, bool defer_wanted, size_t rep_gram_max_slots) {
    SingleShape s;
    s.round_items = ksplit == 1 && round_launches(n_single, n_it, n_cu, use_f4, band_rounds) ? 8 * n_cu : 0;
    const int tail = s.round_items > 0 ? n_single % s.round_items : 0;
    s.tail_p = tail > 0 ? choose_ksplit(tail, n_it, n_cu, use_f4 && !nc2 && ksplit_ok) : 1;
    s.n_full = s.tail_p > 1 ? n_single - tail : n_single;
    // slots for every block pair of the main launch (an upper bound: which items hold a replayed SNP is known on
    // the device only); past rep_gram_max_slots (32 KiB each) the KC launch after the replay runs those items
    // instead (a wide band of data with missing calls, where nearly every item stays in this kernel: ADVICE r03)
    s.defer = defer_wanted && use_f4 && ksplit == 1 && n_it <= F4_SEG_CHUNKS &&
              (size_t)s.n_full * (nc2 ? 2 : 1) <= rep_gram_max_slots;
    return s;
}

ColpairShape shape_colpair(int n_pairs, int n_singles, int n_it, int n_cu, int round_override, bool ksplit_ok,
                           bool defer_wanted, size_t rep_gram_max_slots) {
    ColpairShape c = {};
    const int round = round_override > 0 ? round_override : 4 * n_cu;
    const int min_rounds = round_override > 0 ? 1 : COLPAIR_ROUND_MIN;
    if (n_pairs < 0 || n_singles < 0 || n_it > F4_SEG_CHUNKS || (int64_t)n_pairs < (int64_t)min_rounds * round)
        return c;
    c.round_items = round;
    c.n_pair_full = n_pairs / round * round;
    c.n_rest = n_singles + 2 * (n_pairs - c.n_pair_full);
    // the rest continues the band: rounds of the two-wave kernel (twice the slots), the partial last one K-split
    SingleShape& r = c.rest;
    r.round_items = 2 * round;
    const int tail = c.n_rest % r.round_items;
    r.tail_p = tail > 0 ? choose_ksplit(tail, n_it, n_cu, ksplit_ok) : 1;
    r.n_full = r.tail_p > 1 ? c.n_rest - tail : c.n_rest;
    r.defer = defer_wanted && (size_t)c.n_pair_full * 2 + (size_t)r.n_full <= rep_gram_max_slots;
    return c;
}

int annot_scale_exp(double max_abs) {
    if (!(max_abs > 0.0) || !std::isfinite(max_abs)) return 0;
    int k = 0;
    const double m = std::frexp(max_abs, &k);  // max_abs = m 2^k, m in [0.5, 1): ceil(log2) is k, or k - 1 at m = 0.5
    const int e = m == 0.5 ? k - 1 : k;
    return std::max(0, e);
}

double annot_scale(int e) { return std::ldexp(1.0, 44 - e); }

int annot_batch_items(int want, size_t cap_bytes, size_t unit_bytes) {
    const size_t hold = std::max<size_t>(1, cap_bytes / ((size_t)ANNOT_KSPLIT_MAX * std::max<size_t>(unit_bytes, 1)));
    const size_t n = want > 0 ? std::min<size_t>((size_t)want, hold) : hold;
    return (int)std::min<size_t>(n, (size_t)INT32_MAX);
}

std::vector<AnnotBatch> plan_annot_batches(int n_items, int n_it, int n_cu, bool ksplit_ok, int want,
                                           size_t cap_bytes, size_t unit_bytes) {
    std::vector<AnnotBatch> out;
    const int per = annot_batch_items(want, cap_bytes, unit_bytes);
    for (int first = 0; first < n_items; first += per) {
        const int n = std::min(per, n_items - first);
        int P = choose_ksplit(n, n_it, n_cu, ksplit_ok);
        if (P > ANNOT_KSPLIT_MAX) P = ANNOT_KSPLIT_MAX;
        out.push_back({first, n, P});
    }
    return out;
}

int pairs_window_blocks(const int* L, const int* R, int own_lo, int own_hi) {
    int wb = 1;
    for (int g = own_lo; g < own_hi; ++g)
        if (L[g] >= 0) wb = std::max(wb, R[g] / 32 - L[g] / 32 + 1);
    return wb;
}

std::vector<int32_t> pairs_split_ranges(const int64_t* row_ptr, int32_t n, int64_t budget) {
    std::vector<int32_t> ends;
    int32_t lo = 0;
    while (lo < n) {
        // the last hi with row_ptr[hi] - row_ptr[lo] <= budget (row_ptr is non-decreasing), at least one row
        const int64_t* it = std::upper_bound(row_ptr + lo, row_ptr + n + 1, row_ptr[lo] + std::max<int64_t>(budget, 0));
        const int32_t hi = std::max<int32_t>((int32_t)(it - row_ptr) - 1, lo + 1);
        ends.push_back(hi);
        lo = hi;
    }
    return ends;
}

int band_kernel_code(bool use_t2, int t2_mode, int path, int ksplit, int n_it, bool colpair) {
    if (colpair) return NLDSC_BAND_F4_COLPAIR;
    if (use_t2) return t2_mode == 3 ? NLDSC_BAND_F4_QUAD : t2_mode == 1 ? NLDSC_BAND_F4_ROUTED : NLDSC_BAND_F4_2X2;
    if (path != 2) return path != 0 ? NLDSC_BAND_I8 : NLDSC_BAND_F32;
    return ksplit > 1 ? NLDSC_BAND_F4_KSPLIT : n_it > F4_SEG_CHUNKS ? NLDSC_BAND_F4_SEG : NLDSC_BAND_F4;
}

}  // namespace nldsc

extern "C" {

int nldsc_plan_band(const double* positions, const uint8_t* flags, int32_t n_snp, double ld_wind, int32_t own_begin,
                    int32_t own_end, int32_t max_nc, int32_t* L, int32_t* R, int32_t* items, int32_t cap) {
    if (!positions || !flags || !L || !R || n_snp <= 0 || own_begin < 0 || own_end > n_snp || own_begin > own_end ||
        (max_nc != 1 && max_nc != 2))
        return NLDSC_E_ARG;
    nldsc::replay_windows(positions, flags, n_snp, ld_wind, L, R);
    std::vector<nldsc::PlanItem> it;
    nldsc::plan_items(positions, flags, n_snp, ld_wind, L, R, own_begin, own_end, max_nc, it);
    if ((int64_t)it.size() > (int64_t)cap || !items) return (int)std::min<size_t>(it.size(), INT32_MAX);
    for (size_t k = 0; k < it.size(); ++k) {
        items[4 * k] = it[k].x; items[4 * k + 1] = it[k].y; items[4 * k + 2] = it[k].z; items[4 * k + 3] = 0;
    }
    return (int)it.size();
}

int nldsc_annot_scale_exp(double max_abs) { return nldsc::annot_scale_exp(max_abs); }

int nldsc_annot_plan_batches(int32_t n_items, int32_t n_it, int32_t n_cu, int32_t ksplit_ok, int32_t batch_items,
                             int32_t* batches, int32_t cap) {
    if (n_items < 0 || n_it < 2 || n_cu <= 0 || batch_items < 0) return NLDSC_E_ARG;
    const std::vector<nldsc::AnnotBatch> b = nldsc::plan_annot_batches(n_items, n_it, n_cu, ksplit_ok != 0, batch_items,
                                                                       nldsc::ANNOT_GRAM_CAP_BYTES);
    if ((int64_t)b.size() > (int64_t)cap || !batches) return (int)b.size();
    for (size_t k = 0; k < b.size(); ++k) {
        batches[3 * k] = b[k].first; batches[3 * k + 1] = b[k].n; batches[3 * k + 2] = b[k].ksplit;
    }
    return (int)b.size();
}

int nldsc_plan_batches_unit(int32_t n_items, int32_t n_it, int32_t n_cu, int32_t ksplit_ok, int32_t batch_items,
                            int64_t cap_bytes, int32_t unit_floats, int32_t* batches, int32_t cap) {
    if (n_items < 0 || n_it < 2 || n_cu <= 0 || batch_items < 0 || cap_bytes < 0 || unit_floats < 1) return NLDSC_E_ARG;
    const std::vector<nldsc::AnnotBatch> b = nldsc::plan_annot_batches(
        n_items, n_it, n_cu, ksplit_ok != 0, batch_items, cap_bytes > 0 ? (size_t)cap_bytes : nldsc::ANNOT_GRAM_CAP_BYTES,
        (size_t)unit_floats * sizeof(float));
    if ((int64_t)b.size() > (int64_t)cap || !batches) return (int)b.size();
    for (size_t k = 0; k < b.size(); ++k) {
        batches[3 * k] = b[k].first; batches[3 * k + 1] = b[k].n; batches[3 * k + 2] = b[k].ksplit;
    }
    return (int)b.size();
}

int64_t nldsc_pairs_cell(int32_t g, int32_t nb, int32_t own_begin, int32_t own_end, int32_t L_g, int32_t wb) {
    return nldsc::pairs_cell(g, nb, own_begin, own_end, L_g, wb);
}

int nldsc_pairs_window_blocks(const int32_t* L, const int32_t* R, int32_t n_snp, int32_t own_begin, int32_t own_end) {
    if (!L || !R || own_begin < 0 || own_end > n_snp || own_begin > own_end) return NLDSC_E_ARG;
    return nldsc::pairs_window_blocks(L, R, own_begin, own_end);
}

int nldsc_pairs_split_ranges(const int64_t* row_ptr, int32_t n, int64_t budget, int32_t* ends, int32_t cap) {
    if (!row_ptr || n < 0 || budget < 0) return NLDSC_E_ARG;
    for (int32_t j = 0; j < n; ++j)
        if (row_ptr[j + 1] < row_ptr[j]) return NLDSC_E_ARG;
    const std::vector<int32_t> e = nldsc::pairs_split_ranges(row_ptr, n, budget);
    if ((int64_t)e.size() > (int64_t)cap || !ends) return (int)e.size();
    std::copy(e.begin(), e.end(), ends);
    return (int)e.size();
}

}  // extern "C"
