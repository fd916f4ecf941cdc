// CPU sanitizer driver for the engine's host code (built by `make -C nldsc_amd/csrc sanitize` with
// -fsanitize=address,undefined; run by tests/test_sanitize.py).  No GPU, no HIP.
//  * nldsc_plan_band (band_plan.cpp): window replay and band schedule on random inputs — sorted, tied,
//    negative, NaN and unsorted positions, MAF failures, empty and partial owned ranges, windows from 0 to
//    everything — checked against a brute-force restatement of the reference's ChunkwiseReader pointers
//    (stream.h:131-155,182-197): every needed 32-SNP block pair covered exactly once, every item in range.
//  * launch shaping (band_plan.cpp choose_ksplit, choose_band, shape_single, band_kernel_code): a table of cost-model
//    values and the structural rules the GPU tests rely on.
//  * nldsc_format_scores (tsv_format.cpp): "%.5f" fields, NaN as '', against snprintf on random, tie,
//    tiny, huge and non-finite values.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nldsc_ld.h"
#include "../../nldsc_amd/csrc/band_plan.h"

static int fails = 0;
#define CHECK(c, ...)                                            \
    do {                                                         \
        if (!(c)) {                                              \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                   \
            std::fprintf(stderr, "\n");                          \
            if (++fails > 20) std::exit(1);                      \
        }                                                        \
    } while (0)

// brute-force ChunkwiseReader pointers (same semantics, written independently of band_plan.cpp)
static void naive_replay(const std::vector<double>& pos, const std::vector<uint8_t>& pass, double w,
                         std::vector<int>& L, std::vector<int>& R) {
    const int n = (int)pos.size();
    auto used = [&](int i) { return i >= 0 && i < n && pos[i] >= 0; };
    auto inwin = [&](int a, int b) { return used(a) && used(b) && std::fabs(pos[b] - pos[a]) <= w; };
    L.assign(n, -1);
    R.assign(n, -2);
    int left = 0, right = -1;
    for (int j = 0; j < n; ++j) {
        if (!used(j)) continue;
        for (;;) {
            if (right + 1 >= n) break;
            ++right;
            if (!inwin(j, right)) break;
        }
        if (!(j <= right && pass[j])) continue;
        while (left < j && !(pass[left] && inwin(j, left))) ++left;
        L[j] = left;
        R[j] = right;
    }
}

static void check_plan(std::mt19937_64& rng, int iter) {
    std::uniform_real_distribution<double> U(0.0, 1.0);
    const int n = 1 + (int)(rng() % (iter % 5 == 0 ? 3000 : 300));
    std::vector<double> pos(n);
    double x = 0;
    const double gap = 0.01 + U(rng);
    for (int j = 0; j < n; ++j) {
        x += (U(rng) < 0.1) ? 0.0 : gap * U(rng);  // ~10 % duplicates
        pos[j] = std::round(x * 64.0) / 64.0;       // dyadic: exact window ties
    }
    const int kind = iter % 6;
    if (kind == 1) for (int k = 0; k < 1 + n / 50; ++k) pos[rng() % n] = -1.0;
    if (kind == 2) pos[rng() % n] = std::nan("");
    if (kind == 3) for (int k = 0; k < 1 + n / 20; ++k) std::swap(pos[rng() % n], pos[rng() % n]);
    std::vector<uint8_t> pass(n);
    const double fail_rate = (iter % 3) * 0.2;
    for (auto& p : pass) p = U(rng) >= fail_rate;
    const double ws[] = {0.0, 0.25, 1.0, 3.0, 1e9};
    const double w = ws[rng() % 5] * gap * 4;
    int ob = (int)(rng() % (n + 1)), oe = (int)(rng() % (n + 1));
    if (ob > oe) std::swap(ob, oe);
    if (iter % 4 == 0) { ob = 0; oe = n; }
    const int max_nc = 1 + (int)(rng() % 2);

    std::vector<int32_t> L(n), R(n);
    const int k = nldsc_plan_band(pos.data(), pass.data(), n, w, ob, oe, max_nc, L.data(), R.data(), nullptr, 0);
    CHECK(k >= 0, "plan count %d", k);
    std::vector<int32_t> items(4 * (size_t)std::max(k, 1));
    const int k2 = nldsc_plan_band(pos.data(), pass.data(), n, w, ob, oe, max_nc, L.data(), R.data(), items.data(), k);
    CHECK(k2 == k, "plan %d vs %d", k2, k);
    std::vector<int> NL, NR;
    naive_replay(pos, pass, w, NL, NR);
    for (int j = 0; j < n; ++j) CHECK(L[j] == NL[j] && R[j] == NR[j], "pointers of %d: (%d,%d) vs (%d,%d)", j, L[j], R[j], NL[j], NR[j]);
    const int nblk = (n + 31) / 32;
    std::set<std::pair<int, int>> cover;
    for (int q = 0; q < k; ++q) {
        const int I = items[4 * q], J = items[4 * q + 1], z = items[4 * q + 2];
        CHECK(I >= 0 && I <= J && (z == 1 || (z == 2 && max_nc == 2)) && J + z <= nblk, "item (%d,%d,%d)", I, J, z);
        for (int c = 0; c < z; ++c) CHECK(cover.insert({I, J + c}).second, "block pair (%d,%d) twice", I, J + c);
    }
    auto used = [&](int i) { return pos[i] >= 0; };
    for (int j = 0; j < n; ++j) {
        if (NL[j] < 0) continue;
        for (int i = NL[j]; i <= NR[j] && i < n; ++i) {
            if (i == j || !pass[i] || !used(i) || !(std::fabs(pos[i] - pos[j]) <= w)) continue;
            const bool owned = (j >= ob && j < oe) || (i >= ob && i < oe && NL[i] >= 0);
            if (!(j >= ob && j < oe)) continue;  // the pair contributes to owned j
            (void)owned;
            const int a = std::min(i, j) / 32, b = std::max(i, j) / 32;
            CHECK(cover.count({a, b}), "pair (%d,%d) of owned %d not covered (blocks %d,%d; n=%d w=%g own=[%d,%d))",
                  i, j, j, a, b, n, w, ob, oe);
        }
    }
}

static std::string f5(double v) {
    if (std::isnan(v)) return "";
    char b[512];
    std::snprintf(b, sizeof b, "%.5f", v);
    return b;
}

static void check_tsv(std::mt19937_64& rng, int iter) {
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const int n = 1 + (int)(rng() % 200);
    std::vector<double> c[5];
    std::vector<int32_t> ic[3];
    const double specials[] = {0.0, -0.0, 0.000005, 0.000015, 0.000025, 2.5e-6, 1e-300, -1e-300, 5e-324,
                               123456789.123455, 9.0e13, 8.9999999999e13, 1e300, -1e300, HUGE_VAL, -HUGE_VAL,
                               std::nan(""), 0.5, 1.0, 99999.999995, 1.000005, 2.675e-5};
    for (auto& v : c) {
        v.resize(n);
        for (auto& x : v) {
            const int m = (int)(rng() % 4);
            x = m == 0 ? specials[rng() % (sizeof specials / sizeof specials[0])]
              : m == 1 ? U(rng) * std::pow(10.0, (double)(rng() % 30) - 15.0)
              : m == 2 ? std::round(U(rng) * 1e7) / 1e5 + 5e-6 * (rng() % 2) : U(rng) * 1000.0;
        }
    }
    for (auto& v : ic) {
        v.resize(n);
        for (auto& x : v) x = (int32_t)(rng() % 100000) - 1;
    }
    const int extra = iter % 2;
    std::string prefix, expect;
    for (int i = 0; i < n; ++i) {
        const std::string p = std::to_string(1 + i % 22) + "\trs" + std::to_string(i) + "\t" + std::to_string(1000 * i);
        prefix += p + (i + 1 < n ? "\n" : "");
        expect += p + "\t" + f5(c[0][i]) + "\t" + f5(c[1][i]);
        if (extra)
            expect += "\t" + f5(c[2][i]) + "\t" + std::to_string(ic[0][i]) + "\t" + std::to_string(ic[1][i]) + "\t" +
                      std::to_string(ic[2][i]) + "\t" + f5(c[3][i]);
        expect += "\n";
    }
    std::vector<char> out(prefix.size() + (size_t)n * (16 + 7 * 400) + 1);
    const int64_t got = nldsc_format_scores(prefix.data(), (int64_t)prefix.size(), n, c[0].data(), c[1].data(),
                                            c[2].data(), ic[0].data(), ic[1].data(), ic[2].data(), c[3].data(), extra,
                                            out.data(), (int64_t)out.size());
    CHECK(got == (int64_t)expect.size() && std::memcmp(out.data(), expect.data(), expect.size()) == 0,
          "tsv mismatch (n=%d extra=%d, %lld vs %zu bytes)", n, extra, (long long)got, expect.size());
    // too small a buffer must fail cleanly, not overflow
    const int64_t small = nldsc_format_scores(prefix.data(), (int64_t)prefix.size(), n, c[0].data(), c[1].data(),
                                              c[2].data(), ic[0].data(), ic[1].data(), ic[2].data(), c[3].data(), extra,
                                              out.data(), 8);
    CHECK(small < 0, "undersized buffer accepted (%lld)", (long long)small);
}

// the GPU schedule's condition in one pass: equal to "sorted among the non-negative ones and all non-negative"
static void check_sorted(std::mt19937_64& rng, int iter) {
    const int M = (int)(rng() % 200);
    std::vector<double> P(M);
    double x = 0;
    for (int j = 0; j < M; ++j) {
        x += (double)(rng() % 3);
        const int kind = (int)(rng() % 60);
        P[j] = kind == 0 ? -1.0 : kind == 1 ? std::nan("") : kind == 2 ? x - 2.5 : x;
    }
    bool all_nonneg = true;
    for (double v : P) all_nonneg &= v >= 0.0;
    const bool expect = all_nonneg && nldsc::positions_sorted(P.data(), M);
    CHECK(nldsc::positions_nonneg_sorted(P.data(), M) == expect, "positions_nonneg_sorted (M=%d, iter %d)", M, iter);
}

// Launch shaping (band_plan.h).  The choose_ksplit values are those of the cost-model lambda this function replaced
// in ld_engine.cpp, compiled on its own and run over these inputs (g++ -O2 and clang++ -O3 agree) — not values read
// back from the new function.
static void check_launch_shape(std::mt19937_64& rng) {
    using namespace nldsc;
    static const int table[][4] = {  // n_items, n_it, n_cu, P
        {1458, 2466, 256, 4},  {3283, 2466, 256, 3}, {13000, 2466, 256, 1}, {26034, 2466, 256, 1},
        {2048, 2466, 256, 1},  {2049, 2466, 256, 4}, {1, 2466, 256, 8},     {300, 1564, 256, 6},
        {700, 1025, 256, 5},   {100, 2, 256, 1},     {100, 4, 256, 1},      {20000, 4097, 256, 1},
        {0, 2466, 256, 1},     {1000, 4096, 256, 2}, {1500, 2466, 304, 3},  {500, 512, 64, 1},
        {40, 16, 8, 3},        {2000, 3000, 128, 1}, {12000, 4096, 256, 1}, {5, 5, 256, 2},
        {3, 6, 1, 2},          {1024, 1024, 256, 2}};
    for (const auto& t : table) {
        CHECK(choose_ksplit(t[0], t[1], t[2], true) == t[3], "choose_ksplit(%d, %d, %d) = %d, expected %d", t[0], t[1],
              t[2], choose_ksplit(t[0], t[1], t[2], true), t[3]);
        CHECK(choose_ksplit(t[0], t[1], t[2], false) == 1, "choose_ksplit(%d, %d, %d) disabled", t[0], t[1], t[2]);
    }
    const int n_its[] = {2, 512, 1023, 1024, 1564, 2466, F4_SEG_CHUNKS, F4_SEG_CHUNKS + 1, 8192};
    const int n_cus[] = {1, 8, 64, 256, 304};
    for (int iter = 0; iter < 20000; ++iter) {
        const int n_it = n_its[rng() % 9], n_cu = n_cus[rng() % 5], slots = 8 * n_cu;
        const int edge[] = {0, 1, slots - 1, slots, slots + 1, 2 * slots, 3 * slots + slots / 2};
        const int n = rng() % 2 ? edge[rng() % 7] : (int)(rng() % (size_t)(14 * slots));
        const bool use_f4 = rng() % 8 != 0, rounds = rng() % 4 != 0, nc2 = rng() % 4 == 0, ok = rng() % 4 != 0;
        const bool want = rng() % 4 != 0, t2_cand = rng() % 2 != 0;
        const size_t max_slots = rng() % 2 ? (size_t)1 << 16 : (size_t)(rng() % (size_t)(4 * slots));
        const bool round_cond = use_f4 && rounds && n_it >= 1024 && n_it <= F4_SEG_CHUNKS && n >= slots;
        // the whole band: K-split overridden to 1 under the round-launch condition, super-items only without either
        const bool en = use_f4 && !nc2 && ok;
        const int p_whole = choose_ksplit(n, n_it, n_cu, en);
        const BandChoice c = choose_band(n, n_it, n_cu, use_f4, en, rounds, t2_cand);
        CHECK(c.ksplit == (round_cond ? 1 : p_whole), "band K-split %d (model %d, rounds %d)", c.ksplit, p_whole,
              (int)round_cond);
        CHECK(c.use_t2 == (t2_cand && n > 0 && p_whole == 1), "use_t2 %d (n %d, model %d)", (int)c.use_t2, n, p_whole);
        // the single-block launches
        const int ksplit = rng() % 4 ? 1 : 1 + (int)(rng() % 8);
        const SingleShape s = shape_single(n, n_it, n_cu, use_f4, ksplit, rounds, nc2, ok, want, max_slots);
        CHECK(s.round_items == (round_cond && ksplit == 1 ? slots : 0), "round_items %d (n %d, n_it %d, n_cu %d)",
              s.round_items, n, n_it, n_cu);
        const int tail = n - s.n_full;
        CHECK(s.n_full >= 0 && tail >= 0 && s.tail_p >= 1 && s.tail_p <= 8, "shape (%d, %d, %d)", s.n_full, tail, s.tail_p);
        if (s.tail_p > 1) {
            CHECK(s.round_items > 0 && s.n_full % s.round_items == 0 && tail > 0 && tail < s.round_items,
                  "K-split tail of %d after %d items in rounds of %d", tail, s.n_full, s.round_items);
            CHECK(s.tail_p == choose_ksplit(tail, n_it, n_cu, en) && 2 * s.tail_p <= n_it, "tail_p %d", s.tail_p);
        } else {
            CHECK(tail == 0, "%d items in no launch", tail);
        }
        const bool fits = (size_t)s.n_full * (nc2 ? 2 : 1) <= max_slots;
        CHECK(s.defer == (want && use_f4 && ksplit == 1 && n_it <= F4_SEG_CHUNKS && fits), "defer %d (n_full %d of %zu)",
              (int)s.defer, s.n_full, max_slots);
    }
    // the C3 tail: 1 458 items past 12 full rounds, K-split in 4
    const SingleShape c3 = shape_single(26034, 2466, 256, true, 1, true, false, true, true, (size_t)1 << 16);
    CHECK(c3.round_items == 2048 && c3.n_full == 24576 && c3.tail_p == 4 && c3.defer, "C3 shape (%d, %d, %d, %d)",
          c3.round_items, c3.n_full, c3.tail_p, (int)c3.defer);
    CHECK(band_kernel_code(true, 3, 2, 1, 2466) == NLDSC_BAND_F4_QUAD && band_kernel_code(true, 1, 2, 1, 2466) == NLDSC_BAND_F4_ROUTED &&
              band_kernel_code(true, 2, 2, 1, 2466) == NLDSC_BAND_F4_2X2 && band_kernel_code(false, 3, 2, 1, 2466) == NLDSC_BAND_F4 &&
              band_kernel_code(false, 3, 2, 3, 2466) == NLDSC_BAND_F4_KSPLIT && band_kernel_code(false, 3, 2, 1, 4097) == NLDSC_BAND_F4_SEG &&
              band_kernel_code(false, 3, 1, 1, 2466) == NLDSC_BAND_I8 && band_kernel_code(false, 3, 0, 1, 2466) == NLDSC_BAND_F32,
          "band kernel codes");
}

int main() {
    std::mt19937_64 rng(2024);
    for (int it = 0; it < 600; ++it) check_plan(rng, it);
    for (int it = 0; it < 2000; ++it) check_sorted(rng, it);
    std::mt19937_64 shape_rng(2025);  // (its own stream: the table checks below keep theirs)
    check_launch_shape(shape_rng);
    // argument checks of the C ABI
    double p1[2] = {0, 1};
    uint8_t f1[2] = {1, 1};
    int32_t l1[2], r1[2];
    CHECK(nldsc_plan_band(p1, f1, 2, 1.0, 1, 0, 1, l1, r1, nullptr, 0) < 0, "bad own range accepted");
    CHECK(nldsc_plan_band(p1, f1, 2, 1.0, 0, 2, 3, l1, r1, nullptr, 0) < 0, "bad max_nc accepted");
    for (int it = 0; it < 400; ++it) check_tsv(rng, it);
    if (fails) {
        std::fprintf(stderr, "%d failures\n", fails);
        return 1;
    }
    std::printf("plan_tsv_check OK (600 plans, 2000 position checks, 400 tables)\n");
    return 0;
}
