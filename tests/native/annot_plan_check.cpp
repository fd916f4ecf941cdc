// annot_plan_check.cpp — the pure host arithmetic of annotated runs (band_plan.cpp: annot_scale_exp, annot_scale,
// annot_batch_items, plan_annot_batches and their C ABI wrappers) under ASan + UBSan, on fixed and random inputs,
// against restatements written here.  Prints "annot_plan_check OK" and exits 0 when every check holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../include/nldsc_ld.h"
#include "../../nldsc_amd/csrc/band_plan.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// e_c by search: the smallest e >= 0 with max_abs <= 2^e
static int exp_by_search(double max_abs) {
    int e = 0;
    while (std::ldexp(1.0, e) < max_abs) ++e;
    return e;
}

int main() {
    using namespace nldsc;
    // the issue's maxima
    CHECK(annot_scale_exp(0.0) == 0);
    CHECK(annot_scale_exp(1.0) == 0);
    CHECK(annot_scale_exp(1.5) == 1);
    CHECK(annot_scale_exp(2.0) == 1);
    CHECK(annot_scale_exp(1000.0) == 10);
    CHECK(annot_scale_exp(1e-3) == 0);
    CHECK(annot_scale_exp(-1.0) == 0 && annot_scale_exp(NAN) == 0 && annot_scale_exp(INFINITY) == 0);
    CHECK(annot_scale_exp(std::nextafter(2.0, 3.0)) == 2 && annot_scale_exp(std::nextafter(2.0, 0.0)) == 1);
    CHECK(annot_scale_exp(1e300) == exp_by_search(1e300) && annot_scale_exp(5e-324) == 0);
    CHECK(annot_scale(0) == 17592186044416.0 && annot_scale(10) == 17179869184.0);
    CHECK(nldsc_annot_scale_exp(1000.0) == 10);
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> mant(0.5, 1.0);
    for (int k = 0; k < 20000; ++k) {
        const double x = std::ldexp(mant(rng), (int)(rng() % 80) - 20);
        const int e = annot_scale_exp(x);
        CHECK(e == exp_by_search(x));
        // a SNP's total: fewer than 2^19 pairs of |a r2| <= 2^e each, in units of 1 / scale: below 2^63
        CHECK(std::ldexp(x, 19) * annot_scale(e) <= std::ldexp(1.0, 63));
    }
    for (int e = 0; e < 60; ++e) CHECK(annot_scale_exp(std::ldexp(1.0, e)) == e);

    // batches
    const size_t cap = ANNOT_GRAM_CAP_BYTES;
    CHECK(annot_batch_items(0, cap) == (int)(cap / (8 * 32768)));
    CHECK(annot_batch_items(7, cap) == 7 && annot_batch_items(1, cap) == 1);
    CHECK(annot_batch_items(1 << 30, cap) == (int)(cap / (8 * 32768)));
    CHECK(annot_batch_items(0, 1) == 1);
    CHECK(plan_annot_batches(0, 64, 256, true, 0, cap).empty());
    for (int k = 0; k < 3000; ++k) {
        const int n_items = (int)(rng() % 60000), n_it = 2 * (1 + (int)(rng() % 2048)), n_cu = 1 + (int)(rng() % 304);
        const int want = (rng() & 1) ? 0 : (int)(rng() % 9000);
        const bool ks = (rng() & 2) != 0;
        const std::vector<AnnotBatch> b = plan_annot_batches(n_items, n_it, n_cu, ks, want, cap);
        const int per = annot_batch_items(want, cap);
        int next = 0;
        for (size_t q = 0; q < b.size(); ++q) {
            CHECK(b[q].first == next && b[q].n >= 1 && b[q].n <= per);
            CHECK(q + 1 == b.size() || b[q].n == per);  // only the last batch is ragged
            CHECK(b[q].ksplit >= 1 && b[q].ksplit <= ANNOT_KSPLIT_MAX && 2 * b[q].ksplit <= n_it);
            CHECK(ks || b[q].ksplit == 1);
            CHECK(b[q].ksplit == choose_ksplit(b[q].n, n_it, n_cu, ks));
            CHECK((size_t)b[q].n * (size_t)b[q].ksplit * 32768 <= cap);
            next += b[q].n;
        }
        CHECK(next == n_items);
        // the C ABI wrapper: count first, then the rows
        const int cnt = nldsc_annot_plan_batches(n_items, n_it, n_cu, ks, want, nullptr, 0);
        CHECK(cnt == (int)b.size());
        std::vector<int32_t> rowsv(3 * b.size() + 3, -1);
        CHECK(nldsc_annot_plan_batches(n_items, n_it, n_cu, ks, want, rowsv.data(), (int32_t)b.size()) == cnt);
        for (size_t q = 0; q < b.size(); ++q)
            CHECK(rowsv[3 * q] == b[q].first && rowsv[3 * q + 1] == b[q].n && rowsv[3 * q + 2] == b[q].ksplit);
        CHECK(rowsv[3 * b.size()] == -1);
        if (b.size() > 1) {  // too small a capacity writes nothing
            std::vector<int32_t> small(3, -1);
            CHECK(nldsc_annot_plan_batches(n_items, n_it, n_cu, ks, want, small.data(), 1) == cnt && small[0] == -1);
        }
    }
    CHECK(nldsc_annot_plan_batches(-1, 64, 256, 1, 0, nullptr, 0) == NLDSC_E_ARG);
    CHECK(nldsc_annot_plan_batches(10, 1, 256, 1, 0, nullptr, 0) == NLDSC_E_ARG);
    CHECK(nldsc_annot_plan_batches(10, 64, 0, 1, 0, nullptr, 0) == NLDSC_E_ARG);
    CHECK(nldsc_annot_plan_batches(10, 64, 256, 1, -5, nullptr, 0) == NLDSC_E_ARG);
    if (failures) {
        std::fprintf(stderr, "annot_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("annot_plan_check OK\n");
    return 0;
}
