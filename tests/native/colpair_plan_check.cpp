// colpair_plan_check.cpp — launch shaping of the add+dom column-pair rounds (band_plan.cpp: shape_colpair) under
// ASan + UBSan, on the C3 counts, the edges of its rules and random inputs, against restatements written here.
// Prints "colpair_plan_check OK" and exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <random>

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

int main() {
    using namespace nldsc;
    const int n_cu = 256, n_it = 2466;  // MI355X, C3 rows
    const size_t slots = (size_t)1 << 16;
    {   // C3: 26 034 block pairs = 12 392 pairs + 1 250 leftover singles
        const ColpairShape c = shape_colpair(12392, 1250, n_it, n_cu, 0, true, true, slots);
        CHECK(c.round_items == 4 * n_cu);                 // one pair per SIMD
        CHECK(c.n_pair_full == 12 * 1024);                // 12 full rounds, no pair in a partial round
        CHECK(c.n_rest == 1250 + 2 * (12392 - 12288));    // the last pairs as two singles each, and the leftovers
        CHECK(c.rest.round_items == 8 * n_cu);            // the rest in the two-wave kernel's rounds
        CHECK(c.rest.tail_p == choose_ksplit(c.n_rest, n_it, n_cu, true) && c.rest.tail_p > 1);  // K-split, as a tail is
        CHECK(c.rest.n_full == 0);
        CHECK(c.rest.defer);                              // 2 * 12 288 + 0 slots <= 2^16
        CHECK(band_kernel_code(false, 3, 2, 1, n_it, true) == NLDSC_BAND_F4_COLPAIR);
        CHECK(band_kernel_code(false, 3, 2, 1, n_it) == NLDSC_BAND_F4);
    }
    {   // below COLPAIR_ROUND_MIN full rounds (a shard's 1.6 rounds of single blocks; exactly one pair round): none
        CHECK(shape_colpair(1600, 100, n_it, n_cu, 0, true, true, slots).round_items == 0);
        CHECK(shape_colpair(1024, 32, n_it, n_cu, 0, true, true, slots).round_items == 0);
        CHECK(shape_colpair(2 * 1024 - 1, 0, n_it, n_cu, 0, true, true, slots).round_items == 0);
        const ColpairShape c = shape_colpair(2 * 1024, 0, n_it, n_cu, 0, true, true, slots);
        CHECK(c.round_items == 1024 && c.n_pair_full == 2048 && c.n_rest == 0 && c.rest.n_full == 0 &&
              c.rest.tail_p == 1);
        CHECK(shape_colpair(100000, 0, F4_SEG_CHUNKS + 2, n_cu, 0, true, true, slots).round_items == 0);  // segmented rows
        CHECK(shape_colpair(-1, 0, n_it, n_cu, 0, true, true, slots).round_items == 0);
    }
    {   // a rest above one round of the two-wave kernel: its full rounds stay whole, the tail is K-split
        const ColpairShape c = shape_colpair(3 * 1024 + 1000, 500, n_it, n_cu, 0, true, false, slots);
        CHECK(c.n_pair_full == 3072 && c.n_rest == 2500);
        CHECK(c.rest.tail_p == choose_ksplit(2500 - 2048, n_it, n_cu, true));
        CHECK(c.rest.n_full == (c.rest.tail_p > 1 ? 2048 : 2500));
        CHECK(!c.rest.defer);
        const ColpairShape k = shape_colpair(3 * 1024 + 1000, 500, n_it, n_cu, 0, false, true, slots);  // option ksplit 0
        CHECK(k.rest.tail_p == 1 && k.rest.n_full == k.n_rest);
        // too many deferred slots: the KC launch instead
        CHECK(!shape_colpair(40 * 1024, 0, n_it, n_cu, 0, true, true, slots).rest.defer);
    }
    {   // the tests' round size: from one round on, on any unsegmented rows
        const ColpairShape c = shape_colpair(7, 7, 2, n_cu, 4, true, true, slots);
        CHECK(c.round_items == 4 && c.n_pair_full == 4 && c.n_rest == 7 + 6 && c.rest.round_items == 8);
        CHECK(shape_colpair(3, 7, 2, n_cu, 4, true, true, slots).round_items == 0);
    }
    std::mt19937_64 rng(2024);
    for (int k = 0; k < 20000; ++k) {
        const int np = (int)(rng() % 60000), ns = (int)(rng() % 6000), cu = 1 + (int)(rng() % 320);
        const int ov = rng() % 4 == 0 ? 1 + (int)(rng() % 50) : 0, it = 2 + 2 * (int)(rng() % 2047);
        const ColpairShape c = shape_colpair(np, ns, it, cu, ov, rng() % 2, rng() % 2, slots);
        const int round = ov ? ov : 4 * cu;
        if (np < (ov ? 1 : COLPAIR_ROUND_MIN) * round) {
            CHECK(c.round_items == 0);
            continue;
        }
        CHECK(c.round_items == round && c.n_pair_full % round == 0 && np - c.n_pair_full < round && c.n_pair_full > 0);
        CHECK(2 * c.n_pair_full + c.n_rest == 2 * np + ns);  // every block pair once
        CHECK(c.rest.n_full >= 0 && c.rest.n_full <= c.n_rest && c.rest.tail_p >= 1 && c.rest.tail_p <= 8);
        CHECK(c.rest.tail_p == 1 ? c.rest.n_full == c.n_rest : c.rest.n_full % (2 * round) == 0);
        CHECK(!c.rest.defer || (size_t)2 * c.n_pair_full + c.rest.n_full <= slots);
    }
    if (failures) {
        std::fprintf(stderr, "colpair_plan_check: %d failures\n", failures);
        return 1;
    }
    std::printf("colpair_plan_check OK\n");
    return 0;
}
