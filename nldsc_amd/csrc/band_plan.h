// band_plan.h — host-side window replay (ChunkwiseReader, stream.h:131-155,182-197) and the band kernel's
// work-item schedule; host-only C++ (no HIP), shared by ld_engine.cpp and the sanitizer build.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nldsc {

// one work item of the band kernels: row block x, first column block y, z column blocks (1 or 2), w = 0;
// uploaded as the kernels' int4 (same 16-byte layout)
struct PlanItem {
    int32_t x, y, z, w;
};
static_assert(sizeof(PlanItem) == 16, "PlanItem is the device int4");

void replay_windows(const double* pos, const uint8_t* flags, int n, double w, int* L, int* R);
bool positions_sorted(const double* pos, int M);
bool positions_nonneg_sorted(const double* pos, int M);
void plan_items(const double* pos, const uint8_t* flags, int M, double w, const int* L, const int* R, int own_begin,
                int own_end, int max_nc, std::vector<PlanItem>& out);
void order_items_tiled(std::vector<PlanItem>& items, int nblk, int R, int C, std::vector<PlanItem>& scratch);

// ---- launch shaping: how a run's band items go into kernel launches (pure arithmetic; ld_engine.cpp enqueue_band
// and the schedule phases act on it, tests/native/plan_tsv_check.cpp pins it) ----

// K-loop chunks (128 samples each) per fp32 accumulation segment of the fp4 path: rows longer than this
// (N > 2^19) run the segmented kernel, which folds the fp32 Gram into int32 after every segment
constexpr int F4_SEG_CHUNKS = 4096;
// round launches from this many rounds of single-block items on
constexpr int BAND_ROUND_MIN = 1;

// K-split pieces P (1: none) for n_items single-block fp4 items of n_it chunks on n_cu CUs; enabled: fp4, no
// column-block pair items, option "ksplit"
int choose_ksplit(int n_items, int n_it, int n_cu, bool enabled);
// the whole band: its K-split (overridden to 1 where the band goes in round launches) and whether the super-item
// kernels run (t2_cand: the run qualifies for them)
struct BandChoice { int ksplit; bool use_t2; };
BandChoice choose_band(int n_items, int n_it, int n_cu, bool use_f4, bool ksplit_enabled, bool band_rounds,
                       bool t2_cand);
// the single-block launches of n_single items: items [0, n_full) in launches of round_items (0: one launch), the
// rest K-split in tail_p pieces (1: no tail launch, n_full = n_single); defer: rare-variant epilogues after the replay
struct SingleShape { int round_items, tail_p, n_full; bool defer; };
SingleShape shape_single(int n_single, int n_it, int n_cu, bool use_f4, int ksplit, bool band_rounds, bool nc2,
                         bool ksplit_ok, bool defer_wanted, size_t rep_gram_max_slots);
// ---- add+dom column-pair rounds (option "f4_nc2_dom"): the one-wave 32 x 64 kernel takes the plan's (I, J, 2) pairs
// in whole rounds of one item per SIMD (4 per CU); everything else — the pairs past the last full round, back as two
// single-block items each, and the odd runs' leftover singles — is a single-block list that goes on in rounds of the
// two-wave kernel with its partial last round K-split, as the tail of a single-block band does.
// Pair rounds only from COLPAIR_ROUND_MIN full rounds on: below that the band is a shard's 1-2 rounds, whose launches
// stay what they are (one pair round of 2 048 block pairs is one round of the two-wave kernel).
constexpr int COLPAIR_ROUND_MIN = 2;
// round_items 0: no pair rounds (the single-block plan runs as it is).  Else pairs [0, n_pair_full) go in launches of
// round_items, and `rest` shapes the n_rest single-block items; defer: as SingleShape's, over both kernels' slots.
// round_override > 0 (option "colpair_round_items", tests): that many pairs per round, from one round on.
struct ColpairShape { int round_items, n_pair_full, n_rest; SingleShape rest; };
ColpairShape shape_colpair(int n_pairs, int n_singles, int n_it, int n_cu, int round_override, bool ksplit_ok,
                           bool defer_wanted, size_t rep_gram_max_slots);
// ---- annotated runs (nldsc_engine_run_annot): fixed-point scale and batches ----
// Exponent e_c of an annotation column's fixed-point scale 2^(-44 + e_c): max(0, ceil(log2(max_abs))) for the
// column's largest |a| (finite, >= 0), so |a| <= 2^e_c and a SNP's weighted total (< 2^19 * 2^e_c) fits 63 bits; a
// 0/1 column keeps the plain scale 2^-44.  annot_scale: the multiplier 2^(44 - e) the kernels apply.
int annot_scale_exp(double max_abs);
double annot_scale(int e);
// Gram scratch of an annotated band: its batches keep batch * P * 32 KiB at or below this (1 GiB)
constexpr size_t ANNOT_GRAM_CAP_BYTES = (size_t)1 << 30;
constexpr int ANNOT_KSPLIT_MAX = 8;  // choose_ksplit's largest P
// Items of one batch: `want` (option "annot_batch_items") when positive, else all the cap holds at P =
// ANNOT_KSPLIT_MAX; never above that, never below 1.  unit_bytes: the Gram tiles of one unit (one K piece of one item):
// 8 tiles of 4 KiB, or the 9 of a dom-dom run (ld_kernels.h DD_GRAM_UNIT).
constexpr size_t GRAM_UNIT_BYTES = 32768;
int annot_batch_items(int want, size_t cap_bytes, size_t unit_bytes = GRAM_UNIT_BYTES);
// the batches of n_items single-block items, in order: items [first, first + n) K-split in ksplit pieces
// (choose_ksplit of the batch; the Gram pieces are exact integers, so results do not depend on it)
struct AnnotBatch { int first, n, ksplit; };
std::vector<AnnotBatch> plan_annot_batches(int n_items, int n_it, int n_cu, bool ksplit_ok, int want,
                                           size_t cap_bytes, size_t unit_bytes = GRAM_UNIT_BYTES);

// ---- pair tables (nldsc_engine_run_pairs): the dense count matrix and the owned ranges of a pair budget ----
#ifdef __HIPCC__
#define NLDSC_HD __host__ __device__
#else
#define NLDSC_HD
#endif
// The count pass stores the kept entries of owned SNP g against the 32-SNP block nb in cell
// (g - own_lo) * Wb + (nb - L_g / 32): a row's cells in neighbour order, so the exclusive scan of the matrix is the
// CSR layout sorted by k.  L_g: g's left pointer; Wb: pairs_window_blocks.  -1: no cell (g not owned or not computed,
// or nb outside the Wb blocks from g's left pointer on — such a block holds no neighbour of g).
NLDSC_HD inline int64_t pairs_cell(int g, int nb, int own_lo, int own_hi, int L_g, int Wb) {
    if (g < own_lo || g >= own_hi || L_g < 0) return -1;
    const int c = nb - L_g / 32;
    if (c < 0 || c >= Wb) return -1;
    return (int64_t)(g - own_lo) * Wb + c;
}
// Wb: the widest window of the owned computed SNPs in 32-SNP blocks, max (R_g / 32 - L_g / 32 + 1); at least 1
int pairs_window_blocks(const int* L, const int* R, int own_lo, int own_hi);
// Gram scratch of a pairs band (8 GiB: the C3 band, 26 034 items, in one batch — the emit pass then reads the count
// pass's tiles instead of computing them again)
constexpr size_t PAIRS_GRAM_CAP_BYTES = (size_t)8 << 30;
// cells of the dense count matrix a run may use (option "pairs_max_cells" overrides it): 2^27 ints, 512 MiB
constexpr int64_t PAIRS_MAX_CELLS = (int64_t)1 << 27;
// Owned ranges of at most `budget` pairs from the row_ptr[n + 1] of a sizing call: ends[k] is the end of range k
// (ranges tile [0, n); a single row above the budget is a range of its own; n = 0 gives none)
std::vector<int32_t> pairs_split_ranges(const int64_t* row_ptr, int32_t n, int64_t budget);

// NLDSC_BAND_* (nldsc_ld.h) of a run; path: 0 fp32, 1 int8, 2 fp4; t2_mode: option "t2"
int band_kernel_code(bool use_t2, int t2_mode, int path, int ksplit, int n_it, bool colpair = false);

}  // namespace nldsc
