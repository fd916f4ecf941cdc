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
// ANNOT_KSPLIT_MAX; never above that, never below 1.
int annot_batch_items(int want, size_t cap_bytes);
// the batches of n_items single-block items, in order: items [first, first + n) K-split in ksplit pieces
// (choose_ksplit of the batch; the Gram pieces are exact integers, so results do not depend on it)
struct AnnotBatch { int first, n, ksplit; };
std::vector<AnnotBatch> plan_annot_batches(int n_items, int n_it, int n_cu, bool ksplit_ok, int want,
                                           size_t cap_bytes);

// NLDSC_BAND_* (nldsc_ld.h) of a run; path: 0 fp32, 1 int8, 2 fp4; t2_mode: option "t2"
int band_kernel_code(bool use_t2, int t2_mode, int path, int ksplit, int n_it);

}  // namespace nldsc
