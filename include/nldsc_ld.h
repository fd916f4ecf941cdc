/*
 * nldsc_ld.h — C ABI of the MI355X-native LD-score engine (libnldsc_amd.so).
 *
 * Drop-in boundary for bayarpark/nldsc's `_ldscore` extension:
 *   - nldsc_ld_params  replaces  struct LDScoreParams   nldsc/ldscore/_ldscore/data.h:33-65
 *   - nldsc_ld_result  replaces  struct LDScoreResult   nldsc/ldscore/_ldscore/data.h:21-31
 *   - nldsc_ld_calculate replaces LDScoreResult calculate(LDScoreParams&)
 *                                                       nldsc/ldscore/_ldscore/ldscalc.h:8
 *     as bound by m.def("calculate", &calculate)        nldsc/ldscore/_ldscore/ldscore.cpp:53
 * The pybind11 module `_ldscore` (nldsc_amd/csrc/ldscore_py.cpp) wraps exactly
 * these entry points with the reference's Python signatures.
 *
 * The engine entry points below are the lower-level API used for device-resident
 * inputs, repeated runs (benchmarks) and position sharding across GPUs.
 *
 * Plain C types only: pointers, sizes, ints and doubles.  All output arrays are
 * caller-allocated with n_snp elements.  Every function returns NLDSC_OK (0) or
 * a negative NLDSC_E_* code; when `err` is non-NULL a NUL-terminated message is
 * written into it (at most errlen bytes).
 */
#ifndef NLDSC_LD_H
#define NLDSC_LD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NLDSC_OK 0
#define NLDSC_E_BAD_MAGIC (-1) /* "Invalid PLINK magic number..." (stream.h:88-102) -> ValueError */
#define NLDSC_E_IO (-2)        /* cannot open / read the .bed file */
#define NLDSC_E_SIZE (-3)      /* .bed shorter than 3 + n_snp * ceil(n_org / 4) bytes */
#define NLDSC_E_ARG (-4)       /* invalid argument (sizes, NULL pointers, ranges) */
#define NLDSC_E_HIP (-5)       /* HIP runtime error */
#define NLDSC_E_OOM (-6)       /* device or host allocation failed */
#define NLDSC_E_NODEV (-7)     /* no HIP device visible: there is no CPU fallback */
#define NLDSC_E_SPACE (-8)     /* a caller's output array is too small; the message names the needed count */

/* flags */
#define NLDSC_FLAG_STRICT_PLINK_ORDER 1u /* use PLINK sample order in the last .bed byte (reference
                                            keeps the high n_org%4 bit pairs, stream.h:55-66) */
#define NLDSC_FLAG_ADDITIVE_ONLY 2u      /* skip the dominance terms: l2d = NaN, l2d_ws = l2d_wse = -1 */
#define NLDSC_FLAG_EXACT_I8 4u           /* correlations from exact integer Gram products (int8 MFMA) */
#define NLDSC_FLAG_FP32 8u               /* correlations from fp32 standardised values (fp32 MFMA) */
#define NLDSC_FLAG_EXACT_F4 16u          /* exact integer Gram products on fp4 MFMAs (n_org < 2^27, segmented
                                            above 2^19; larger cohorts fall back to EXACT_I8) */
#define NLDSC_FLAG_EXACT_RARE 32u        /* rare variants (<= 16 calls in one genotype class): exact standardised
                                            vectors instead of the default, the reference's fp32 ones replayed
                                            step for step (encoder.h:124-133, tools.h:54-85) — its rounding is
                                            not small against a nearly constant vector: the fp32 mean does not
                                            centre it, and a residual without hom-A1 calls is exactly constant
                                            (std 0) but rounding noise in the reference, often above --std-thr */
/* None of EXACT_F4, EXACT_I8, FP32: the engine default, EXACT_F4 (engine option "band_mode" overrides it). */

typedef struct nldsc_ld_params {
    const char* bedfile;      /* LDScoreParams::bedfile   (data.h:34) */
    int32_t n_snp;            /* LDScoreParams::n_snp     (data.h:36) */
    int32_t n_org;            /* LDScoreParams::n_org     (data.h:37) */
    double ld_wind;           /* LDScoreParams::ld_wind   (data.h:39), same unit as positions */
    const double* positions;  /* LDScoreParams::positions (data.h:40), n_snp values; < 0 = unused */
    double maf;               /* LDScoreParams::maf       (data.h:42) */
    double std_thr;           /* LDScoreParams::std_thr   (data.h:43) */
    double rsq_thr;           /* LDScoreParams::rsq_thr   (data.h:44) */
    uint32_t flags;           /* NLDSC_FLAG_* */
    int32_t device;           /* HIP device ordinal; -1 = the calling thread's current device */
} nldsc_ld_params;

typedef struct nldsc_ld_result { /* LDScoreResult (data.h:21-31); n_snp elements each */
    double* l2;              /* additive LD score; NaN for unused / MAF-failed SNPs */
    double* l2d;             /* dominance LD score; NaN likewise */
    double* maf;             /* MAF of every decoded SNP; NaN for unused SNPs */
    double* residuals_std;   /* std of the dominance residual; NaN unless the SNP passed MAF */
    int32_t* l2_ws;          /* window size (additive), -1 when not computed */
    int32_t* l2d_ws;         /* neighbours with residual std > std_thr, -1 when not computed */
    int32_t* l2d_wse;        /* ... of which r2adj > rsq_thr, -1 when not computed */
} nldsc_ld_result;

/* One-shot call: read `p->bedfile`, compute on the GPU, fill `r`. */
int nldsc_ld_calculate(const nldsc_ld_params* p, nldsc_ld_result* r, char* err, size_t errlen);
/* The same on a subset of the individuals (PLINK's / LDSC's --keep): idx[n_keep] are the kept individuals' 0-based
 * .fam line numbers, strictly ascending (nldsc_engine_set_keep below: the rules and the sample order); p->n_org is
 * the file's individual count.  idx == NULL: everyone, as nldsc_ld_calculate. */
int nldsc_ld_calculate_keep(const nldsc_ld_params* p, const int32_t* idx, int32_t n_keep, nldsc_ld_result* r,
                            char* err, size_t errlen);
/* One-shot partitioned LD scores (nldsc_engine_run_annot below: the layout of `annot`, `l2_annot`, `l2d_annot` and the
 * rules): read `p->bedfile`, on the individuals idx[n_keep] when idx != NULL (nldsc_ld_calculate_keep), fill `r` and
 * the per-annotation scores of all n_snp SNPs. */
int nldsc_ld_calculate_annot(const nldsc_ld_params* p, const int32_t* keep_idx, int32_t n_keep, const double* annot,
                             int32_t n_annot, nldsc_ld_result* r, double* l2_annot, double* l2d_annot, char* err,
                             size_t errlen);

/* Library / device information. */
const char* nldsc_version(void);
int nldsc_device_count(void);

/* ---- engine API ------------------------------------------------------------------------ */
typedef struct nldsc_engine nldsc_engine;

int nldsc_engine_create(int32_t device, nldsc_engine** out, char* err, size_t errlen);
void nldsc_engine_destroy(nldsc_engine* e);

/* Engine options (no reference counterpart: the schedule and kernel choice of this engine; every setting gives the
 * same results, which the GPU tests compare).  Read at each run (orient: at each load); NLDSC_E_ARG for an unknown
 * name or a value out of range.  Defaults in brackets.
 *   band_mode    default correlation path when a run's flags name none: 0 fp32, 1 exact int8, [2] exact fp4
 *   gpu_plan     [1] band schedule on the GPU for sorted non-negative positions; 0 the host replay always
 *   plan_fused   [1] that schedule in one launch (items included) for slices of <= 32768 SNPs; 0 the kernel chain
 *   orient       [1] store rows minor-homozygote-as-00 at load (the exact kernels' operands mostly zero)
 *   ksplit       [1] K-split small launches (a rank's shard of one chromosome)
 *   t2           super-item kernels for missing-free blocks: 0 none, 1 2x2 routed, 2 2x2 for all, [3] 4x4 quad
 *   band_rounds  [1] single-block fp4 band in launches of one round of wave slots; 0 one launch
 *   f4_nc2       [1] additive-only fp4 items of two column blocks; 0 single block pairs
 *   f4_nc2_dom   [1] add+dom fp4 bands of long unsegmented rows (2^17 <= n_org < 2^19, GPU plan, band_rounds 1):
 *                pairs of neighbouring column blocks (32x64 tiles) at one wave per SIMD, in whole
 *                rounds of 4 items per CU from two such rounds on; the pairs past the last full round and the rows' odd
 *                blocks run as single block pairs (rounds of the single-block kernel, the partial last one K-split).
 *                With super-item routing the pairs and singles no super-item kernel takes whole are compacted first, and
 *                a pair runs with the one block the routing leaves it.
 *                0 single block pairs.  Plain runs only: annotated, pairs and covariate runs keep their batches
 *   colpair_round_items [0] tests: pair items per round of f4_nc2_dom (0: 4 per CU), then from one round on and on
 *                rows of any unsegmented length
 *   q_rounds     [1] quad super-items in launches of one workgroup per CU; 0 one launch
 *   defer_rep    [1] K loops of items holding a replayed rare variant in the main launch; 0 a later KC launch
 *   annot_batch_items [0] annotated runs: block-pair items per batch (0: what the Gram scratch cap holds)
 *   pairs_batch_items [0] pairs runs: the same
 *   pairs_max_cells   [0] pairs runs: cells of the dense count matrix a run may use (0: 2^27)
 *   cov_batch_items   [0] covariate runs: block-pair items per batch (0: what the Gram scratch cap holds)
 *   debug_timing [0] per-run stage timings on stderr */
int nldsc_engine_set_option(nldsc_engine* e, const char* name, int64_t value, char* err, size_t errlen);

/* Page-locked host memory mapped into every device's address space (hipHostMalloc), NULL on failure; free with
 * nldsc_host_free (which ignores pointers it did not hand out).  A host-result run whose seven result arrays (owned
 * slices) all lie in such buffers is written by the GPU directly — no landing buffer, no host copies — and positions
 * there are uploaded by DMA in place. */
void* nldsc_host_alloc(size_t bytes);
void nldsc_host_free(void* p);

/* Make a .bed image resident on the engine's device.  `bed` is the complete file content
 * (3 magic bytes + n_snp rows of ceil(n_org/4) bytes), in host memory (_host) or in device
 * memory of the engine's device (_device, e.g. a torch tensor's data pointer; copied).
 * The rows are stored at a 64-byte-aligned pitch (pitched copies; padding read as missing), the
 * layout every run reads in place. */
int nldsc_engine_load_bed_file(nldsc_engine* e, const char* path, int32_t n_snp, int32_t n_org,
                               char* err, size_t errlen);
int nldsc_engine_load_bed_host(nldsc_engine* e, const uint8_t* bed, size_t len, int32_t n_snp,
                               int32_t n_org, char* err, size_t errlen);
int nldsc_engine_load_bed_device(nldsc_engine* e, const void* bed, size_t len, int32_t n_snp,
                                 int32_t n_org, char* err, size_t errlen);

/* LD scores on a subset of the individuals (a reference panel inside a larger .bed: one ancestry group, unrelated,
 * QC-passed samples; PLINK's / LDSC's --keep).  The next loads (all four) keep only the individuals idx[0 .. n_keep):
 * 0-based .fam line numbers, strictly ascending, of a file of n_org_file individuals; the list is copied to the
 * device.  idx == NULL clears the list.  With a list: NLDSC_E_ARG unless 1 <= n_keep <= n_org_file and every entry
 * lies in [0, n_org_file) above the entry before it.  An image already resident is not affected.
 *   - An individual's identity is PLINK's: .fam line s is bit pair s % 4, low pairs first (bits 2(s%4)+1 : 2(s%4)), of
 *     byte s / 4 of every row, whatever sample order a run uses.
 *   - With a list set the loaders take n_org = n_org_file (another n_org: NLDSC_E_ARG) and run their magic / size
 *     checks against it; each slice of rows is compacted on the GPU to the .bed rows `plink --keep` would write (kept
 *     individual k at pair k % 4 of byte k / 4, the last byte's unused pairs 00) and loaded as an image of n_keep
 *     individuals.  Afterwards runs pass n_org = n_keep.
 *   - Runs on such an image always use PLINK's sample order, as if NLDSC_FLAG_STRICT_PLINK_ORDER were set: the
 *     reference's order would read the compact last byte's padding pairs as people at n_keep % 4 != 0, and the
 *     reference has no --keep to mirror.
 *   - A keep-load followed by a run equals, bit for bit in all seven result arrays, a plain load of the physically
 *     subsetted .bed run with NLDSC_FLAG_STRICT_PLINK_ORDER, in every band mode and with every engine option. */
int nldsc_engine_set_keep(nldsc_engine* e, const int32_t* idx, int32_t n_keep, int32_t n_org_file, char* err,
                          size_t errlen);
/* n_keep of the resident image when it was loaded with a keep list, 0 for a plain image. */
int nldsc_engine_kept(const nldsc_engine* e);

/* Compute LD scores for the SNPs with index in [own_begin, own_end) (position sharding:
 * each GPU owns a contiguous SNP range and recomputes the pairs it shares with its
 * neighbours' ranges, so no partial sums cross GPUs).  Entries of `r` outside the owned
 * range are left untouched.  p->bedfile is ignored (the loaded image is used).  `r`'s arrays
 * may be ordinary host memory or nldsc_host_alloc buffers (written by the GPU in place). */
int nldsc_engine_run(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                     nldsc_ld_result* r, char* err, size_t errlen);

/* Partitioned LD scores (stratified LD score regression; LDSC's --annot): nldsc_engine_run plus, for every
 * annotation column c of `annot`, L2[j, c] = a[j, c] + sum_k a[k, c] r2adj(j, k) over SNP j's window (the a[j, c]
 * is the self term, as the 1 of L2) and L2D[j, c] = sum_k a[k, c] r2adj_dominance(j, k) over the neighbours L2D
 * counts.  `annot`, `l2_annot` and `l2d_annot` are category-major [n_annot][p->n_snp] host arrays; entries outside
 * the owned range are left untouched.  `r` is filled exactly as nldsc_engine_run fills it, bit for bit.
 *   - l2_annot[c][j] is NaN exactly where r->l2[j] is, l2d_annot[c][j] exactly where r->l2d[j] is.  l2d_annot may be
 *     NULL with NLDSC_FLAG_ADDITIVE_ONLY; non-NULL with that flag it is filled with NaN.
 *   - The sums accumulate as 64-bit integers in units of 2^(-44 + e_c), e_c = max(0, ceil(log2(max_j |a[j, c]|))): a
 *     0/1 column has the resolution of L2 itself; what that rounding drops of each work item's partial sum goes to a
 *     second integer accumulator in units of 2^-40 of the first, so a total carries the fp64 partial sums' precision.
 *     Results do not depend on the schedule (engine options, batches, K-split) and are bit-reproducible.  Negative
 *     values are allowed.
 *   - NLDSC_E_ARG, with the reason in `err`, unless 1 <= n_annot <= NLDSC_MAX_ANNOT, every value of `annot` is
 *     finite, the run takes the exact fp4 path (NLDSC_FLAG_FP32 / NLDSC_FLAG_EXACT_I8, or option band_mode 0 / 1,
 *     are rejected) and n_org < 2^19.  Host results only: the device-table runs take no annotations.
 *   - The band goes in batches of single block-pair items (option annot_batch_items, 0 = as many as 1 GiB of Gram
 *     scratch holds), whatever the options t2, f4_nc2 and band_rounds say.  Stateless: the next run is a plain one. */
#define NLDSC_MAX_ANNOT 1024
int nldsc_engine_run_annot(nldsc_engine* e, const nldsc_ld_params* p, const double* annot, int32_t n_annot,
                           int32_t own_begin, int32_t own_end, nldsc_ld_result* r, double* l2_annot,
                           double* l2d_annot, char* err, size_t errlen);

/* The pairwise LD table behind the LD scores: nldsc_engine_run plus, for every owned computed SNP j, one entry per
 * neighbour k the run counts in l2_ws[j] — the ordered pairs (j, k) the pair epilogue adds to L2[j] — in CSR over the
 * owned range: row_ptr[own_end - own_begin + 1] (row j - own_begin is [row_ptr[..], row_ptr[.. + 1])), then k[] (the
 * neighbour's SNP index, ascending within a row), rv[] (the additive correlation r: the epilogue's fp64 dot product
 * times its hoisted 1 / n_org, so r2adj(r) = 1 - (1 - r r) (n_org - 1) / (n_org - 2) is the term of L2[j]) and rdv[]
 * (corr(A_j, R_k) likewise, the term of L2D[j]; NaN where k has no passing residual — the pair is not in l2d_ws[j] —
 * and with NLDSC_FLAG_ADDITIVE_ONLY).  SNPs that are not computed have empty rows.  `r` is filled exactly as
 * nldsc_engine_run fills it, bit for bit.
 *   - Signs are those of the file's allele coding (A counts A2 copies as the .bed stores them), whatever orientation
 *     the engine keeps a row in.
 *   - r(j, k) and r(k, j) are the same bits.  Inside one 32-SNP block the fp64 form is symmetric only to rounding:
 *     there the pair's entries both carry the value of the entry with j < k, so for j > k in one block r2adj(r) may
 *     differ from the term the run added to L2[j] in the last bits.
 *   - The table is bit-reproducible and does not depend on the schedule (engine options, batches, K-split): no
 *     position is decided by an atomic.  Non-finite values (windows poisoned by an all-missing SNP) are emitted as
 *     they are.
 *   - min_r2 (NaN: no filter) keeps an entry when r2adj(r) > min_r2 or r2adj(rd) > min_r2 (strict; non-finite values
 *     compare false and drop out).
 *   - Sizing: row_ptr and *n_pairs are always written.  When *n_pairs > cap, or k is NULL, nothing is emitted and the
 *     call returns NLDSC_E_SPACE with the needed count in `err`; `r` is written in that case too.  (An empty table
 *     is NLDSC_OK whatever the capacity.)
 *   - NLDSC_E_ARG, with the reason in `err`, unless the run takes the exact fp4 path and n_org < 2^19 (as an annotated
 *     run), and when own_n * Wb — Wb the widest window of the owned SNPs in 32-SNP blocks — exceeds 2^27 cells
 *     (option pairs_max_cells): narrow the owned range.  Host results only; annotations and pairs in one run are not
 *     supported.
 *   - The band goes in batches like an annotated run's (option pairs_batch_items): a count pass, a scan, and — when
 *     the table is emitted — an emit pass, which computes the Gram tiles again unless one batch held the whole band.
 *     Device memory: 4 bytes per cell and 20 bytes per pair.  Stateless: the next run is a plain one. */
int nldsc_engine_run_pairs(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                           nldsc_ld_result* r, double min_r2, int64_t* row_ptr, int32_t* k, double* rv,
                           double* rdv, int64_t cap, int64_t* n_pairs, char* err, size_t errlen);

/* Covariate-adjusted LD scores (cov-LDSC, Luo et al., Hum. Mol. Genet. 2021, here also for the dominance scores):
 * nldsc_engine_run with every genotype vector residualised on the run's covariates before the correlations, for LD
 * scores that match summary statistics computed with those covariates (principal components, sex, age) in the model.
 * q_basis is category-major [n_covar][p->n_org] host memory: an orthonormal basis Q of the centred covariates' column
 * space (the caller drops constant and dependent columns; the engine takes Q, not the covariates), row i = .fam line
 * i of the image's individuals (the kept ones, in order, for an image loaded with a keep list).
 *   - With A_j, R_j SNP j's standardised additive and dominance-residual vectors (0 at missing calls), U_j = Q^T A_j,
 *     W_j = Q^T R_j, v_j = 1 - |U_j|^2 / N:  A~_j = (A_j - Q U_j) / sqrt(v_j);  R~_j = the standardised residual of
 *     the dominance coding on the intercept, A_j and the covariates: (R_j - Q W_j - g_j (A_j - Q U_j)) / sqrt(w_j),
 *     g_j = -(W_j . U_j) / (N v_j), w_j = 1 - |W_j|^2 / N - g_j^2 v_j.  L2[j] = 1 + sum_k r2adj(A~_j . A~_k / N),
 *     L2D[j] = sum_k r2adj(A~_j . R~_k / N) over the neighbour sets of the plain run, r2adj(r) = 1 - (1 - r^2)
 *     (n' - 1) / (n' - 2) with n' = N - n_covar.
 *   - maf, l2_ws and the windows are the plain run's, bit for bit.  residuals_std[j] is rstd_j sqrt(w_j), the std of
 *     the residual of the model with covariates; l2d_ws / l2d_wse membership (std > std_thr) is taken on it.
 *   - v_j < 1e-6 (the additive coding is, to rounding, a linear function of the covariates): A~_j := 0, every r with
 *     it is 0, the SNP stays computed.  w_j < 1e-6: R~_j := 0 and residual std 0.  NaN patterns are the plain run's.
 *   - The run implies NLDSC_FLAG_EXACT_RARE (closed-form vectors of rare variants: the reference has no such model
 *     whose fp32 rounding could be replayed).  Results do not depend on the schedule (engine options, batches,
 *     K-split, owned ranges) and are bit-reproducible.
 *   - NLDSC_E_ARG, with the reason in `err`, unless 1 <= n_covar <= NLDSC_MAX_COVAR and n_covar <= n_org - 3; every
 *     value of q_basis is finite, its Gram matrix is within 1e-8 of the identity and its column sums within
 *     1e-8 sqrt(n_org) of 0; the run takes the exact fp4 path with n_org < 2^19 (as an annotated run) in PLINK's sample
 *     order (NLDSC_FLAG_STRICT_PLINK_ORDER, or an image of kept samples).  Host results only: the device-table and split
 *     runs take no covariates, and covariates with annotations or a pair table in one run are not supported.
 *   - The projections go first (one pass over the resident image on the fp64 matrix cores, part of the statistics
 *     stage's time), then the band in batches like an annotated run's (option cov_batch_items).  Stateless: the next
 *     run is a plain one. */
#define NLDSC_MAX_COVAR 64
int nldsc_engine_run_covar(nldsc_engine* e, const nldsc_ld_params* p, const double* q_basis, int32_t n_covar,
                           int32_t own_begin, int32_t own_end, nldsc_ld_result* r, char* err, size_t errlen);
/* One-shot: read `p->bedfile`, on the individuals keep_idx[n_keep] when keep_idx != NULL (nldsc_ld_calculate_keep;
 * q_basis then has n_keep rows), in PLINK's sample order. */
int nldsc_ld_calculate_covar(const nldsc_ld_params* p, const int32_t* keep_idx, int32_t n_keep, const double* q_basis,
                             int32_t n_covar, nldsc_ld_result* r, char* err, size_t errlen);
/* Dominance-by-dominance LD scores (d-LDSC): nldsc_engine_run plus
 *   l2dd[j] = 1 + sum over k of r2adj(R_j . R_k / n_org)
 * with R the standardised dominance residual the run already forms for L2D (orthogonal to the additive coding).  The
 * pair (j, k) counts exactly when it counts towards l2d_ws[j] (k in j's window and pointers, k passed MAF,
 * rstd_k > std_thr) and j itself has rstd_j > std_thr; the self term 1 follows l2's; r2adj and n_org are l2d's.  l2dd[j]
 * is NaN where l2[j] is NaN and where rstd_j <= std_thr (R_j is undefined).  Its neighbour count is l2d_ws[j]: no new
 * count array.  l2dd: [n_snp] host array; the owned slice is written.
 *   - The run implies NLDSC_FLAG_EXACT_RARE (closed-form vectors of rare variants: the new statistic has no reference
 *     arithmetic to replay), so the seven ordinary arrays equal, bit for bit, those of a plain run with that flag,
 *     and on data without replayed SNPs those of a default plain run.
 *   - Every block pair goes through the K-split partial kernel with a ninth exact product (h . h), then through an
 *     epilogue that adds the ordinary sums and the new one; the per-SNP sums are fixed-point, so l2dd is
 *     bit-reproducible and does not depend on the schedule (batches: option annot_batch_items; K-split; owned ranges).
 *   - NLDSC_E_ARG, with the reason in `err`: n_org >= 2^19 (the partial kernel takes unsegmented rows); a run that
 *     does not take the exact fp4 path; NLDSC_FLAG_ADDITIVE_ONLY (no dominance residuals); l2dd NULL.  Host results
 *     only; annotations, a pair table or covariates go in runs of their own.  Stateless: the next run is a plain one. */
int nldsc_engine_run_domdom(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                            nldsc_ld_result* r, double* l2dd, char* err, size_t errlen);
/* One-shot: read `p->bedfile`, on the individuals keep_idx[n_keep] when keep_idx != NULL (nldsc_ld_calculate_keep). */
int nldsc_ld_calculate_domdom(const nldsc_ld_params* p, const int32_t* keep_idx, int32_t n_keep, nldsc_ld_result* r,
                              double* l2dd, char* err, size_t errlen);
/* The projections of the last covariate run, for tests and tools: u, w [n_covar][n_snp] (U_j in the file's allele
 * coding, W_j), v, wd [n_snp] (v_j, w_j; 1 for SNPs that are not computed or have every call missing, whose U and W
 * are 0).  Any pointer may be NULL.  NLDSC_E_ARG when the engine's last covariate run did not complete. */
int nldsc_engine_covar_projections(nldsc_engine* e, double* u, double* w, double* v, double* wd);

/* nldsc_engine_run with the owned slice of the result left in device memory (the multi-GPU gather of
 * SURVEY.md §8 e1 then runs device to device over RCCL, without a host round trip): `table_dev`, device memory
 * of the engine's device holding 7 * width doubles with width >= own_end - own_begin, receives row k =
 * l2, l2d, maf, residuals_std, l2_ws, l2d_ws, l2d_wse (LDScoreResult, data.h:21-31; window sizes as doubles),
 * column c = SNP own_begin + c, columns past the owned range NaN.  Returns once the table is written (the
 * engine stream is synchronised), so any stream may read it. */
int nldsc_engine_run_device(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                            double* table_dev, int32_t width, char* err, size_t errlen);

/* nldsc_engine_run_device in two calls, computing each pair that straddles two ranks' owned ranges once (multi-GPU
 * strong scaling; no reference counterpart: the reference is single-process, ldscalc.h:34-35).  The loaded slice
 * holds the owned SNPs [own_begin, own_end) and the right halo [own_end, n_snp) (one window, no left halo).
 * _split computes the pairs whose lower SNP is owned, accumulates the per-SNP sums of every SNP of the slice, and
 * writes the right halo's accumulators (exact fixed-point sums and counts) to `export_dev`: device memory of
 * 6 * export_cap int64 (row-major [6][export_n], export_n = n_snp - own_end <= export_cap), synchronised on return.
 * The caller sends that block to the rank owning those SNPs (whose slice starts at them) and passes the block
 * received from the left neighbour to _finish, which adds it to the first import_n owned SNPs (import_n <=
 * own_end - own_begin; 0 for the first rank), finalizes and writes `table_dev` as nldsc_engine_run_device does.  Counts,
 * MAF and residual std equal those of nldsc_engine_run_device with the left halo loaded; L2 / L2D to the last bits
 * (the exchanged sums are exact integers; each work item's fp64 partial sums follow the slice's block grid). */
int nldsc_engine_run_device_split(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                                  double* table_dev, int32_t width, int64_t* export_dev, int32_t export_cap,
                                  int32_t* export_n, char* err, size_t errlen);
int nldsc_engine_run_device_finish(nldsc_engine* e, const int64_t* import_dev, int32_t import_n, char* err,
                                   size_t errlen);

/* Per-stage device timings (milliseconds, HIP events on the engine stream) of the last run:
 * [0] genotype count, [1] per-SNP statistics, [2] window replay + schedule (host time; overlaps [0]),
 * [3] band correlation kernel (all launches), [4] finalize, [5] total.
 * Also: algorithmic FLOPs (2N(1/2 sum WSA + sum WSD)), FLOPs issued to the matrix cores by the
 * band kernels (counted on the GPU per work item as each kernel decides them: the products of missing-free blocks
 * and the transposed products of diagonal blocks that are skipped are not counted; padded sample slots are), SNP
 * pairs (sum WSA) of the last run, and the band kernel's work-item count (block pairs, also when column-block pair
 * items ran).  With f4_nc2_dom the count is that of the single-block plan, so it does not depend on the option: a
 * pair item whose two column blocks differ in missingness runs the loop of their union and issues the missing-call
 * products for the missing-free block as well (on all-zero operands), which the count leaves out. */
int nldsc_engine_timings(const nldsc_engine* e, double* ms6, double* flop_alg, double* flop_issued,
                         double* pairs, int32_t* n_band_items);
/* Path of the last run: 2 = exact Gram on fp4 MFMAs, 1 = exact Gram on int8 MFMAs, 0 = fp32;
 * *ops_alg_i8 = algorithmic ops of the exact formulation, 2N (2 sum WSA + 2 sum WSD). */
int nldsc_engine_path(const nldsc_engine* e, int32_t* exact_i8, double* ops_alg_i8);
/* K-split factor of the last run's fp4 band kernel: the number of K pieces each work item was split into
 * (1 = single pass; > 1 for launches too small to fill the GPU, e.g. one rank's shard of a chromosome). */
int nldsc_engine_ksplit(const nldsc_engine* e);
/* Band launch rounds of the last run: the number of work items per launch of the single-block fp4 band kernel when
 * its items went in launches of one round of the GPU's wave slots each (so the items of a launch stay at nearby K
 * offsets and share their strips through L2), 0 when they went in one launch. */
int nldsc_engine_band_round_items(const nldsc_engine* e);
/* K-split factor of the last run's partial last round when its band went in round launches (1: not split). */
int nldsc_engine_band_tail_ksplit(const nldsc_engine* e);
/* Band kernel of the last run: NLDSC_BAND_F32 (fp32 MFMA GEMM), NLDSC_BAND_I8, NLDSC_BAND_F4 (one wave per
 * 32x32 block pair), NLDSC_BAND_F4_SEG (rows above 2^19 samples), NLDSC_BAND_F4_KSPLIT, NLDSC_BAND_F4_2X2
 * (4-wave workgroups over 2x2 block pairs sharing their strips through LDS), NLDSC_BAND_F4_ROUTED (missing-free
 * 2x2 super-items in the 2x2 workgroups, the rest in the single-block kernel), NLDSC_BAND_F4_QUAD (the default for
 * sorted non-negative positions: missing-free 4x4 super-items in the quad workgroups, the rest in the single-block
 * kernel).  All exact paths give bitwise the same results. */
#define NLDSC_BAND_F32 0
#define NLDSC_BAND_I8 1
#define NLDSC_BAND_F4 2
#define NLDSC_BAND_F4_SEG 3
#define NLDSC_BAND_F4_KSPLIT 4
#define NLDSC_BAND_F4_2X2 5
#define NLDSC_BAND_F4_ROUTED 6
#define NLDSC_BAND_F4_QUAD 7 /* option t2 = 3: missing-free 4x4 super-items in the quad workgroups (64x64 tiles per
                                wave), the rest in the single-block kernel */
#define NLDSC_BAND_F4_COLPAIR 8 /* option f4_nc2_dom: add+dom bands of long rows, pairs of neighbouring column blocks
                                   (32x64 tiles) at one wave per SIMD in whole rounds, the rest in the single-block
                                   kernel; nldsc_engine_band_round_items then counts the block pairs of a pair
                                   round (two per pair item: 8 per CU), the unit of the work-item count */
int nldsc_engine_band_kernel(const nldsc_engine* e);
/* The column-pair rounds of the last run (NLDSC_BAND_F4_COLPAIR; all zero when no pair round ran): out[0] the pair
 * items launched as pairs (whole rounds), out[1] the pairs the plan emitted (under super-item routing: those that keep
 * a block after the compaction), out[2] the single-block items of the rest of the band (the odd runs' leftover singles
 * and two for every pair past the last whole round; under routing before the kernel drops the routed ones of the
 * latter).  Returns NLDSC_OK, or NLDSC_E_ARG for a NULL argument. */
int nldsc_engine_band_pair_items(const nldsc_engine* e, int32_t out[3]);
/* Where the last host-result run (nldsc_engine_run) wrote its owned slice: 1 straight into the caller's arrays (all
 * seven in nldsc_host_alloc buffers, zero copy), 0 through the engine's landing buffer and host copies, -1 no host
 * result written (device-table runs, empty owned ranges). */
int nldsc_engine_result_direct(const nldsc_engine* e);

/* Load SNP rows [snp_begin, snp_end) of a .bed file of n_snp_file SNPs as the engine's image
 * (snp_end - snp_begin SNPs; the run then takes the positions of that slice).  Position sharding
 * (SURVEY.md §8 e1): each GPU reads only its owned range plus the window halo around it.
 * Same magic / size checks and messages as nldsc_engine_load_bed_file. */
int nldsc_engine_load_bed_file_range(nldsc_engine* e, const char* path, int32_t n_snp_file, int32_t n_org,
                                     int32_t snp_begin, int32_t snp_end, char* err, size_t errlen);

/* Host-only plan of the band kernel (no GPU needed; the engine calls the same code):
 * replays the reference's sliding-window pointers (stream.h:131-155,182-197) from positions and
 * MAF-pass flags (flags[j] bit 0) into L/R (n_snp each; L = -1 for SNPs the reference does not
 * compute) and lists the work items (I, J0, nc, 0) covering every needed 32x32 block pair for the
 * owned range (max_nc 1 or 2; any other value is an argument error).  Returns the item count; when it
 * exceeds `cap` (or items == NULL) nothing is written to `items` and the count is returned; < 0 on bad
 * arguments. */
int nldsc_plan_band(const double* positions, const uint8_t* flags, int32_t n_snp, double ld_wind, int32_t own_begin,
                    int32_t own_end, int32_t max_nc, int32_t* L, int32_t* R, int32_t* items, int32_t cap);

/* Host-only arithmetic of annotated runs (no GPU needed; the engine calls the same code).  _scale_exp: e_c of a
 * column whose largest |a| is max_abs (0 for max_abs <= 1).  _plan_batches: the batches of a band of n_items items of
 * n_it K-loop chunks on n_cu CUs, batches[3 k ..] = (first item, items, K-split pieces); batch_items as the engine
 * option annot_batch_items.  Returns the batch count; when it exceeds `cap` (or batches == NULL) nothing is
 * written; < 0 on bad arguments. */
int nldsc_annot_scale_exp(double max_abs);
int nldsc_annot_plan_batches(int32_t n_items, int32_t n_it, int32_t n_cu, int32_t ksplit_ok, int32_t batch_items,
                             int32_t* batches, int32_t cap);
/* The same for units (one K piece of one item) of unit_floats floats of Gram scratch under a cap of cap_bytes (0: the
 * engine's 1 GiB): 8192 for the runs above, 9216 for a dom-dom run's nine tiles.  Every batch keeps
 * items * pieces * unit_floats * 4 <= cap_bytes (a single item's pieces excepted: a batch holds one item at least). */
int nldsc_plan_batches_unit(int32_t n_items, int32_t n_it, int32_t n_cu, int32_t ksplit_ok, int32_t batch_items,
                            int64_t cap_bytes, int32_t unit_floats, int32_t* batches, int32_t cap);

/* Host-only arithmetic of pairs runs (no GPU needed; the engine and its kernels use the same code).  _cell: the cell
 * of the dense count matrix that holds owned SNP g's entries against 32-SNP block nb, (g - own_begin) * wb +
 * (nb - L_g / 32), or -1 (g outside the owned range, L_g < 0, nb outside the wb blocks from L_g's on).
 * _window_blocks: wb of an owned range from the pointers L, R (n_snp each): max over computed SNPs of R / 32 - L / 32
 * + 1, at least 1.  _split_ranges: owned ranges of at most `budget` pairs from the row_ptr[n + 1] of a sizing call,
 * ends[k] = end of range k (the ranges tile [0, n); a single row above the budget is a range of its own); returns
 * the range count; when it exceeds `cap` (or ends == NULL) nothing is written; < 0 on bad arguments. */
int64_t nldsc_pairs_cell(int32_t g, int32_t nb, int32_t own_begin, int32_t own_end, int32_t L_g, int32_t wb);
int nldsc_pairs_window_blocks(const int32_t* L, const int32_t* R, int32_t n_snp, int32_t own_begin, int32_t own_end);
int nldsc_pairs_split_ranges(const int64_t* row_ptr, int32_t n, int64_t budget, int32_t* ends, int32_t cap);

/* The score table as the reference writes it (make_output + DataFrame.to_csv(sep="\t", index=False,
 * float_format="%.5f"), nldsc/ldscore/routine.py:94-101), without the header line: row i = prefix line i
 * (the caller's "CHR\tSNP\tBP" text, lines separated by '\n'), then L2, L2D [, MAF, WSA, WSD, WSDE,
 * RSTD when extra]; floats "%.5f", NaN as an empty field.  Host-only, no GPU.  Returns the bytes
 * written to `out`, or NLDSC_E_OOM when `cap` is too small, NLDSC_E_ARG on bad arguments. */
int64_t nldsc_format_scores(const char* prefix, int64_t prefix_len, int32_t n, const double* l2, const double* l2d,
                            const double* maf, const int32_t* l2_ws, const int32_t* l2d_ws, const int32_t* l2d_wse,
                            const double* rstd, int32_t extra, char* out, int64_t cap);

/* Deterministic synthetic PLINK .bed on the device (benchmarks / full-size tests):
 * writes the complete file image (magic + rows) to `bed_dev` (len >= 3 + n_snp*ceil(n_org/4)).
 * Model as nldsc_amd/synth.py: latent AR(1) haplotypes, thr[j] = Phi^-1(p_j), `missing` rate. */
int nldsc_synth_bed_device(int32_t device, void* bed_dev, int32_t n_snp, int32_t n_org,
                           const float* thr_host, float rho, float missing, uint64_t seed,
                           char* err, size_t errlen);

#ifdef __cplusplus
}
#endif
#endif /* NLDSC_LD_H */
