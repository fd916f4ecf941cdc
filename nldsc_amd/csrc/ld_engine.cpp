// ld_engine.cpp — host side of libnldsc_amd.so: the C ABI declared in include/nldsc_ld.h.
//
// One engine = one HIP device + one stream + device buffers that persist across runs.
// A run (nldsc_engine_run) is the whole hot path of bayarpark/nldsc's `calculate`
// (nldsc/ldscore/_ldscore/ldscalc.h:8-65) over a .bed image already resident in HBM:
//   count (resident rows, kept at an aligned pitch by the loaders) -> per-SNP statistics ->
//   window replay + tile schedule (host, O(M), overlapping the count) ->
//   band correlation kernels -> finalize -> results to host.
#include <hip/hip_runtime.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <immintrin.h>

#include "../../include/nldsc_ld.h"
#include "band_plan.h"
#include "ld_kernels.h"

#define NLDSC_VERSION "0.1.0"

namespace {

constexpr int BLK = 32;             // SNPs per MFMA block
constexpr int CHUNK_BYTES = 32;     // one K-loop chunk of a 2-bit row (16 B per lane half)
constexpr int kLoadThreads = 8;     // .bed file loads: reader threads (pread + H2D + placement per slice)
constexpr int kCopyThreads = 3;     // host result copies: helper threads beside the calling one
// resident row pitch: an even number of 32-byte chunks (the fp4 K loop takes two per iteration)
constexpr int ROW_ALIGN_BYTES = 64;
// item order of the single-block-pair schedule: tiles of TILE_R row blocks x TILE_C diagonal offsets
constexpr int TILE_R = 16, TILE_C = 16;

// resident layout of a .bed image: rows of ceil(N/4) bytes padded to row_bytes, n_rows = M rounded up to 32, the rows of
// each 32-SNP block interleaved in 32-byte chunks (ld_kernels.hip tile_off)
int row_pitch(int32_t n_org) {
    const int nb = n_org / 4 + (n_org % 4 > 0);
    return (nb + ROW_ALIGN_BYTES - 1) / ROW_ALIGN_BYTES * ROW_ALIGN_BYTES;
}
int padded_rows(int32_t n_snp) { return (n_snp + BLK - 1) / BLK * BLK; }

// Message of BedStreamReader::check_plink_magic_number (stream.h:88-102), verbatim.
const char* kBadMagic =
    "Invalid PLINK magic number in BED file.The file is incorrect, or it was created using an incompatible "
    "version of PLINK.";

int set_err(char* err, size_t errlen, int code, const char* fmt, ...) {
    if (err && errlen) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, errlen, fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return set_err(err, errlen, NLDSC_E_HIP, "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), \
                           __FILE__, __LINE__, #expr);                                                \
    } while (0)

// device buffer, freed with its owner (an engine's: on the engine's device, ~nldsc_engine)
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t want) {
        if (want <= n && p) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc(&p, std::max<size_t>(want, 1) * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// page-locked host buffer (async H2D copies out of it do not block the calling thread)
struct HostPinned {
    uint8_t* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t want) {
        if (want <= n) return hipSuccess;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipHostMalloc((void**)&p, std::max<size_t>(want, 1));
        if (e == hipSuccess) n = want;
        return e;
    }
    ~HostPinned() {
        if (p) (void)hipHostFree(p);
    }
};

// Host work of a run split over the calling thread and kCopyThreads helpers, which sleep on a condition variable
// between runs: the copies of its results (pinned landing buffer -> the caller's arrays, 3.5 MB at M = 80 000: ~0.33 ms
// on one core; below kMinParallel bytes the caller copies alone, a wake-up costs more) and of its positions, and the
// schedule's window edges.
class CopyPool {
  public:
    struct Seg {
        void* dst;
        const void* src;
        size_t n;
    };
    static constexpr size_t kMinParallel = 256 << 10;
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void copy(const Seg* segs, int nseg) {
        size_t total = 0;
        for (int k = 0; k < nseg; ++k) total += segs[k].n;
        if (total < kMinParallel) {
            for (int k = 0; k < nseg; ++k) std::memcpy(segs[k].dst, segs[k].src, segs[k].n);
            return;
        }
        // part p: bytes [total * p / parts, total * (p + 1) / parts) of the segments laid end to end
        parallel([&](int p, int parts) {
            const size_t lo = total * p / parts, hi = total * (p + 1) / parts;
            size_t base = 0;
            for (int k = 0; k < nseg && base < hi; base += segs[k].n, ++k) {
                const size_t a = std::max(lo, base), b = std::min(hi, base + segs[k].n);
                if (a < b)
                    std::memcpy(static_cast<uint8_t*>(segs[k].dst) + (a - base),
                                static_cast<const uint8_t*>(segs[k].src) + (a - base), b - a);
            }
        });
    }
    // f(part, parts) for part = 0 .. parts - 1 (parts = kCopyThreads + 1), part 0 on the calling thread.  Helper
    // threads start on first use; if the system refuses a thread, every part runs on the calling thread from then on
    // (a std::system_error must not cross the C ABI: ADVICE r04)
    void parallel(const std::function<void(int, int)>& f) {
        if (th_.empty() && !serial_) {
            try {
                for (int t = 0; t < kCopyThreads; ++t) th_.emplace_back([this, t] { loop(t + 1); });
            } catch (const std::exception&) {
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    stop_ = true;
                }
                cv_.notify_all();
                for (auto& t : th_) t.join();
                th_.clear();
                stop_ = false;
                serial_ = true;
            }
        }
        if (serial_) {
            for (int p = 0; p <= kCopyThreads; ++p) f(p, kCopyThreads + 1);
            return;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            pending_ = kCopyThreads;
            ++gen_;
        }
        cv_.notify_all();
        f(0, kCopyThreads + 1);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
    }

  private:
    void loop(int idx) {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            const std::function<void(int, int)>* f = job_;
            lk.unlock();
            (*f)(idx, kCopyThreads + 1);
            lk.lock();
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int, int)>* job_ = nullptr;
    int pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
    bool serial_ = false;
};

// Spin on a pinned word the GPU writes (a blocking event wait wakes the thread tens of microseconds late: the host waits
// on the critical path of short runs), with a CPU pause per poll, for at most ~1 ms — then the caller's blocking event
// wait takes over (a stalled plan no longer burns 2 s of a core that loaders and RCCL proxies share).
bool spin_until_nonneg(volatile const int* w) {
    const auto t0 = std::chrono::steady_clock::now();
    while (*w < 0) {
        _mm_pause();
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1000)) return false;
    }
    return true;
}

// Pinned host buffers handed out by nldsc_host_alloc: a run whose result arrays (or positions) lie inside one is
// written (read) by the GPU directly, without the engine's own landing buffer and host copies.
std::mutex g_host_mu;
std::map<uintptr_t, size_t> g_host_bufs;  // start -> bytes

// device pointer of [p, p + bytes) when it lies inside one nldsc_host_alloc buffer, else nullptr
void* registered_device_ptr(const void* p, size_t bytes) {
    if (!p) return nullptr;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    uintptr_t base = 0;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_bufs.upper_bound(a);
        if (it == g_host_bufs.begin()) return nullptr;
        --it;
        if (a + bytes > it->first + it->second) return nullptr;
        base = it->first;
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, reinterpret_cast<void*>(base), 0) != hipSuccess || !d) return nullptr;
    return static_cast<uint8_t*>(d) + (a - base);
}

}  // namespace

struct nldsc_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t plan_stream = nullptr;  // the GPU schedule runs here, beside the count kernel
    hipEvent_t ev_pos = nullptr;        // positions uploaded and their window edges searched (the schedule's input)
    hipEvent_t ev[6] = {};
    hipEvent_t ev_dbg[2] = {};  // option debug_timing: after the super-item launch, before the single-block launches
    bool debug_timing = false;
    hipEvent_t ev_plan = nullptr;  // GPU plan counters landed in h_meta
    hipEvent_t ev_stats = nullptr;   // SNP constants and replay flags written (the replay's inputs)
    hipEvent_t ev_replay = nullptr;  // replayed constants written (the KC launch and finalize wait on it)
    // side stream: the rare-variant replay beside the band (ev_replay), then the issued-product count (ev_issued)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_issued = nullptr;
    // resident .bed image
    DevBuf<uint8_t> bed;      // resident rows, block-interleaved (ld_kernels.hip tile_off)
    DevBuf<uint8_t> stage_dev;  // loads: rows of the .bed layout on their way into `bed` (released after the load)
    DevBuf<uint8_t> lastb;  // each row's original last byte (the per-run count kernel masks a copy of it)
    DevBuf<uint8_t> flip;   // per SNP: resident row stores the swapped (00 <-> 11) coding
    DevBuf<uint8_t> row_miss;  // per SNP: bit 0 / 1 = a missing call among the reference's / PLINK's individual slots
    DevBuf<uint32_t> miss_flags;  // (the load kernels' per-row word of the same flags)
    DevBuf<int> lcounts;          // per row: genotype counts of its stored bytes [0, nb - 1), load_parts parts
    bool orient = true;     // store rows minor-homozygote-as-00 at load (option "orient" 0: file coding)
    bool oriented = false;  // the resident image was oriented
    int32_t n_snp = 0, n_org = 0;
    // loads on a subset of the individuals (nldsc_engine_set_keep): the kept samples' .fam line numbers on the device,
    // their count and the file's individual count for the next loads; `kept`: the resident image holds that many kept
    // samples of a larger file (0: a plain image) — its runs use PLINK's sample order
    DevBuf<int32_t> keep_idx;
    int32_t keep_n = 0, keep_n_file = 0, kept = 0;
    // work buffers

    DevBuf<int> counts, cparts, Lw, Rw, Aw, ws_acc;  // (cparts: the count kernel's per-part counts)
    // the per-SNP results, one allocation: L2, L2D, MAF, RSTD (fp64) then WSA, WSD, WSDE (int32), each M long, so the
    // owned slices come back in two strided copies (one when a run owns every SNP)
    DevBuf<double> res;
    template <class T>
    struct View {
        T* p = nullptr;
    };
    View<double> l2, l2d, maf, rstd;
    View<int> ws3;
    DevBuf<float2> lut;
    DevBuf<nldsc::SnpConst> cst;
    DevBuf<uint8_t> sflags;
    DevBuf<uint8_t> blk_rep;  // per 32-SNP block: holds a rare variant with replayed fp32 vectors (KC items)
    DevBuf<float> gram;       // K-split partial Gram tiles
    // rare-variant items of the single-block fp4 kernel, deferred: their Gram tiles (8192 floats per block pair), the
    // block pairs, the slot counter (launch_band_f4 rep_gram; option "defer_rep" 0: the separate KC launch instead)
    DevBuf<float> rep_gram;
    DevBuf<int4> rep_items;
    DevBuf<int> rep_count;
    bool defer_rep = true;
    // annotated runs (nldsc_engine_run_annot): the annotation matrix, its per-column scales 2^(44 - e_c) and the
    // per-annotation accumulators (l2c_acc | residual limb, l2dc_acc likewise: [2][n_annot][M] each), category-major;
    // the finalized owned slice on its way to the host;
    // option "annot_batch_items" (0: what nldsc::ANNOT_GRAM_CAP_BYTES of Gram scratch holds)
    DevBuf<double> annot_dev, annot_scale, l2c_acc, l2dc_acc, annot_out;
    int annot_batch_items = 0;
    // pairs runs (nldsc_engine_run_pairs): the dense count matrix [own_n][Wb] (+ one int: Wb as the device found it),
    // the row lengths, the table's row_ptr and its k / r | rd on their way to the host; options "pairs_batch_items"
    // (as annot_batch_items) and "pairs_max_cells" (0: nldsc::PAIRS_MAX_CELLS)
    DevBuf<int> pairs_cnt, pairs_len, pairs_k;
    DevBuf<long long> pairs_ptr;
    DevBuf<double> pairs_val;
    std::vector<int> h_pairs_len;
    int pairs_batch_items = 0;
    int64_t pairs_max_cells = 0;
    // covariate runs (nldsc_engine_run_covar): the basis as the projection kernel reads it (ld_kernels.h CovArgs qt,
    // built in h_qt), the projection's plane sums, then U | W | W' ([3][n_covar][M]) and isv, gamma, isw, v, w
    // ([5][M]); option "cov_batch_items" (as annot_batch_items); cov_n / cov_M: the covariates and SNPs of the last
    // covariate run (nldsc_engine_covar_projections; 0: none yet)
    DevBuf<double> cov_qt, cov_part, cov_uw, cov_sc;
    std::vector<double> h_qt;
    int cov_batch_items = 0;
    int cov_n = 0, cov_M = 0;
    // dom-dom runs (nldsc_engine_run_domdom): the fixed-point sums of r2adj(R_j . R_k) ([M]) and the finalized owned
    // slice on its way to the host; their batches follow option "annot_batch_items"
    DevBuf<double> l2dd_acc, l2dd_out;
    // the device table of a run (finish_table's input), kept for a split run between its two calls
    // (nldsc_engine_run_device_split / _finish: `pending`)
    struct SplitState {
        bool pending = false;
        int32_t M = 0, N = 0, row_bytes = 0, width = 0;
        int32_t own_lo = 0, own_hi = 0;
        bool dom = true;
        double* table = nullptr;
        double ms1 = 0.0;  // the first call's host time
    } split;
    bool ksplit_ok = true;    // option "ksplit" 0 disables the K-split
    // deferred rare-variant Gram tiles: at most this many block-pair slots (32 KiB each: 2 GiB)
    size_t rep_gram_max_slots = (size_t)1 << 16;
    int last_ksplit = 1;
    int last_round_items = 0;
    // nldsc_engine_band_pair_items: pair items launched as pairs, pairs the plan emitted, single-block items of the rest
    int last_pair_items[3] = {0, 0, 0};
    int last_direct = -1;  // nldsc_engine_result_direct
    int last_tail_ksplit = 1;
    // fp4 band kernels on the GPU plan (option "t2"): 3 (default) missing-free 4 x 4 super-items in the quad
    // workgroups (64 x 64 tiles per wave), the rest in the single-block kernel (C5 slice band -25 % against 1, the
    // others unchanged: profiles/r03_ab_t2_quad.json); 1 the same with missing-free 2 x 2 super-items in the 2 x 2
    // block-pair workgroups; 2 everything in the 2 x 2 workgroups; 0 single-block only
    int t2_mode = 3;
    // additive-only fp4 band in 32 x 64 tiles (column-block pair items, the row strip decoded once for two column
    // blocks; option "f4_nc2" 0 turns it off): C2 band 2.85 -> 2.78 ms, one engine per process (r03_c2_nc2.json)
    bool f4_nc2 = true;
    // add+dom fp4 band of long unsegmented rows in 32 x 64 tiles at one wave per SIMD (column-block pair items in
    // rounds of 4 per CU, nldsc::shape_colpair; option "f4_nc2_dom" 0 turns it off), the rest of the band in the
    // single-block kernel.  colpair_round_items (option, tests): pairs per round, also on short rows
    bool f4_nc2_dom = true;
    int colpair_round_items = 0;
    DevBuf<int4> items_p, items_s;   // the column-pair plan: pairs; leftover singles, then the last pairs' blocks
    DevBuf<int4> items_pu, items_su; // routed runs: the same lists without the items the super-item kernel takes whole
    DevBuf<int> compact_tmp2;        // (their chunk counts and totals; the totals land in h_meta[10..11])
    DevBuf<int> plan_counts_p, plan_counts_s;
    // single-block fp4 band in launches of one round of wave slots (option "band_rounds" 0: one launch)
    bool band_rounds = true;
    DevBuf<uint8_t> blk_miss;
    // quad super-items in launches of one workgroup per CU when there are at least 16 such rounds (option "q_rounds" 0:
    // one launch): the workgroups on an XCD then stream their shared strips at nearby K offsets; C5 slice band
    // 351 -> 333 ms, C3 missing-free (6 rounds, below the threshold) 12.34 -> 12.51 ms (profiles/r03_ab_q_rounds.json)
    bool q_rounds = true;
    int last_band_kernel = NLDSC_BAND_F4;
    // 32-SNP blocks without a missing call among the individual slots of sample order o (row_miss, at load): the
    // super-item kernels take only missing-free blocks, so with none the run skips their plan, routing and launches
    int free_blocks[2] = {0, 0};
    DevBuf<double> pos, l2_acc, l2d_acc;
    DevBuf<int4> items;
    // host scratch
    std::vector<uint8_t> h_flags, h_all_pass;
    std::vector<int> h_L, h_R;
    std::vector<nldsc::PlanItem> h_items, h_scratch;
    HostPinned h_stage;  // pinned upload staging of the plan (L, R, items)
    HostPinned h_meta;   // GPU plan counters (items, diagonal items)
    HostPinned h_pos;    // pinned copy of the positions (the upload does not stall this thread)
    HostPinned h_res;    // pinned landing buffer of host-result runs (the GPU writes it, then host copies out)
    CopyPool copies;     // the host copies out of h_res, split over threads
    // [0..1] device-table runs: sums of the positive WSA / WSD over the owned slice; [2] MFMA products issued
    DevBuf<unsigned long long> sums;
    HostPinned h_sums;
    DevBuf<int> plan_counts, plan_meta, plan_counts2;
    DevBuf<int2> plan_rows, plan_rows2;
    DevBuf<int4> items2;  // super-items of the 2 x 2 / quad kernel
    DevBuf<int4> items_u;  // routed runs: the single-block items no super-item kernel takes (compacted)
    DevBuf<int> compact_tmp;
    HostPinned h_route;    // their count
    hipEvent_t ev_route = nullptr;
    bool gpu_plan = true;  // band schedule on the GPU for non-negative sorted positions (option "gpu_plan" 0: host)
    // slices of at most PLAN_SMALL_N SNPs (a rank's shard): the GPU schedule in one fused launch, items included
    // (option "plan_fused" 0: the kernel chain of long slices)
    bool plan_fused = true;
    // timings of the last run
    double ms[6] = {0, 0, 0, 0, 0, 0};
    double flop_alg = 0, flop_issued = 0, pairs = 0, ops_alg_i8 = 0;
    int32_t n_band_items = 0;
    int last_path = 0;     // path of the last run: 0 fp32, 1 exact int8, 2 exact fp4
    int band_mode = 2;     // default correlation path (option "band_mode" 0 fp32, 1 int8, 2 fp4): exact fp4
                           // (int8 from N = 2^27)
    int n_cu = 256;

    // (the DevBuf members free themselves after this body: on `device`, set here)
    ~nldsc_engine() {
        (void)hipSetDevice(device);
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_dbg) if (e) (void)hipEventDestroy(e);
        if (ev_plan) (void)hipEventDestroy(ev_plan);
        if (copy_stream) (void)hipStreamDestroy(copy_stream);
        if (ev_issued) (void)hipEventDestroy(ev_issued);
        if (stream) (void)hipStreamDestroy(stream);
        if (plan_stream) (void)hipStreamDestroy(plan_stream);
        if (ev_pos) (void)hipEventDestroy(ev_pos);
        if (ev_stats) (void)hipEventDestroy(ev_stats);
        if (ev_replay) (void)hipEventDestroy(ev_replay);
        if (ev_route) (void)hipEventDestroy(ev_route);
    }
};

namespace {

int check_dims(int32_t n_snp, int32_t n_org, char* err, size_t errlen) {
    if (n_snp <= 0) return set_err(err, errlen, NLDSC_E_ARG, "n_snp must be positive (got %d)", n_snp);
    if (n_org <= 0) return set_err(err, errlen, NLDSC_E_ARG, "n_org must be positive (got %d)", n_org);
    return NLDSC_OK;
}

size_t bed_bytes_needed(int32_t n_snp, int32_t n_org) {
    const size_t nb = (size_t)(n_org / 4 + (n_org % 4 > 0));
    return 3 + nb * (size_t)n_snp;
}

int check_magic(const uint8_t* m, size_t len, int32_t n_snp, int32_t n_org, char* err, size_t errlen) {
    if (len < 3 || m[0] != 0x6c || m[1] != 0x1b || m[2] != 0x01)
        return set_err(err, errlen, NLDSC_E_BAD_MAGIC, "%s", kBadMagic);
    if (len < bed_bytes_needed(n_snp, n_org))
        return set_err(err, errlen, NLDSC_E_SIZE,
                       "BED file too short: %zu bytes, expected at least %zu for %d SNPs x %d individuals", len,
                       bed_bytes_needed(n_snp, n_org), n_snp, n_org);
    return NLDSC_OK;
}

int use_device(int32_t device, int* resolved, char* err, size_t errlen) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(err, errlen, NLDSC_E_NODEV, "no HIP device visible (nldsc_amd has no CPU fallback)");
    int d = device;
    if (d < 0) HIPCHK(hipGetDevice(&d));
    if (d >= n) return set_err(err, errlen, NLDSC_E_ARG, "device %d out of range (%d visible)", d, n);
    HIPCHK(hipSetDevice(d));
    *resolved = d;
    return NLDSC_OK;
}

// device buffers of a resident image of n_snp rows (all rows, pitch padding, saved last bytes, per-row flags)
hipError_t alloc_image(nldsc_engine* e, int32_t n_snp, int32_t n_org) {
    e->n_snp = e->n_org = 0;  // no valid image until finish_image
    e->kept = 0;
    e->oriented = e->orient;  // (the load's slices all use the orientation rule in force when it starts)
    hipError_t he = e->bed.ensure((size_t)padded_rows(n_snp) * (size_t)row_pitch(n_org));
    if (he == hipSuccess) he = e->lastb.ensure((size_t)n_snp);
    if (he == hipSuccess) he = e->flip.ensure((size_t)n_snp);
    if (he == hipSuccess) he = e->row_miss.ensure((size_t)n_snp);
    if (he == hipSuccess) he = e->miss_flags.ensure((size_t)n_snp);
    if (he == hipSuccess)
        he = e->lcounts.ensure((size_t)n_snp * 3);
    return he;
}

// Rows [row0, row0 + n_rows) (whole 32-SNP blocks but for the image's last) of n_snp from a .bed slice in device memory
// into the resident layout, oriented, last bytes saved, missing flags of both sample orders (the last byte keeps its
// high / low N % 4 pairs) — one pass over the slice (ld_kernels.h launch_load_slice)
hipError_t load_slice(nldsc_engine* e, const uint8_t* src, int32_t row0, int32_t n_rows, int32_t n_snp, int32_t n_org,
                      hipStream_t st) {
    const int nb = n_org / 4 + (n_org % 4 > 0), rem = n_org % 4;
    const uint32_t keep_compat = rem ? (0xFFu << (8 - 2 * rem)) & 0xFFu : 0xFFu;
    const uint32_t keep_strict = rem ? (1u << (2 * rem)) - 1u : 0xFFu;
    return nldsc::launch_load_slice(src, nb, row0, n_rows, n_snp, e->bed.p, row_pitch(n_org), e->oriented, e->flip.p,
                                    e->lastb.p, keep_compat, keep_strict, e->miss_flags.p, e->lcounts.p, st);
}

// Loads with a keep list: the file's individual count must be the list's; *n_img = the image's individuals (the kept
// count, or n_org without a list)
int keep_dims(const nldsc_engine* e, int32_t n_org, int32_t* n_img, char* err, size_t errlen) {
    *n_img = n_org;
    if (e->keep_n == 0) return NLDSC_OK;
    if (n_org != e->keep_n_file)
        return set_err(err, errlen, NLDSC_E_ARG, "n_org %d is not the keep list's file count %d", n_org, e->keep_n_file);
    *n_img = e->keep_n;
    return NLDSC_OK;
}

// load_slice of the kept samples of a slice of the file's rows (pitch nb_file): compacted into `compact` (n_rows rows
// of ceil(keep_n / 4) bytes, launch_subset_slice), then placed as a slice of keep_n individuals, on one stream
hipError_t load_slice_keep(nldsc_engine* e, const uint8_t* src, size_t nb_file, uint8_t* compact, int32_t row0,
                           int32_t n_rows, int32_t n_snp, hipStream_t st) {
    hipError_t he = nldsc::launch_subset_slice(src, (int)nb_file, n_rows, e->keep_idx.p, e->keep_n, compact, st);
    if (he == hipSuccess) he = load_slice(e, compact, row0, n_rows, n_snp, e->keep_n, st);
    return he;
}

size_t round16(size_t n) { return (n + 15) / 16 * 16; }

// after every slice is in: per-row missing flags, the missing-free block counts, and mark the image valid
hipError_t finish_image(nldsc_engine* e, int32_t n_snp, int32_t n_org) {
    hipError_t he = nldsc::launch_load_flags(e->miss_flags.p, n_snp, e->row_miss.p, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) {  // missing-free blocks per sample order
        std::vector<uint8_t> rm((size_t)n_snp);
        he = hipMemcpy(rm.data(), e->row_miss.p, (size_t)n_snp, hipMemcpyDeviceToHost);
        e->free_blocks[0] = e->free_blocks[1] = 0;
        for (int32_t b = 0; he == hipSuccess && b < (n_snp + 31) / 32; ++b) {
            uint8_t m = 0;
            for (int32_t j = 32 * b; j < std::min(n_snp, 32 * b + 32); ++j) m |= rm[(size_t)j];
            for (int o = 0; o < 2; ++o) e->free_blocks[o] += ((m >> o) & 1) ? 0 : 1;
        }
    }
    if (he == hipSuccess) {
        e->n_snp = n_snp;
        e->n_org = n_org;
        e->kept = e->keep_n;  // (loads with a list pass n_org = keep_n)
    }
    return he;
}

}  // namespace

extern "C" {

const char* nldsc_version(void) { return NLDSC_VERSION; }

int nldsc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The environment knobs of rounds 1-4 ($NLDSC_T2, $NLDSC_BAND_MODE, ...) became engine options
// (nldsc_engine_set_option) in round 5; a process that still sets one is told once, on stderr, which option replaces
// it instead of silently running the defaults.
static void warn_legacy_env_once() {
    static std::once_flag once;
    std::call_once(once, [] {
        static const char* const legacy[][2] = {
            {"NLDSC_BAND_MODE", "band_mode"}, {"NLDSC_GPU_PLAN", "gpu_plan"},   {"NLDSC_ORIENT", "orient"},
            {"NLDSC_KSPLIT", "ksplit"},       {"NLDSC_T2", "t2"},               {"NLDSC_BAND_ROUNDS", "band_rounds"},
            {"NLDSC_F4_NC2", "f4_nc2"},       {"NLDSC_Q_ROUNDS", "q_rounds"},   {"NLDSC_DEFER_REP", "defer_rep"},
            {"NLDSC_DEBUG_TIMING", "debug_timing"}, {"NLDSC_QUAD_ADD", nullptr}, {"NLDSC_REPLAY_OVERLAP", nullptr}};
        for (const auto& kv : legacy)
            if (std::getenv(kv[0]))
                std::fprintf(stderr, "nldsc_amd: $%s is no longer read; %s%s%s\n", kv[0],
                             kv[1] ? "use the engine option \"" : "the study mode it selected was removed",
                             kv[1] ? kv[1] : "", kv[1] ? "\" (nldsc_engine_set_option / Engine(options=...))" : "");
    });
}

int nldsc_engine_create(int32_t device, nldsc_engine** out, char* err, size_t errlen) {
    warn_legacy_env_once();
    if (!out) return set_err(err, errlen, NLDSC_E_ARG, "out is NULL");
    *out = nullptr;
    int d = 0;
    int rc = use_device(device, &d, err, errlen);
    if (rc) return rc;
    nldsc_engine* e = new (std::nothrow) nldsc_engine();
    if (!e) return set_err(err, errlen, NLDSC_E_OOM, "out of host memory");
    e->device = d;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > 0)
            e->n_cu = prop.multiProcessorCount;
    }
    hipError_t he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->plan_stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_issued, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_pos, hipEventDisableTiming);
    for (auto& ev : e->ev)
        if (he == hipSuccess) he = hipEventCreate(&ev);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_plan, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_stats, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_replay, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e->ev_route, hipEventDisableTiming);
    for (auto& ev : e->ev_dbg)
        if (he == hipSuccess) he = hipEventCreate(&ev);
    if (he != hipSuccess) {
        delete e;
        return set_err(err, errlen, NLDSC_E_HIP, "HIP error %s creating stream/events", hipGetErrorString(he));
    }
    *out = e;
    return NLDSC_OK;
}

void nldsc_engine_destroy(nldsc_engine* e) { delete e; }

int nldsc_engine_set_option(nldsc_engine* e, const char* name, int64_t value, char* err, size_t errlen) {
    if (!e || !name) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine or option name");
    struct Opt {
        const char* name;
        int64_t lo, hi;
        std::function<void(int64_t)> set;
    };
    const Opt opts[] = {
        {"band_mode", 0, 2, [&](int64_t v) { e->band_mode = (int)v; }},
        {"gpu_plan", 0, 1, [&](int64_t v) { e->gpu_plan = v != 0; }},
        {"plan_fused", 0, 1, [&](int64_t v) { e->plan_fused = v != 0; }},
        {"orient", 0, 1, [&](int64_t v) { e->orient = v != 0; }},
        {"ksplit", 0, 1, [&](int64_t v) { e->ksplit_ok = v != 0; }},
        {"t2", 0, 3, [&](int64_t v) { e->t2_mode = (int)v; }},
        {"band_rounds", 0, 1, [&](int64_t v) { e->band_rounds = v != 0; }},
        {"f4_nc2", 0, 1, [&](int64_t v) { e->f4_nc2 = v != 0; }},
        {"f4_nc2_dom", 0, 1, [&](int64_t v) { e->f4_nc2_dom = v != 0; }},
        {"colpair_round_items", 0, 1 << 20, [&](int64_t v) { e->colpair_round_items = (int)v; }},
        {"q_rounds", 0, 1, [&](int64_t v) { e->q_rounds = v != 0; }},
        {"defer_rep", 0, 1, [&](int64_t v) { e->defer_rep = v != 0; }},
        {"annot_batch_items", 0, INT32_MAX, [&](int64_t v) { e->annot_batch_items = (int)v; }},
        {"pairs_batch_items", 0, INT32_MAX, [&](int64_t v) { e->pairs_batch_items = (int)v; }},
        {"pairs_max_cells", 0, INT64_MAX, [&](int64_t v) { e->pairs_max_cells = v; }},
        {"cov_batch_items", 0, INT32_MAX, [&](int64_t v) { e->cov_batch_items = (int)v; }},
        {"debug_timing", 0, 1, [&](int64_t v) { e->debug_timing = v != 0; }},
    };
    for (const Opt& o : opts)
        if (std::strcmp(o.name, name) == 0) {
            if (value < o.lo || value > o.hi)
                return set_err(err, errlen, NLDSC_E_ARG, "option %s: value %lld outside [%lld, %lld]", name,
                               (long long)value, (long long)o.lo, (long long)o.hi);
            o.set(value);
            return NLDSC_OK;
        }
    return set_err(err, errlen, NLDSC_E_ARG, "unknown engine option \"%s\"", name);
}

void* nldsc_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_bufs[reinterpret_cast<uintptr_t>(p)] = bytes;
    return p;
}

void nldsc_host_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_bufs.find(reinterpret_cast<uintptr_t>(p));
        if (it == g_host_bufs.end()) return;  // not ours
        g_host_bufs.erase(it);
    }
    (void)hipHostFree(p);
}

int nldsc_engine_set_keep(nldsc_engine* e, const int32_t* idx, int32_t n_keep, int32_t n_org_file, char* err,
                          size_t errlen) {
    if (!e) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine");
    if (!idx) {  // no list: the next loads take every individual
        e->keep_n = e->keep_n_file = 0;
        return NLDSC_OK;
    }
    if (n_keep < 1 || n_keep > n_org_file)
        return set_err(err, errlen, NLDSC_E_ARG, "keep list: need 1 <= n_keep <= n_org_file (got %d of %d)", n_keep,
                       n_org_file);
    for (int32_t k = 0; k < n_keep; ++k)
        if (idx[k] < 0 || idx[k] >= n_org_file || (k > 0 && idx[k] <= idx[k - 1]))
            return set_err(err, errlen, NLDSC_E_ARG,
                           "keep list: entry %d (%d) is outside [0, %d) or not above the entry before it", k, idx[k],
                           n_org_file);
    HIPCHK(hipSetDevice(e->device));
    e->keep_n = e->keep_n_file = 0;  // (no list while the copy may fail)
    HIPCHK(e->keep_idx.ensure((size_t)n_keep));
    // (the engine stream orders the copy after an earlier load's kernels that read the old list)
    HIPCHK(hipMemcpyAsync(e->keep_idx.p, idx, sizeof(int32_t) * (size_t)n_keep, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->keep_n = n_keep;
    e->keep_n_file = n_org_file;
    return NLDSC_OK;
}

int nldsc_engine_kept(const nldsc_engine* e) { return e ? e->kept : NLDSC_E_ARG; }

int nldsc_engine_load_bed_host(nldsc_engine* e, const uint8_t* bed, size_t len, int32_t n_snp, int32_t n_org,
                               char* err, size_t errlen) {
    if (!e || !bed) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine or buffer");
    int rc = check_dims(n_snp, n_org, err, errlen);
    if (rc) return rc;
    rc = check_magic(bed, len, n_snp, n_org, err, errlen);
    if (rc) return rc;
    int32_t n_img = 0;
    rc = keep_dims(e, n_org, &n_img, err, errlen);
    if (rc) return rc;
    HIPCHK(hipSetDevice(e->device));
    const size_t nb = (size_t)(n_org / 4 + (n_org % 4 > 0)), nb_img = (size_t)(n_img / 4 + (n_img % 4 > 0));
    HIPCHK(alloc_image(e, n_snp, n_img));
    // rows go up in slices of ~64 MiB of whole 32-SNP blocks into a device staging buffer, then into the resident
    // layout (load_slice); the stream orders each slice's kernels before the next copy over the same staging bytes
    const size_t rows_per = std::max<size_t>(32, (size_t(64) << 20) / nb / 32 * 32);
    // (with a keep list: a second region takes the slice compacted to the kept samples, which load_slice then places)
    const size_t rows_max = std::min(rows_per, (size_t)n_snp), src_bytes = round16(rows_max * nb + 16);
    HIPCHK(e->stage_dev.ensure(e->keep_n ? src_bytes + rows_max * nb_img + 16 : rows_max * nb + 16));
    for (size_t r0 = 0; r0 < (size_t)n_snp; r0 += rows_per) {
        const size_t nr = std::min(rows_per, (size_t)n_snp - r0);
        HIPCHK(hipMemcpyAsync(e->stage_dev.p, bed + 3 + r0 * nb, nr * nb, hipMemcpyHostToDevice, e->stream));
        if (e->keep_n)
            HIPCHK(load_slice_keep(e, e->stage_dev.p, nb, e->stage_dev.p + src_bytes, (int)r0, (int)nr, n_snp,
                                   e->stream));
        else
            HIPCHK(load_slice(e, e->stage_dev.p, (int)r0, (int)nr, n_snp, n_org, e->stream));
    }
    HIPCHK(finish_image(e, n_snp, n_img));
    e->stage_dev.release();
    return NLDSC_OK;
}

int nldsc_engine_load_bed_device(nldsc_engine* e, const void* bed, size_t len, int32_t n_snp, int32_t n_org,
                                 char* err, size_t errlen) {
    if (!e || !bed) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine or buffer");
    int rc = check_dims(n_snp, n_org, err, errlen);
    if (rc) return rc;
    int32_t n_img = 0;
    rc = keep_dims(e, n_org, &n_img, err, errlen);
    if (rc) return rc;
    const size_t need = bed_bytes_needed(n_snp, n_org);
    if (len < 3) return set_err(err, errlen, NLDSC_E_BAD_MAGIC, "%s", kBadMagic);
    HIPCHK(hipSetDevice(e->device));
    uint8_t magic[3];
    HIPCHK(hipMemcpy(magic, bed, 3, hipMemcpyDeviceToHost));
    if (magic[0] != 0x6c || magic[1] != 0x1b || magic[2] != 0x01)
        return set_err(err, errlen, NLDSC_E_BAD_MAGIC, "%s", kBadMagic);
    if (len < need)
        return set_err(err, errlen, NLDSC_E_SIZE, "BED image too short: %zu bytes, expected at least %zu", len, need);
    HIPCHK(alloc_image(e, n_snp, n_img));
    if (e->keep_n) {
        // the kept samples go through a staging region in row slices of whole 32-SNP blocks, ~64 MiB of compact rows
        // each (the stream orders a slice's placement before the next slice's compaction over the same bytes)
        const size_t nb = (size_t)(n_org / 4 + (n_org % 4 > 0)), nb_img = (size_t)(n_img / 4 + (n_img % 4 > 0));
        const size_t rows_per = std::max<size_t>(32, (size_t(64) << 20) / nb_img / 32 * 32);
        HIPCHK(e->stage_dev.ensure(std::min(rows_per, (size_t)n_snp) * nb_img + 16));
        for (size_t r0 = 0; r0 < (size_t)n_snp; r0 += rows_per) {
            const size_t nr = std::min(rows_per, (size_t)n_snp - r0);
            HIPCHK(load_slice_keep(e, static_cast<const uint8_t*>(bed) + 3 + r0 * nb, nb, e->stage_dev.p, (int)r0,
                                   (int)nr, n_snp, e->stream));
        }
        HIPCHK(finish_image(e, n_snp, n_img));
        e->stage_dev.release();
        return NLDSC_OK;
    }
    HIPCHK(load_slice(e, static_cast<const uint8_t*>(bed) + 3, 0, n_snp, n_snp, n_org, e->stream));
    HIPCHK(finish_image(e, n_snp, n_org));
    return NLDSC_OK;
}

int nldsc_engine_load_bed_file_range(nldsc_engine* e, const char* path, int32_t n_snp_file, int32_t n_org,
                                     int32_t snp_begin, int32_t snp_end, char* err, size_t errlen) {
    if (!e || !path) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine or path");
    int rc = check_dims(n_snp_file, n_org, err, errlen);
    if (rc) return rc;
    if (snp_begin < 0 || snp_end > n_snp_file || snp_begin >= snp_end)
        return set_err(err, errlen, NLDSC_E_ARG, "SNP range [%d, %d) outside [0, %d) or empty", snp_begin, snp_end,
                       n_snp_file);
    int32_t n_img = 0;
    rc = keep_dims(e, n_org, &n_img, err, errlen);
    if (rc) return rc;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        // the reference's ifstream fails silently and then rejects the (unread) magic number
        return set_err(err, errlen, NLDSC_E_BAD_MAGIC, "%s", kBadMagic);
    }
    uint8_t magic[3] = {0, 0, 0};
    const size_t got = std::fread(magic, 1, 3, f);
    if (got < 3 || magic[0] != 0x6c || magic[1] != 0x1b || magic[2] != 0x01) {
        std::fclose(f);
        return set_err(err, errlen, NLDSC_E_BAD_MAGIC, "%s", kBadMagic);
    }
    const size_t nb = (size_t)(n_org / 4 + (n_org % 4 > 0));
    const size_t first = 3 + nb * (size_t)snp_begin, bytes = nb * (size_t)(snp_end - snp_begin);
    const size_t need = first + bytes;  // file bytes the slice needs (the whole file for [0, n_snp_file))
    auto too_short = [&](size_t have) {
        std::fclose(f);
        return set_err(err, errlen, NLDSC_E_SIZE,
                       "BED file too short: %zu bytes, expected at least %zu for %d SNPs x %d individuals", have,
                       need, snp_end, n_org);
    };
    if (fseeko(f, 0, SEEK_END) != 0) return too_short(3);
    const off_t fsize = ftello(f);
    if (fsize < 0 || (size_t)fsize < need) return too_short(fsize < 0 ? 0 : (size_t)fsize);
    HIPCHK(hipSetDevice(e->device));
    const int32_t n_snp = snp_end - snp_begin;
    {
        const hipError_t ha = alloc_image(e, n_snp, n_img);
        if (ha != hipSuccess) {
            std::fclose(f);
            return set_err(err, errlen, NLDSC_E_HIP, "HIP error %s allocating the image", hipGetErrorString(ha));
        }
    }
    // Rows stream through T reader threads, each with its own pinned slot (~32 MiB of whole rows), device staging slot
    // and stream: thread t reads slices t, t + T, ... with pread (several reads in flight: the page cache copies and
    // the device's queue run in parallel, where one fread loop held the load to one core's memcpy rate), then queues
    // the slice's H2D copy and the kernels that place its rows (load_slice), and waits for both before it reuses the
    // slot.  Slices are independent (each names its rows), so their order does not matter.
    const int fd = fileno(f);
    // (slices of whole 32-SNP blocks: load_slice)
    const size_t rows_per = std::max<size_t>(32, (size_t(32) << 20) / nb / 32 * 32), CH = rows_per * nb;
    const size_t n_slices = (bytes + CH - 1) / CH;
    const int T = (int)std::max<size_t>(1, std::min<size_t>(n_slices, (size_t)kLoadThreads));
    uint8_t* stage = nullptr;
    if (hipHostMalloc((void**)&stage, (size_t)T * CH) != hipSuccess) {
        std::fclose(f);
        return set_err(err, errlen, NLDSC_E_OOM, "cannot allocate pinned staging buffer");
    }
    // (with a keep list: T more slots after the file's, each a slice compacted to the kept samples)
    const size_t nb_img = (size_t)(n_img / 4 + (n_img % 4 > 0));
    const size_t src_bytes = round16((size_t)T * CH + 16), CH_img = round16(rows_per * nb_img);
    const bool keep = e->keep_n != 0;
    hipError_t he = e->stage_dev.ensure(keep ? src_bytes + (size_t)T * CH_img + 16 : (size_t)T * CH + 16);
    std::vector<hipStream_t> streams(T, nullptr);
    std::vector<hipEvent_t> done(T, nullptr);
    for (int t = 0; t < T && he == hipSuccess; ++t) {
        he = hipStreamCreateWithFlags(&streams[t], hipStreamNonBlocking);
        if (he == hipSuccess) he = hipEventCreateWithFlags(&done[t], hipEventDisableTiming);
    }
    std::atomic<bool> stop{false};
    std::atomic<size_t> short_at{SIZE_MAX};
    std::vector<hipError_t> terr(T, hipSuccess);
    const int dev = e->device;
    uint8_t* const dstage = e->stage_dev.p;
    auto reader = [&](int t) {
        hipError_t r = hipSetDevice(dev);
        uint8_t* buf = stage + (size_t)t * CH;
        uint8_t* dslot = dstage + (size_t)t * CH;
        bool pending = false;
        for (size_t k = (size_t)t; r == hipSuccess && k < n_slices && !stop.load(); k += (size_t)T) {
            const size_t off = k * CH, n = std::min(CH, bytes - off);
            if (pending) r = hipEventSynchronize(done[t]);
            if (r != hipSuccess) break;
            size_t got = 0;
            while (got < n) {
                const ssize_t q = pread(fd, buf + got, n - got, (off_t)(first + off + got));
                if (q < 0 && errno == EINTR) continue;
                if (q <= 0) break;
                got += (size_t)q;
            }
            if (got != n) {
                size_t cur = short_at.load();
                while (first + off + got < cur && !short_at.compare_exchange_weak(cur, first + off + got)) {
                }
                stop.store(true);
                break;
            }
            r = hipMemcpyAsync(dslot, buf, n, hipMemcpyHostToDevice, streams[t]);
            if (r == hipSuccess)
                r = keep ? load_slice_keep(e, dslot, nb, dstage + src_bytes + (size_t)t * CH_img, (int)(off / nb),
                                           (int)(n / nb), n_snp, streams[t])
                         : load_slice(e, dslot, (int)(off / nb), (int)(n / nb), n_snp, n_org, streams[t]);
            if (r == hipSuccess) r = hipEventRecord(done[t], streams[t]);
            pending = true;
        }
        if (r == hipSuccess && streams[t]) r = hipStreamSynchronize(streams[t]);
        if (r != hipSuccess) stop.store(true);
        terr[t] = r;
    };
    if (he == hipSuccess) {
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back(reader, t);
        reader(0);
        for (auto& th : pool) th.join();
        for (hipError_t r : terr)
            if (he == hipSuccess && r != hipSuccess) he = r;
    }
    for (int t = 0; t < T; ++t) {
        if (streams[t]) (void)hipStreamDestroy(streams[t]);
        if (done[t]) (void)hipEventDestroy(done[t]);
    }
    (void)hipHostFree(stage);
    e->stage_dev.release();
    if (short_at.load() != SIZE_MAX) return too_short(short_at.load());
    std::fclose(f);
    if (he != hipSuccess) return set_err(err, errlen, NLDSC_E_HIP, "HIP error %s loading BED", hipGetErrorString(he));
    HIPCHK(finish_image(e, n_snp, n_img));
    return NLDSC_OK;
}

int nldsc_engine_load_bed_file(nldsc_engine* e, const char* path, int32_t n_snp, int32_t n_org, char* err,
                               size_t errlen) {
    if (!e || !path) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine or path");
    int rc = check_dims(n_snp, n_org, err, errlen);
    if (rc) return rc;
    return nldsc_engine_load_bed_file_range(e, path, n_snp, n_org, 0, n_snp, err, errlen);
}

}  // extern "C"

namespace {

using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// What a run's parameters alone decide (with the engine's default path): sizes of the resident image and the variant
// of the kernels.
struct RunShape {
    int M, N, nb, row_bytes, pitch_words, n_it, nblk, Mpad;
    uint32_t tail_keep;  // last .bed byte: the bit pairs that are individuals
    bool dom, strict;
    int order;  // bit of row_miss: the individual slots of this run's sample order
    int path;   // 0 fp32, 1 exact int8, 2 exact fp4
    bool use_i8, use_f4;
    int max_nc;
    bool replay, split;
    int own_begin, own_end, flush_hi;
};

RunShape run_shape(const nldsc_engine* e, const nldsc_ld_params* p, int own_begin, int own_end, bool split) {
    const int M = p->n_snp, N = p->n_org, row_bytes = row_pitch(N), nblk = (M + BLK - 1) / BLK;
    // (an image of kept samples is laid out in PLINK's order, whatever the flag says: nldsc_engine_set_keep)
    const bool strict = (p->flags & NLDSC_FLAG_STRICT_PLINK_ORDER) != 0 || e->kept > 0;
    // last .bed byte: bit pairs that are individuals for the reference (high pairs first,
    // stream.h:55-66) or for PLINK (low pairs first) — the rest are recoded as missing (-> 0)
    const int rem = N % 4;
    uint32_t tail_keep = 0xFFu;
    if (rem) tail_keep = strict ? (uint32_t)((1u << (2 * rem)) - 1u) : (uint32_t)(0xFFu << (8 - 2 * rem)) & 0xFFu;
    int path = (p->flags & NLDSC_FLAG_EXACT_F4) ? 2 : (p->flags & NLDSC_FLAG_EXACT_I8) ? 1
             : (p->flags & NLDSC_FLAG_FP32) ? 0 : e->band_mode;
    // fp4 Gram entries are <= 16N: the segmented fp4 kernel keeps them exact in int32 up to N < 2^27
    if (path == 2 && N >= (1 << 27)) path = 1;
    RunShape s = {};
    s.M = M, s.N = N, s.nb = N / 4 + (N % 4 > 0), s.row_bytes = row_bytes, s.pitch_words = row_bytes / 4;
    s.n_it = row_bytes / CHUNK_BYTES, s.nblk = nblk, s.Mpad = nblk * BLK, s.tail_keep = tail_keep;
    s.dom = !(p->flags & NLDSC_FLAG_ADDITIVE_ONLY), s.strict = strict, s.order = strict ? 1 : 0;
    s.path = path, s.use_i8 = path != 0, s.use_f4 = path == 2;
    // rows longer than one fp32-exact segment: the segmented kernel (single blocks, register strips)
    // fp32 items pair a row block with up to 2 column blocks (2 waves / SIMD); the exact paths take one
    s.max_nc = s.use_i8 ? 1 : 2;
    // rare variants: the reference's fp32 residual replayed (its sums assume N < 2^23)
    s.replay = N < (1 << 23) && !(p->flags & NLDSC_FLAG_EXACT_RARE);
    // per-SNP sums accumulate for the owned SNPs, or (split runs) for every SNP from own_begin on (the right halo's to
    // be exported)
    s.split = split, s.own_begin = own_begin, s.own_end = own_end, s.flush_hi = split ? M : own_end;
    return s;
}

// How the band is scheduled: what the positions and the engine's options decide on top of the shape.
struct PlanMode {
    bool sorted, gpu_plan, fused, t2_cand, nc2, nc2d, routed, quad;
    int route_shift;  // super-items of 2^route_shift blocks a side
};

PlanMode plan_mode(const nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, bool annot = false) {
    PlanMode m;
    // band schedule: on the GPU when every position is >= 0 and sorted (the kernels run ahead of the
    // count and the host only waits for two counters), else the host replay of the reference's pointers
    const bool nonneg_sorted = nldsc::positions_nonneg_sorted(p->positions, s.M);
    m.sorted = nonneg_sorted || nldsc::positions_sorted(p->positions, s.M);
    m.gpu_plan = e->gpu_plan && nonneg_sorted && s.max_nc == 1;
    m.fused = m.gpu_plan && e->plan_fused && s.M <= nldsc::PLAN_SMALL_N;
    // the 2 x 2 block-pair workgroups: fp4, unsegmented rows, GPU plan, and no K-split (nldsc::choose_band); with
    // super-item routing (t2 modes 1 and 3) only when a missing-free block exists in this run's sample order (routing
    // takes none otherwise: C3 / C2 synthetic data, 1 % missing — the super plan, the compaction and two empty quad
    // launches cost ~50 us per run)
    m.t2_cand = e->t2_mode > 0 && m.gpu_plan && s.use_f4 && s.n_it <= nldsc::F4_SEG_CHUNKS && s.n_it >= 2 &&
                (e->t2_mode == 2 || e->free_blocks[s.order] > 0);
    // additive-only fp4 items of two column blocks (GPU plan, unsegmented rows; no K-split: its partial kernel takes
    // single block pairs)
    m.nc2 = e->f4_nc2 && m.gpu_plan && s.use_f4 && !s.dom && s.n_it <= nldsc::F4_SEG_CHUNKS;
    // add+dom column-pair rounds beside the single-block plan: long unsegmented rows in round launches (or any
    // unsegmented rows with the tests' round size); plain runs only (enqueue_band)
    m.nc2d = e->f4_nc2_dom && m.gpu_plan && s.use_f4 && s.dom && s.n_it <= nldsc::F4_SEG_CHUNKS && e->band_rounds &&
             (s.n_it >= 1024 || e->colpair_round_items > 0);
    // annotated runs: single-block items only, whatever the options say (enqueue_band_annot)
    if (annot) m.t2_cand = m.nc2 = m.nc2d = false;
    m.routed = e->t2_mode == 1 || e->t2_mode == 3;
    m.quad = e->t2_mode == 3;
    m.route_shift = m.quad ? 2 : 1;
    return m;
}

int check_run_args(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end, nldsc_ld_result* r,
                   double* table_dev, int32_t width, bool split, long long* export_dev, int32_t export_cap, char* err,
                   size_t errlen) {
    if (!e || !p || (!r && !table_dev)) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    // any run overwrites the accumulators a pending split run left for run_device_finish
    e->split.pending = false;
    if (!e->bed.p) return set_err(err, errlen, NLDSC_E_ARG, "no BED image loaded");
    if (p->n_snp != e->n_snp || p->n_org != e->n_org)
        return set_err(err, errlen, NLDSC_E_ARG, "params (%d SNPs x %d) do not match the loaded BED (%d x %d)",
                       p->n_snp, p->n_org, e->n_snp, e->n_org);
    if (!p->positions) return set_err(err, errlen, NLDSC_E_ARG, "positions is NULL");
    if (!table_dev && (!r->l2 || !r->l2d || !r->maf || !r->residuals_std || !r->l2_ws || !r->l2d_ws || !r->l2d_wse))
        return set_err(err, errlen, NLDSC_E_ARG, "a result array is NULL");
    const int M = p->n_snp;
    if (own_begin < 0 || own_end > M || own_begin > own_end)
        return set_err(err, errlen, NLDSC_E_ARG, "owned range [%d, %d) outside [0, %d)", own_begin, own_end, M);
    if (table_dev && (width <= 0 || width < own_end - own_begin))
        return set_err(err, errlen, NLDSC_E_ARG, "table width %d below the owned range's %d SNPs", width,
                       own_end - own_begin);
    if (split && (!table_dev || (export_cap > 0 && !export_dev)))
        return set_err(err, errlen, NLDSC_E_ARG, "split runs write a device table and need an export buffer");
    if (split && own_begin == own_end) return set_err(err, errlen, NLDSC_E_ARG, "split runs need an owned SNP");
    if (split && export_cap < p->n_snp - own_end)
        return set_err(err, errlen, NLDSC_E_ARG, "export capacity %d below the %d halo SNPs", export_cap,
                       p->n_snp - own_end);
    return NLDSC_OK;
}

// nothing owned: no kernel runs and no output is written (an empty GPU plan would leave the left pointers unfilled); a
// device table is all NaN
int run_nothing_owned(nldsc_engine* e, int M, int own, double* table_dev, int32_t width, char* err, size_t errlen) {
    for (int k = 0; k < 6; ++k) e->ms[k] = 0.0;
    e->pairs = e->flop_alg = e->ops_alg_i8 = e->flop_issued = 0.0;
    e->n_band_items = 0;
    e->last_ksplit = e->last_tail_ksplit = 1;
    e->last_round_items = 0;
    e->last_pair_items[0] = e->last_pair_items[1] = e->last_pair_items[2] = 0;
    e->last_direct = -1;
    e->last_band_kernel = NLDSC_BAND_F4;
    if (table_dev) {
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(e->sums.ensure(3));
        HIPCHK(hipMemsetAsync(e->sums.p, 0, 3 * sizeof(unsigned long long), e->stream));
        HIPCHK(nldsc::launch_pack_table(e->l2.p, e->l2d.p, e->maf.p, e->rstd.p, e->ws3.p, M, own, own, width,
                                        table_dev, e->sums.p, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return NLDSC_OK;
}

// Host-result runs (nldsc_engine_run): where the owned slice lands.  `h` are host pointers (DMA targets), `d` their
// device-mapped views (finalize_out_kernel writes them over the host link, no DMA after the band): the caller's arrays
// themselves when they lie in nldsc_host_alloc buffers (`direct`), else the engine's pinned landing buffer h_res,
// copied out by the host.  h_res also takes finalize's per-workgroup pair-count sums.
struct HostOut {
    struct Cols {
        double *l2, *l2d, *maf, *rstd;
        int32_t *wsa, *wsd, *wsde;
    } callers, h, d;
    bool direct;
    size_t b8, b4;  // bytes of an fp64 / int32 column of the owned slice
    int n_wsum;
    unsigned long long *wsum_h, *wsum_d;
};

int resolve_host_out(nldsc_engine* e, const nldsc_ld_result* r, int own_begin, int own_end, HostOut* out, char* err,
                     size_t errlen) {
    HostOut& o = *out;
    const int n_own = own_end - own_begin;
    const size_t b8 = o.b8 = sizeof(double) * (size_t)n_own, b4 = o.b4 = sizeof(int32_t) * (size_t)n_own;
    o.n_wsum = nldsc::finalize_out_blocks(n_own);
    const size_t wsum_off = (4 * b8 + 3 * b4 + 7) / 8 * 8;
    HIPCHK(e->h_res.ensure(wsum_off + 2 * sizeof(unsigned long long) * (size_t)o.n_wsum));
    uint8_t* dres = nullptr;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dres), e->h_res.p, 0));
    o.wsum_h = reinterpret_cast<unsigned long long*>(e->h_res.p + wsum_off);
    o.wsum_d = reinterpret_cast<unsigned long long*>(dres + wsum_off);
    const size_t ob = (size_t)own_begin;
    o.callers = {r->l2 + ob, r->l2d + ob, r->maf + ob, r->residuals_std + ob, r->l2_ws + ob, r->l2d_ws + ob,
                 r->l2d_wse + ob};
    auto reg8 = [&](double* c) { return static_cast<double*>(registered_device_ptr(c, b8)); };
    auto reg4 = [&](int32_t* c) { return static_cast<int32_t*>(registered_device_ptr(c, b4)); };
    const HostOut::Cols reg = {reg8(o.callers.l2), reg8(o.callers.l2d), reg8(o.callers.maf), reg8(o.callers.rstd),
                               reg4(o.callers.wsa), reg4(o.callers.wsd), reg4(o.callers.wsde)};
    o.direct = reg.l2 && reg.l2d && reg.maf && reg.rstd && reg.wsa && reg.wsd && reg.wsde;
    e->last_direct = o.direct ? 1 : 0;
    auto cols = [&](uint8_t* base) {  // the seven columns end to end in the landing buffer
        double* c8 = reinterpret_cast<double*>(base);
        int32_t* c4 = reinterpret_cast<int32_t*>(base + 4 * b8);
        return HostOut::Cols{c8, c8 + n_own, c8 + 2 * n_own, c8 + 3 * n_own, c4, c4 + n_own, c4 + 2 * n_own};
    };
    o.h = o.direct ? o.callers : cols(e->h_res.p);
    o.d = o.direct ? reg : cols(dres);
    return NLDSC_OK;
}

// A covariate run's request (nldsc_engine_run_covar): the caller's orthonormal basis, [n][n_org]
struct CovRun {
    const double* q;
    int n;
};

nldsc::CovArgs cov_args(const nldsc_engine* e, const RunShape& s, const CovRun& cv) {
    const size_t qm = (size_t)cv.n * (size_t)s.M;
    return {e->cov_qt.p, cv.n, e->cov_part.p, e->cov_uw.p, e->cov_uw.p + qm, e->cov_uw.p + 2 * qm, e->cov_sc.p};
}

// The restrictions of a covariate run, each with its reason (those of an annotated run: the same partial kernel; and
// the sample order the basis rows are in), the basis checked (finite, orthonormal, centred) and uploaded in the
// projection kernel's tile order (on the main stream, before the prologue), the buffers sized.
int prepare_cov(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const CovRun& cv, bool other, char* err,
                size_t errlen) {
    if (other)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "covariates with annotations or a pair table in one run are not supported");
    if (cv.n < 1 || cv.n > NLDSC_MAX_COVAR)
        return set_err(err, errlen, NLDSC_E_ARG, "n_covar %d outside [1, %d]", cv.n, NLDSC_MAX_COVAR);
    if (!cv.q) return set_err(err, errlen, NLDSC_E_ARG, "q_basis is NULL");
    if (cv.n > p->n_org - 3)
        return set_err(err, errlen, NLDSC_E_ARG, "n_covar %d leaves fewer than 3 degrees of freedom of %d individuals",
                       cv.n, p->n_org);
    if (p->n_org >= (1 << 19))
        return set_err(err, errlen, NLDSC_E_ARG,
                       "covariate runs need n_org < 2^19 (got %d): the K-split partial kernel takes unsegmented rows",
                       p->n_org);
    if (s.path != 2)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "covariate runs take the exact fp4 path only: this run's flags or the band_mode option select %s",
                       s.path == 0 ? "fp32" : "exact int8");
    if (!s.strict)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "covariate runs use PLINK's sample order (the basis rows are .fam lines): set "
                       "NLDSC_FLAG_STRICT_PLINK_ORDER");
    const size_t N = (size_t)s.N, C = (size_t)cv.n;
    const double tol_sum = 1e-8 * std::sqrt((double)s.N);
    for (size_t c = 0; c < C; ++c) {
        const double* col = cv.q + c * N;
        double sum = 0.0;
        for (size_t i = 0; i < N; ++i) {
            if (!std::isfinite(col[i]))
                return set_err(err, errlen, NLDSC_E_ARG, "q_basis column %zu, individual %zu: the value is not finite",
                               c, i);
            sum += col[i];
        }
        if (!(std::fabs(sum) <= tol_sum))
            return set_err(err, errlen, NLDSC_E_ARG,
                           "q_basis column %zu is not centred: its sum is %.3e (limit 1e-8 sqrt(n_org))", c, sum);
    }
    for (size_t a = 0; a < C; ++a)
        for (size_t b = a; b < C; ++b) {
            const double *x = cv.q + a * N, *y = cv.q + b * N;
            double d[4] = {0.0, 0.0, 0.0, 0.0};
            size_t i = 0;
            for (; i + 4 <= N; i += 4)
                for (int k = 0; k < 4; ++k) d[k] += x[i + k] * y[i + k];
            for (; i < N; ++i) d[0] += x[i] * y[i];
            const double dot = (d[0] + d[1]) + (d[2] + d[3]);
            if (!(std::fabs(dot - (a == b ? 1.0 : 0.0)) <= 1e-8))
                return set_err(err, errlen, NLDSC_E_ARG,
                               "q_basis is not orthonormal: columns %zu . %zu = %.12g (limit 1e-8 from %d)", a, b, dot,
                               a == b ? 1 : 0);
        }
    // the projection kernel's tiles: [chunk][group][128 samples][16 covariates], zero padded
    const int NG = nldsc::covar_groups(cv.n);
    const size_t tile = (size_t)128 * 16 * NG, n_qt = (size_t)s.n_it * tile;
    e->h_qt.assign(n_qt, 0.0);
    for (size_t c = 0; c < C; ++c) {
        const double* col = cv.q + c * N;
        const size_t g = c / 16, cc = c % 16;
        for (size_t i = 0; i < N; ++i) e->h_qt[(i / 128) * tile + (g * 128 + i % 128) * 16 + cc] = col[i];
    }
    HIPCHK(hipSetDevice(e->device));
    const size_t M = (size_t)s.M;
    const int P = nldsc::covar_pieces(s.nblk, s.n_it, e->n_cu);
    HIPCHK(e->cov_qt.ensure(n_qt));
    HIPCHK(e->cov_part.ensure((size_t)P * (size_t)s.nblk * 96 * 16 * NG));
    HIPCHK(e->cov_uw.ensure(3 * C * M));
    HIPCHK(e->cov_sc.ensure(5 * M));
    e->cov_n = e->cov_M = 0;  // (no projections to report until this run's are written)
    HIPCHK(hipMemcpyAsync(e->cov_qt.p, e->h_qt.data(), sizeof(double) * n_qt, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return NLDSC_OK;
}

// A dom-dom run's request (nldsc_engine_run_domdom): the caller's L2DD array, [n_snp]
struct DomDomRun {
    double* l2dd;
};

// The restrictions of a dom-dom run, each with its reason (those of an annotated run: the same partial kernel; and the
// dominance residual must exist).  They need the parameters and the engine's options only, so they come before the
// parameters are held against the loaded image.
int check_dd(const nldsc_engine* e, const nldsc_ld_params* p, const DomDomRun& dd, bool other, char* err,
             size_t errlen) {
    if (other)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "dom-dom scores with annotations, a pair table or covariates in one run are not supported");
    if (!dd.l2dd) return set_err(err, errlen, NLDSC_E_ARG, "l2dd is NULL");
    if (p->flags & NLDSC_FLAG_ADDITIVE_ONLY)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "dom-dom scores need the dominance residuals: not with NLDSC_FLAG_ADDITIVE_ONLY");
    if (p->n_org >= (1 << 19))
        return set_err(err, errlen, NLDSC_E_ARG,
                       "dom-dom runs need n_org < 2^19 (got %d): the K-split partial kernel takes unsegmented rows",
                       p->n_org);
    const RunShape s = run_shape(e, p, 0, p->n_snp, false);
    if (s.path != 2)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "dom-dom runs take the exact fp4 path only: this run's flags or the band_mode option select %s",
                       s.path == 0 ? "fp32" : "exact int8");
    return NLDSC_OK;
}

// the accumulator and the owned slice's landing buffer of a dom-dom run, the accumulator zeroed (main stream, before
// the prologue)
int prepare_dd(nldsc_engine* e, const RunShape& s, char* err, size_t errlen) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->l2dd_acc.ensure((size_t)s.M));
    HIPCHK(e->l2dd_out.ensure((size_t)std::max(s.own_end - s.own_begin, 1)));
    HIPCHK(hipMemsetAsync(e->l2dd_acc.p, 0, sizeof(double) * (size_t)s.M, e->stream));
    return NLDSC_OK;
}

// the work buffers of a run, sized (allocation happens on the first run of a size; the enqueue phases allocate only
// what depends on the schedule's counts)
int ensure_run_buffers(nldsc_engine* e, const RunShape& s, const PlanMode& m, char* err, size_t errlen) {
    const size_t M = (size_t)s.M;
    HIPCHK(e->counts.ensure(M * 4));
    HIPCHK(e->cparts.ensure(M * 3));
    HIPCHK(e->rep_count.ensure(1));  // (zeroed by the statistics kernel)
    HIPCHK(e->lut.ensure((size_t)s.Mpad * 4));
    HIPCHK(e->cst.ensure((size_t)s.Mpad));
    HIPCHK(e->sflags.ensure((size_t)s.Mpad));
    HIPCHK(e->blk_rep.ensure((size_t)s.nblk));
    HIPCHK(e->pos.ensure(M));
    HIPCHK(e->res.ensure(4 * M + (3 * M + 1) / 2));
    e->l2.p = e->res.p;
    e->l2d.p = e->l2.p + M;
    e->maf.p = e->l2d.p + M;
    e->rstd.p = e->maf.p + M;
    e->ws3.p = reinterpret_cast<int*>(e->rstd.p + M);
    HIPCHK(e->Lw.ensure(M));
    HIPCHK(e->Rw.ensure(M));
    HIPCHK(e->l2_acc.ensure(M));
    HIPCHK(e->l2d_acc.ensure(M));
    HIPCHK(e->ws_acc.ensure(M * 4));  // WSA, WSD, WSDE, non-finite flags
    if (m.gpu_plan) {
        const size_t n_t = (size_t)(s.nblk + 15) / 16;
        // window edges A | E, then the right-pointer scan's tile maxima
        HIPCHK(e->Aw.ensure(2 * M + (M + 255) / 256));
        HIPCHK(e->plan_rows.ensure((size_t)s.nblk));
        HIPCHK(e->plan_counts.ensure(n_t * n_t));
        HIPCHK(e->plan_meta.ensure(12));  // [0, 4) single-block plan, [4, 8) super-item plan, [8, 10) column-pair plan
        HIPCHK(e->h_meta.ensure(12 * sizeof(int)));
        if (m.nc2d) {
            HIPCHK(e->plan_counts_p.ensure(n_t * n_t));
            HIPCHK(e->plan_counts_s.ensure(n_t * n_t));
        }
        if (m.fused) HIPCHK(e->items.ensure(nldsc::plan_small_items(s.M)));  // (emitted with the plan)
        if (m.t2_cand) {
            const size_t nblk2 = (size_t)(s.nblk + 1) / 2, n_t2 = (nblk2 + 15) / 16;
            HIPCHK(e->plan_rows2.ensure(nblk2));
            HIPCHK(e->plan_counts2.ensure(
                std::max<size_t>(n_t2 * n_t2, (size_t)nldsc::plan_super_counts(s.M, m.route_shift))));
        }
    }
    return NLDSC_OK;
}

// Everything that needs no schedule, on three streams: positions, window edges and tail counts on the main stream, the
// plan on the plan stream beside them, then statistics, pair range, replay flags, left pointers, the blocks' missing
// flags, and the rare-variant replay on the side stream.
int enqueue_prologue(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m, char* err,
                     size_t errlen, const CovRun* cv = nullptr) {
    const int M = s.M;
    hipStream_t st = e->stream, cs = e->copy_stream, ps = e->plan_stream;
    const uint8_t* flip = e->oriented ? e->flip.p : nullptr;
    // The positions go up and the schedule's window edges are searched first (~0.02 ms: beside the count kernel, whose
    // streaming saturates HBM, those dependent loads took 0.05-0.1 ms on the critical path of short runs); then the
    // count kernel, with the rest of the schedule beside it on the plan stream.
    const size_t b_pos = sizeof(double) * (size_t)M;
    if (registered_device_ptr(p->positions, b_pos)) {  // (pinned: the DMA reads them in place)
        HIPCHK(hipMemcpyAsync(e->pos.p, p->positions, b_pos, hipMemcpyHostToDevice, st));
    } else {
        HIPCHK(e->h_pos.ensure(b_pos));
        const CopyPool::Seg seg = {e->h_pos.p, p->positions, b_pos};
        e->copies.copy(&seg, 1);
        HIPCHK(hipMemcpyAsync(e->pos.p, e->h_pos.p, b_pos, hipMemcpyHostToDevice, st));
    }
    if (m.gpu_plan)
        HIPCHK(nldsc::launch_plan_edges(e->pos.p, M, p->ld_wind, e->Aw.p, e->Aw.p + M, e->plan_meta.p, st));
    HIPCHK(hipEventRecord(e->ev_pos, st));
    // non-individual slots read as missing (0x55) for the int8 / fp32 kernels, as 00 (all fp4 planes zero) for fp4;
    // the genotype counts: the load's (every byte before the last) plus this run's last byte
    const uint32_t pad = s.use_f4 ? 0x00u : 0x55u;
    HIPCHK(hipEventRecord(e->ev[0], st));  // (count_ms: the tail kernel alone; the host total covers the above)
    HIPCHK(nldsc::launch_tail_counts(e->bed.p, e->lastb.p, M, s.nb, s.row_bytes, s.tail_keep, pad, e->lcounts.p,
                                     1, e->cparts.p, st));  // (the load's parts add into one: load_tiled_kernel)
    HIPCHK(hipEventRecord(e->ev[1], st));
    if (m.gpu_plan) {
        HIPCHK(hipStreamWaitEvent(ps, e->ev_pos, 0));
        HIPCHK(nldsc::launch_plan(M, s.own_begin, s.own_end, e->Aw.p, e->Aw.p + M, e->Rw.p, e->plan_rows.p,
                                  e->plan_counts.p, e->plan_meta.p, ps, m.nc2, m.fused ? e->items.p : nullptr));
        if (m.t2_cand)
            HIPCHK(nldsc::launch_plan_super(M, e->plan_rows.p, e->plan_rows2.p, e->plan_counts2.p, e->plan_meta.p + 4,
                                            m.route_shift, ps));
        for (int k = 0; k < 8; ++k) reinterpret_cast<volatile int*>(e->h_meta.p)[k] = -1;  // (counts land >= 0)
        HIPCHK(hipMemcpyAsync(e->h_meta.p, e->plan_meta.p, 8 * sizeof(int), hipMemcpyDeviceToHost, ps));
        HIPCHK(hipEventRecord(e->ev_plan, ps));
    }
    HIPCHK(nldsc::launch_snp_stats(e->cparts.p, 1, e->counts.p, e->rep_count.p, flip, e->pos.p, M, s.Mpad, s.N, p->maf,
                                   p->std_thr, e->lut.p, e->cst.p, e->sflags.p, e->maf.p, e->rstd.p, st, e->l2_acc.p,
                                   e->l2d_acc.p, e->ws_acc.p, e->blk_rep.p));
    // split runs: the pairs whose lower SNP is owned (flag bit 3), before the replay may touch the flags (ev_stats)
    if (s.split) HIPCHK(nldsc::launch_pair_range(e->sflags.p, M, s.own_begin, s.own_end, st));
    // covariate runs: every SNP's projections on the covariate basis, then its residual std and residual-pass flag
    // (bit 1) for the model with covariates — before anything reads that bit (the band); part of the statistics
    // stage's time (ev[1] .. ev[2])
    if (cv)
        HIPCHK(nldsc::launch_covar_project(e->bed.p, s.row_bytes, M, s.N, e->counts.p, p->std_thr, cov_args(e, s, *cv),
                                           nldsc::covar_pieces(s.nblk, s.n_it, e->n_cu), e->sflags.p, e->rstd.p, st));
    // rare variants: the reference's fp32 residual replayed (its sums assume N < 2^23); the flags per block here,
    // the replay itself after the schedule (below)
    // Invariant of the overlap: the replay rewrites, for replayed SNPs only, sflags bit 1 (residual pass; a byte
    // read-modify-write), cst and lut.  What runs beside it on the main stream reads sflags bits 0 (MAF pass:
    // left_pointer_kernel, the host flag copy) and 2 (missing calls: the band kernels' rm / cm), which the
    // replay never changes, and never reads a replayed SNP's cst / lut before ev_replay: the items
    // of blocks holding one are skipped (skip_item) until the KC launch, and the K-split part kernel, which runs
    // them, stores Gram tiles without reading constants.  No other kernel writes sflags after snp_stats_kernel.
    if (s.replay) {
        HIPCHK(nldsc::launch_replay_flags(e->counts.p, flip, e->sflags.p, M, e->blk_rep.p, st, true));
        HIPCHK(hipEventRecord(e->ev_stats, st));
    }
    HIPCHK(hipEventRecord(e->ev[2], st));
    // What needs no schedule goes out before the host waits for it (C2 / a rank's shard: the count ends first, and
    // the host's enqueue after that wait is on the critical path): the left pointers (the window edges came before the
    // count), the blocks' missing flags (from the load) and the rare-variant replay — a few long sequential sums, on
    // the side stream beside the band launch for the items without a replayed SNP; only the KC launch and finalize
    // wait for it (ev_replay).  (Its sums assume N < 2^23.)
    if (m.gpu_plan) HIPCHK(nldsc::launch_left_pointers(e->Aw.p, e->sflags.p, e->pos.p, M, e->Lw.p, st));
    if (s.use_f4) {  // per 32-SNP block: holds a missing call (the kernels' m-product predicate: routing, issued count)
        HIPCHK(e->blk_miss.ensure((size_t)s.nblk));
        HIPCHK(nldsc::launch_block_missing_rows(e->row_miss.p, M, s.order, e->blk_miss.p, m.gpu_plan ? ps : st));
    }
    if (s.replay) {
        HIPCHK(hipStreamWaitEvent(cs, e->ev_stats, 0));
        HIPCHK(nldsc::launch_reference_residuals(e->bed.p, s.row_bytes, s.N, s.strict, e->counts.p, flip, M, p->std_thr,
                                                 e->cst.p, e->lut.p, e->sflags.p, e->rstd.p, cs));
        HIPCHK(hipEventRecord(e->ev_replay, cs));
    }
    return NLDSC_OK;
}

// the band's work, as the schedule decided it
struct Schedule {
    int n_items = 0, n_items2 = 0;  // single-block items, super-items
    int ksplit = 1;                 // K-split of the whole band
    bool use_t2 = false;            // the super-item kernels run
    bool compact = false;           // the single-block kernel's items are compacted (items_u, count in h_route)
    bool colpair = false;           // the add+dom column-pair plan is queued (items_p / items_s, counts in h_meta[8..9])
};

// The GPU plan: the host waits for its two counters, decides the kernels, and queues the work lists on the plan stream.
int schedule_on_gpu(nldsc_engine* e, const RunShape& s, const PlanMode& m, Schedule* out, char* err, size_t errlen) {
    Schedule& sc = *out;
    hipStream_t ps = e->plan_stream;
    // the count kernel is running meanwhile; the host polls the pinned counters (a blocking event wait wakes
    // the thread tens of microseconds late: the schedule is on the critical path of short runs — a 1/8 shard,
    // C2 — whose count ends first), then the event confirms the whole copy
    (void)spin_until_nonneg(reinterpret_cast<volatile const int*>(e->h_meta.p) + 1);
    HIPCHK(hipEventSynchronize(e->ev_plan));
    const int* meta = reinterpret_cast<const int*>(e->h_meta.p);
    sc.n_items = meta[1];
    const nldsc::BandChoice c = nldsc::choose_band(sc.n_items, s.n_it, e->n_cu, s.use_f4,
                                                   s.use_f4 && !m.nc2 && e->ksplit_ok, e->band_rounds, m.t2_cand);
    sc.ksplit = c.ksplit;
    sc.use_t2 = c.use_t2;
    // The work lists go out on the plan stream, beside the count kernel: the items, the super-items and, with
    // super-item routing (blk_miss), the list of the items the single-block kernel keeps, compacted in order,
    // so its launches (round launches, the K-split tail) are sized by its own work — its length reaches the host
    // before the band.  The main stream waits for them.
    if (sc.use_t2) {
        sc.n_items2 = meta[5];
        HIPCHK(e->items2.ensure(std::max<size_t>((size_t)sc.n_items2, 1)));
        HIPCHK(nldsc::launch_plan_emit_super(s.M, e->plan_rows2.p, e->plan_meta.p + 4, e->plan_counts2.p, e->items2.p,
                                             m.route_shift, ps));
    }
    if (!sc.use_t2 || m.routed) {
        HIPCHK(e->items.ensure(std::max<size_t>((size_t)sc.n_items, 1)));  // (fused: already holds them)
        if (sc.n_items > 0 && !m.fused)
            HIPCHK(nldsc::launch_plan_emit(s.M, e->plan_rows.p, e->plan_meta.p, e->plan_counts.p, e->items.p, ps,
                                           m.nc2));
    }
    // add+dom column-pair rounds: the pairs and leftover singles of the same rows, beside the single-block list (which
    // stays the run's item count and its issued-product count); their totals reach the host before the band
    // (h_meta[8..9]; routed runs compact both lists in enqueue_band, counts in h_meta[10..11])
    {
        const int round = e->colpair_round_items > 0 ? e->colpair_round_items : 4 * e->n_cu;
        const int min_rounds = e->colpair_round_items > 0 ? 1 : nldsc::COLPAIR_ROUND_MIN;
        // (with the super-item kernels: only beside routing, which leaves the single-block kernels the rest)
        sc.colpair = m.nc2d && (!sc.use_t2 || m.routed) && (sc.ksplit == 1 || e->colpair_round_items > 0) &&
                     (int64_t)sc.n_items >= (int64_t)2 * min_rounds * round;
    }
    if (sc.colpair) {
        HIPCHK(e->items_p.ensure((size_t)sc.n_items));
        HIPCHK(e->items_s.ensure((size_t)sc.n_items));
        volatile int* tot = reinterpret_cast<volatile int*>(e->h_meta.p) + 8;
        tot[0] = tot[1] = -1;  // (the copy below lands the counts, >= 0)
        HIPCHK(nldsc::launch_plan_split(s.M, e->plan_rows.p, e->plan_meta.p, e->plan_counts_p.p, e->plan_counts_s.p,
                                        e->plan_meta.p + 8, e->items_p.p, e->items_s.p, ps));
        HIPCHK(hipMemcpyAsync(e->h_meta.p + 8 * sizeof(int), e->plan_meta.p + 8, 2 * sizeof(int), hipMemcpyDeviceToHost,
                              ps));
    }
    sc.compact = sc.use_t2 && m.routed && sc.n_items > 0;
    if (sc.compact) {
        const size_t n_chunks = ((size_t)sc.n_items + 255) / 256;  // (ld_kernels.hip COMPACT_CHUNK)
        HIPCHK(e->items_u.ensure((size_t)sc.n_items));
        HIPCHK(e->compact_tmp.ensure(n_chunks + 1));
        HIPCHK(e->h_route.ensure(sizeof(int)));
        *reinterpret_cast<volatile int*>(e->h_route.p) = -1;  // (the copy below lands the count, >= 0)
        HIPCHK(nldsc::launch_compact_items(e->items.p, sc.n_items, e->blk_miss.p, m.route_shift, s.nblk,
                                           e->compact_tmp.p, e->compact_tmp.p + n_chunks, e->items_u.p, ps));
        HIPCHK(hipMemcpyAsync(e->h_route.p, e->compact_tmp.p + n_chunks, sizeof(int), hipMemcpyDeviceToHost, ps));
    }
    HIPCHK(hipEventRecord(e->ev_route, ps));
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_route, 0));  // the band reads the schedule and the lists
    return NLDSC_OK;
}

// The host replay of the reference's pointers and the host plan, uploaded on the main stream.
int schedule_on_host(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m, Schedule* out,
                     char* err, size_t errlen) {
    const int M = s.M;
    hipStream_t st = e->stream;
    e->h_L.resize(M);
    e->h_R.resize(M);
    const uint8_t* flags = nullptr;
    if (m.sorted) {
        // Sorted positions: nothing waits for the GPU.  The right pointers and the all-pass left
        // pointers do not depend on the MAF flags, and SNPs failing MAF only shrink the set of needed
        // block pairs (their L_j grow, their rows and columns drop), so the all-pass schedule is a
        // superset of the exact one; it is planned here while the GPU counts, and the exact left
        // pointers come from the device flags (left_pointer_kernel).  The kernels mask every pair
        // with the exact pointers.
        e->h_all_pass.assign(M, 1);
        flags = e->h_all_pass.data();
    } else {
        // unsorted positions: the reference's sequential pointer semantics need the MAF flags first
        e->h_flags.resize(s.Mpad);
        HIPCHK(hipMemcpyAsync(e->h_flags.data(), e->sflags.p, s.Mpad, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        flags = e->h_flags.data();
    }
    nldsc::replay_windows(p->positions, flags, M, p->ld_wind, e->h_L.data(), e->h_R.data());
    nldsc::plan_items(p->positions, flags, M, p->ld_wind, e->h_L.data(), e->h_R.data(), s.own_begin, s.own_end,
                      s.max_nc, e->h_items);
    // the band kernel reads rows [32 I, 32 (J0 + nc)) of geno / lut: check before launching
    if (s.pitch_words % 8 != 0 || s.n_it * 8 != s.pitch_words)
        return set_err(err, errlen, NLDSC_E_ARG, "internal: bad row pitch %d", s.pitch_words);
    for (const nldsc::PlanItem& it : e->h_items)
        if (it.x < 0 || it.y < it.x || (it.z != 1 && it.z != 2) || it.y + it.z > s.nblk)
            return set_err(err, errlen, NLDSC_E_ARG, "internal: bad work item (%d, %d, %d) for %d blocks", it.x,
                           it.y, it.z, s.nblk);
    if (s.max_nc == 1) nldsc::order_items_tiled(e->h_items, s.nblk, TILE_R, TILE_C, e->h_scratch);
    HIPCHK(e->items.ensure(std::max<size_t>(e->h_items.size(), 1)));
    // the plan goes up through pinned staging: a copy from pageable memory would block this thread
    // until the stream drains (the count kernel), pinned copies are queued and return at once
    const size_t bL = sizeof(int) * (size_t)M, bI = sizeof(nldsc::PlanItem) * e->h_items.size();
    HIPCHK(e->h_stage.ensure(2 * bL + bI));
    std::memcpy(e->h_stage.p, e->h_L.data(), bL);
    std::memcpy(e->h_stage.p + bL, e->h_R.data(), bL);
    if (bI) std::memcpy(e->h_stage.p + 2 * bL, e->h_items.data(), bI);
    if (m.sorted) {
        HIPCHK(e->Aw.ensure((size_t)M));
        HIPCHK(hipMemcpyAsync(e->Aw.p, e->h_stage.p, bL, hipMemcpyHostToDevice, st));
        HIPCHK(nldsc::launch_left_pointers(e->Aw.p, e->sflags.p, e->pos.p, M, e->Lw.p, st));
    } else {
        HIPCHK(hipMemcpyAsync(e->Lw.p, e->h_stage.p, bL, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(e->Rw.p, e->h_stage.p + bL, bL, hipMemcpyHostToDevice, st));
    if (bI) HIPCHK(hipMemcpyAsync(e->items.p, e->h_stage.p + 2 * bL, bI, hipMemcpyHostToDevice, st));
    out->n_items = (int)e->h_items.size();
    out->ksplit = nldsc::choose_ksplit(out->n_items, s.n_it, e->n_cu, s.use_f4 && !m.nc2 && e->ksplit_ok);
    return NLDSC_OK;
}

// what every band launch of the run shares (ld_kernels.h)
nldsc::BandArgs fill_band_args(const nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m) {
    nldsc::BandArgs a;
    a.geno = reinterpret_cast<const uint32_t*>(e->bed.p);  // the resident rows (Mpad rows at row_bytes pitch) in place
    a.pitch_words = s.pitch_words, a.n_it = s.n_it, a.cst = e->cst.p, a.lut = e->lut.p;
    a.pos = e->pos.p, a.Lw = e->Lw.p, a.Rw = e->Rw.p, a.sflags = e->sflags.p, a.n_snp = s.M;
    a.ld_wind = p->ld_wind, a.n_org = (double)s.N, a.rsq_thr = p->rsq_thr;
    a.own_lo = s.own_begin, a.own_hi = s.flush_hi;
    a.l2_acc = e->l2_acc.p, a.l2d_acc = e->l2d_acc.p, a.ws_acc = e->ws_acc.p;
    a.dom = s.dom, a.blk_rep = s.replay ? e->blk_rep.p : nullptr;
    a.rows = e->plan_rows.p, a.nblk = s.nblk, a.route_shift = m.route_shift, a.st = e->stream;
    return a;
}

// the single-block launches of a run: the list (compacted when routed), its shape, the routing map they drop items by
struct SingleLaunch {
    const int4* items;
    int n;
    nldsc::SingleShape shape;
    const uint8_t* miss;
};

// which = 1: the launch for the items without a replayed SNP (beside the replay), 2: the KC launch after it
hipError_t launch_super(nldsc_engine* e, const nldsc::BandArgs& a, const PlanMode& m, int n_items2, int which) {
    if (m.quad)
        return nldsc::launch_band_f4_q(a, e->items2.p, n_items2, which, e->blk_miss.p,
                                       e->q_rounds && n_items2 >= 16 * e->n_cu ? e->n_cu : 0);
    return nldsc::launch_band_f4_t2(a, e->items2.p, n_items2, which, m.routed ? e->blk_miss.p : nullptr);
}

hipError_t launch_single(nldsc_engine* e, const nldsc::BandArgs& a, const RunShape& s, const PlanMode& m, int ksplit,
                         const SingleLaunch& L, int which) {
    if (!s.use_f4) return nldsc::launch_band_i8(a, L.items, L.n, which);
    if (ksplit > 1) return nldsc::launch_band_f4_split(a, ksplit, L.items, L.n, e->gram.p, which, nullptr);
    const int n_full = L.shape.n_full, per = m.nc2 ? 2 : 1;
    const bool dfr = L.shape.defer && n_full > 0;
    const nldsc::DeferredEpi rep = {e->rep_gram.p, e->rep_items.p, e->rep_count.p};
    hipError_t r = nldsc::launch_band_f4(a, per, L.items, n_full, which, L.miss, L.shape.round_items,
                                         dfr ? &rep : nullptr);
    if (r == hipSuccess && dfr && (which & 2))  // after the replay: the deferred items' epilogues
        r = nldsc::launch_band_f4_deferred_epi(a, n_full * per, rep);
    if (r != hipSuccess || n_full == L.n) return r;
    return nldsc::launch_band_f4_split(a, L.shape.tail_p, L.items + n_full, L.n - n_full, e->gram.p, which, L.miss);
}

// Column-pair rounds (nldsc::shape_colpair): the pairs' full rounds in the one-wave kernel, then the rest as a
// single-block band; the deferred rare-variant items of both share the slot tables, their epilogues after the replay
// (pairs / rest: the lists, compacted in routed runs; miss: the routing map then — a pair may keep one block, and the
// last pairs' single blocks are not compacted)
hipError_t launch_colpair(nldsc_engine* e, const nldsc::BandArgs& a, const nldsc::ColpairShape& cp, const int4* pairs,
                          const int4* rest, const uint8_t* miss, int which) {
    const nldsc::SingleShape& rs = cp.rest;
    const bool dfr = rs.defer;
    const nldsc::DeferredEpi rep = {e->rep_gram.p, e->rep_items.p, e->rep_count.p};
    hipError_t r = nldsc::launch_band_f4(a, 2, pairs, cp.n_pair_full, which, miss, cp.round_items, dfr ? &rep : nullptr);
    if (r == hipSuccess)
        r = nldsc::launch_band_f4(a, 1, rest, rs.n_full, which, miss, rs.round_items, dfr ? &rep : nullptr);
    if (r == hipSuccess && dfr && (which & 2))
        r = nldsc::launch_band_f4_deferred_epi(a, 2 * cp.n_pair_full + rs.n_full, rep);
    if (r != hipSuccess || rs.n_full == cp.n_rest) return r;
    return nldsc::launch_band_f4_split(a, rs.tail_p, rest + rs.n_full, cp.n_rest - rs.n_full, e->gram.p, which, miss);
}

// An annotated run's request (nldsc_engine_run_annot): the caller's category-major arrays
struct AnnotRun {
    const double* annot;
    int n;
    double *l2, *l2d;
};

// The restrictions of an annotated run, each with its reason, then the annotation matrix and its fixed-point scales
// to the device (on the main stream, before the prologue) and the accumulators sized.
int prepare_annot(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const AnnotRun& an, char* err,
                  size_t errlen) {
    if (an.n < 1 || an.n > NLDSC_MAX_ANNOT)
        return set_err(err, errlen, NLDSC_E_ARG, "n_annot %d outside [1, %d]", an.n, NLDSC_MAX_ANNOT);
    if (!an.annot || !an.l2 || (!an.l2d && s.dom))
        return set_err(err, errlen, NLDSC_E_ARG,
                       "annot, l2_annot or l2d_annot is NULL (l2d_annot may be NULL only with NLDSC_FLAG_ADDITIVE_ONLY)");
    if (p->n_org >= (1 << 19))
        return set_err(err, errlen, NLDSC_E_ARG,
                       "annotated runs need n_org < 2^19 (got %d): the K-split partial kernel takes unsegmented rows",
                       p->n_org);
    if (s.path != 2)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "annotated runs take the exact fp4 path only: this run's flags or the band_mode option select %s",
                       s.path == 0 ? "fp32" : "exact int8");
    const size_t M = (size_t)s.M, C = (size_t)an.n;
    std::vector<double> scale(C);
    for (size_t c = 0; c < C; ++c) {
        double mx = 0.0;
        const double* col = an.annot + c * M;
        for (size_t j = 0; j < M; ++j) {
            if (!std::isfinite(col[j]))
                return set_err(err, errlen, NLDSC_E_ARG, "annotation %zu, SNP %zu: the value is not finite", c, j);
            mx = std::max(mx, std::fabs(col[j]));
        }
        scale[c] = nldsc::annot_scale(nldsc::annot_scale_exp(mx));
    }
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(e->annot_dev.ensure(C * M));
    HIPCHK(e->annot_scale.ensure(C));
    HIPCHK(e->l2c_acc.ensure(2 * C * M));
    if (s.dom) HIPCHK(e->l2dc_acc.ensure(2 * C * M));
    HIPCHK(e->annot_out.ensure(2 * C * (size_t)(s.own_end - s.own_begin)));
    // (pageable sources: the copies return once the bytes are staged, so `scale` may go out of scope)
    HIPCHK(hipMemcpyAsync(e->annot_dev.p, an.annot, sizeof(double) * C * M, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->annot_scale.p, scale.data(), sizeof(double) * C, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemsetAsync(e->l2c_acc.p, 0, sizeof(double) * 2 * C * M, e->stream));
    if (s.dom) HIPCHK(hipMemsetAsync(e->l2dc_acc.p, 0, sizeof(double) * 2 * C * M, e->stream));
    return NLDSC_OK;
}

nldsc::AnnotArgs annot_args(const nldsc_engine* e, const RunShape& s, const AnnotRun& an) {
    const size_t limb = (size_t)an.n * (size_t)s.M;  // (the residual limbs follow the accumulators)
    return {e->annot_dev.p, e->annot_scale.p, an.n, e->l2c_acc.p, s.dom ? e->l2dc_acc.p : nullptr,
            e->l2c_acc.p + limb, s.dom ? e->l2dc_acc.p + limb : nullptr};
}

// The band of an annotated run (ev[3] .. ev[4]): after the rare-variant replay, the single-block items in batches
// (nldsc::plan_annot_batches) through the K-split partial kernel and the annotated epilogue (launch_band_f4_annot);
// then the issued-product count as enqueue_band queues it.
int enqueue_band_annot(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m,
                       const Schedule& sc, const AnnotRun& an, char* err, size_t errlen) {
    hipStream_t st = e->stream, cs = e->copy_stream;
    const int n_items = sc.n_items;
    HIPCHK(hipEventRecord(e->ev[3], st));
    const std::vector<nldsc::AnnotBatch> batches = nldsc::plan_annot_batches(
        n_items, s.n_it, e->n_cu, e->ksplit_ok, e->annot_batch_items, nldsc::ANNOT_GRAM_CAP_BYTES);
    size_t units = 0;
    int p_max = 1;
    for (const nldsc::AnnotBatch& b : batches) {
        units = std::max(units, (size_t)b.n * (size_t)b.ksplit);
        p_max = std::max(p_max, b.ksplit);
    }
    e->n_band_items = n_items;
    e->last_ksplit = p_max;
    e->last_round_items = 0;
    e->last_pair_items[0] = e->last_pair_items[1] = e->last_pair_items[2] = 0;
    e->last_tail_ksplit = 1;
    e->last_band_kernel = NLDSC_BAND_F4_KSPLIT;
    HIPCHK(e->gram.ensure(std::max<size_t>(units, 1) * 8192));
    const nldsc::BandArgs a = fill_band_args(e, p, s, m);
    const nldsc::AnnotArgs aa = annot_args(e, s, an);
    // the annotated epilogue reads the replayed constants of the KC items: the whole band waits for the replay
    if (s.replay) HIPCHK(hipStreamWaitEvent(st, e->ev_replay, 0));
    for (const nldsc::AnnotBatch& b : batches)
        HIPCHK(nldsc::launch_band_f4_annot(a, aa, b.ksplit, e->items.p + b.first, b.n, e->gram.p));
    e->last_path = s.path;
    HIPCHK(hipEventRecord(e->ev[4], st));
    HIPCHK(e->sums.ensure(3));
    HIPCHK(e->h_sums.ensure(3 * sizeof(unsigned long long)));
    HIPCHK(hipStreamWaitEvent(cs, e->ev[3], 0));
    HIPCHK(hipMemsetAsync(e->sums.p + 2, 0, sizeof(unsigned long long), cs));
    HIPCHK(nldsc::launch_issued_products(e->items.p, n_items, nullptr, 0, m.gpu_plan ? e->plan_rows.p : nullptr,
                                         e->blk_miss.p, s.nblk, s.path, s.dom, 0, m.route_shift, e->sums.p + 2, cs));
    HIPCHK(hipMemcpyAsync(e->h_sums.p + 2 * sizeof(unsigned long long), e->sums.p + 2, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, cs));
    HIPCHK(hipEventRecord(e->ev_issued, cs));
    return NLDSC_OK;
}

// The band of a covariate run (ev[3] .. ev[4]): the single-block items in batches (as an annotated band's) through the
// K-split partial kernel and the covariate epilogue (launch_band_f4_cov); no replay to wait for (prepare_cov's run
// takes the closed-form vectors); then the issued-product count as enqueue_band queues it.
int enqueue_band_cov(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m,
                     const Schedule& sc, const CovRun& cv, char* err, size_t errlen) {
    hipStream_t st = e->stream, cs = e->copy_stream;
    const int n_items = sc.n_items;
    HIPCHK(hipEventRecord(e->ev[3], st));
    const std::vector<nldsc::AnnotBatch> batches = nldsc::plan_annot_batches(
        n_items, s.n_it, e->n_cu, e->ksplit_ok, e->cov_batch_items, nldsc::ANNOT_GRAM_CAP_BYTES);
    size_t units = 0;
    int p_max = 1;
    for (const nldsc::AnnotBatch& b : batches) {
        units = std::max(units, (size_t)b.n * (size_t)b.ksplit);
        p_max = std::max(p_max, b.ksplit);
    }
    e->n_band_items = n_items;
    e->last_ksplit = p_max;
    e->last_round_items = 0;
    e->last_pair_items[0] = e->last_pair_items[1] = e->last_pair_items[2] = 0;
    e->last_tail_ksplit = 1;
    e->last_band_kernel = NLDSC_BAND_F4_KSPLIT;
    HIPCHK(e->gram.ensure(std::max<size_t>(units, 1) * 8192));
    const nldsc::BandArgs a = fill_band_args(e, p, s, m);
    const nldsc::CovArgs ca = cov_args(e, s, cv);
    for (const nldsc::AnnotBatch& b : batches)
        HIPCHK(nldsc::launch_band_f4_cov(a, ca, b.ksplit, e->items.p + b.first, b.n, e->gram.p));
    e->last_path = s.path;
    HIPCHK(hipEventRecord(e->ev[4], st));
    HIPCHK(e->sums.ensure(3));
    HIPCHK(e->h_sums.ensure(3 * sizeof(unsigned long long)));
    HIPCHK(hipStreamWaitEvent(cs, e->ev[3], 0));
    HIPCHK(hipMemsetAsync(e->sums.p + 2, 0, sizeof(unsigned long long), cs));
    HIPCHK(nldsc::launch_issued_products(e->items.p, n_items, nullptr, 0, m.gpu_plan ? e->plan_rows.p : nullptr,
                                         e->blk_miss.p, s.nblk, s.path, s.dom, 0, m.route_shift, e->sums.p + 2, cs));
    HIPCHK(hipMemcpyAsync(e->h_sums.p + 2 * sizeof(unsigned long long), e->sums.p + 2, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, cs));
    HIPCHK(hipEventRecord(e->ev_issued, cs));
    return NLDSC_OK;
}

// The band of a dom-dom run (ev[3] .. ev[4]): the single-block items in batches (as an annotated band's, sized for
// units of nine tiles) through the K-split partial kernel with the h.h product and the dom-dom epilogue
// (launch_band_f4_dd); no replay to wait for (the run takes the closed-form vectors); then the issued-product count
// as enqueue_band queues it, one more product per item.
int enqueue_band_dd(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m,
                    const Schedule& sc, char* err, size_t errlen) {
    hipStream_t st = e->stream, cs = e->copy_stream;
    const int n_items = sc.n_items;
    HIPCHK(hipEventRecord(e->ev[3], st));
    const size_t unit = nldsc::DD_GRAM_UNIT;
    const std::vector<nldsc::AnnotBatch> batches = nldsc::plan_annot_batches(
        n_items, s.n_it, e->n_cu, e->ksplit_ok, e->annot_batch_items, nldsc::ANNOT_GRAM_CAP_BYTES, unit * sizeof(float));
    size_t units = 0;
    int p_max = 1;
    for (const nldsc::AnnotBatch& b : batches) {
        units = std::max(units, (size_t)b.n * (size_t)b.ksplit);
        p_max = std::max(p_max, b.ksplit);
    }
    e->n_band_items = n_items;
    e->last_ksplit = p_max;
    e->last_round_items = 0;
    e->last_pair_items[0] = e->last_pair_items[1] = e->last_pair_items[2] = 0;
    e->last_tail_ksplit = 1;
    e->last_band_kernel = NLDSC_BAND_F4_KSPLIT;
    HIPCHK(e->gram.ensure(std::max<size_t>(units, 1) * unit));
    const nldsc::BandArgs a = fill_band_args(e, p, s, m);
    for (const nldsc::AnnotBatch& b : batches)
        HIPCHK(nldsc::launch_band_f4_dd(a, b.ksplit, e->items.p + b.first, b.n, e->gram.p, e->l2dd_acc.p));
    e->last_path = s.path;
    HIPCHK(hipEventRecord(e->ev[4], st));
    HIPCHK(e->sums.ensure(3));
    HIPCHK(e->h_sums.ensure(3 * sizeof(unsigned long long)));
    HIPCHK(hipStreamWaitEvent(cs, e->ev[3], 0));
    HIPCHK(hipMemsetAsync(e->sums.p + 2, 0, sizeof(unsigned long long), cs));
    HIPCHK(nldsc::launch_issued_products(e->items.p, n_items, nullptr, 0, m.gpu_plan ? e->plan_rows.p : nullptr,
                                         e->blk_miss.p, s.nblk, s.path, s.dom, 0, m.route_shift, e->sums.p + 2, cs,
                                         true));
    HIPCHK(hipMemcpyAsync(e->h_sums.p + 2 * sizeof(unsigned long long), e->sums.p + 2, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, cs));
    HIPCHK(hipEventRecord(e->ev_issued, cs));
    return NLDSC_OK;
}

// A pairs run's request (nldsc_engine_run_pairs): the filter, the caller's CSR arrays and their capacity; `emitted`:
// the table is in the device buffers, to be copied out once the stream is drained
struct PairsRun {
    double min_r2;
    int64_t* row_ptr;
    int32_t* k;
    double *r, *rd;
    int64_t cap;
    int64_t* n_pairs;
    bool emitted;
};

// The restrictions of a pairs run, each with its reason (those of an annotated run: the same two kernels' inputs).
int prepare_pairs(const nldsc_ld_params* p, const RunShape& s, const PairsRun& pr, bool annot, char* err,
                  size_t errlen) {
    if (!pr.row_ptr || !pr.n_pairs) return set_err(err, errlen, NLDSC_E_ARG, "row_ptr or n_pairs is NULL");
    if (pr.cap < 0) return set_err(err, errlen, NLDSC_E_ARG, "negative capacity %lld", (long long)pr.cap);
    if (pr.k && pr.cap > 0 && (!pr.r || !pr.rd)) return set_err(err, errlen, NLDSC_E_ARG, "r or rd is NULL beside k");
    if (annot) return set_err(err, errlen, NLDSC_E_ARG, "annotations and a pair table in one run are not supported");
    if (p->n_org >= (1 << 19))
        return set_err(err, errlen, NLDSC_E_ARG,
                       "pairs runs need n_org < 2^19 (got %d): the K-split partial kernel takes unsegmented rows",
                       p->n_org);
    if (s.path != 2)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "pairs runs take the exact fp4 path only: this run's flags or the band_mode option select %s",
                       s.path == 0 ? "fp32" : "exact int8");
    return NLDSC_OK;
}

// The band of a pairs run (ev[3] .. ev[4]): after the rare-variant replay, the single-block items in batches (as an
// annotated band's) through the K-split partial kernel and the count pass of the pairs epilogue, which also adds the
// ordinary sums; the row scan, the row lengths to the host, row_ptr and the pair count there; then, when the caller's
// arrays hold the table, the emit pass over the same batches — their Gram tiles computed again unless one batch held
// the whole band.  The host waits for the stream twice (the window width, the row lengths).
int enqueue_band_pairs(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m,
                       const Schedule& sc, PairsRun& pr, char* err, size_t errlen) {
    hipStream_t st = e->stream, cs = e->copy_stream;
    const int n_items = sc.n_items, n_own = s.own_end - s.own_begin;
    HIPCHK(hipEventRecord(e->ev[3], st));
    const std::vector<nldsc::AnnotBatch> batches = nldsc::plan_annot_batches(
        n_items, s.n_it, e->n_cu, e->ksplit_ok, e->pairs_batch_items, nldsc::PAIRS_GRAM_CAP_BYTES);
    size_t units = 0;
    int p_max = 1;
    for (const nldsc::AnnotBatch& b : batches) {
        units = std::max(units, (size_t)b.n * (size_t)b.ksplit);
        p_max = std::max(p_max, b.ksplit);
    }
    e->n_band_items = n_items;
    e->last_ksplit = p_max;
    e->last_round_items = 0;
    e->last_pair_items[0] = e->last_pair_items[1] = e->last_pair_items[2] = 0;
    e->last_tail_ksplit = 1;
    e->last_band_kernel = NLDSC_BAND_F4_KSPLIT;
    HIPCHK(e->gram.ensure(std::max<size_t>(units, 1) * 8192));
    const nldsc::BandArgs a = fill_band_args(e, p, s, m);
    // the widest window of the owned range in blocks, from the device's pointers
    HIPCHK(e->pairs_len.ensure((size_t)n_own + 1));
    int Wb = 1;
    HIPCHK(nldsc::launch_pairs_window_blocks(e->Lw.p, e->Rw.p, s.own_begin, s.own_end, e->pairs_len.p + n_own, st));
    HIPCHK(hipMemcpyAsync(&Wb, e->pairs_len.p + n_own, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t max_cells = e->pairs_max_cells > 0 ? e->pairs_max_cells : nldsc::PAIRS_MAX_CELLS;
    if (Wb < 1 || (int64_t)n_own * Wb > max_cells)
        return set_err(err, errlen, NLDSC_E_ARG,
                       "the count matrix of %d owned SNPs x %d window blocks exceeds %lld cells: narrow the owned range "
                       "to at most %lld SNPs", n_own, Wb, (long long)max_cells, (long long)(max_cells / std::max(Wb, 1)));
    const size_t cells = (size_t)n_own * (size_t)Wb;
    HIPCHK(e->pairs_cnt.ensure(cells));
    HIPCHK(hipMemsetAsync(e->pairs_cnt.p, 0, sizeof(int) * cells, st));
    nldsc::PairsArgs pa = {e->pairs_cnt.p, Wb, nullptr, 0, nullptr, nullptr, nullptr, pr.min_r2,
                           e->oriented ? e->flip.p : nullptr, e->counts.p};
    // the epilogue reads the replayed constants of the KC items: the whole band waits for the replay
    if (s.replay) HIPCHK(hipStreamWaitEvent(st, e->ev_replay, 0));
    for (const nldsc::AnnotBatch& b : batches)
        HIPCHK(nldsc::launch_band_f4_pairs(a, pa, b.ksplit, e->items.p + b.first, b.n, e->gram.p, false, true));
    HIPCHK(nldsc::launch_pairs_row_scan(e->pairs_cnt.p, Wb, n_own, e->pairs_len.p, st));
    e->h_pairs_len.resize((size_t)n_own);
    HIPCHK(hipMemcpyAsync(e->h_pairs_len.data(), e->pairs_len.p, sizeof(int) * (size_t)n_own, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t total = 0;
    for (int j = 0; j < n_own; ++j) {
        pr.row_ptr[j] = total;
        total += e->h_pairs_len[(size_t)j];
    }
    pr.row_ptr[n_own] = total;
    *pr.n_pairs = total;
    if (pr.k && total <= pr.cap && total > 0) {
        const size_t T = (size_t)total;
        HIPCHK(e->pairs_ptr.ensure((size_t)n_own + 1));
        HIPCHK(e->pairs_k.ensure(T));
        HIPCHK(e->pairs_val.ensure(2 * T));
        HIPCHK(hipMemcpyAsync(e->pairs_ptr.p, pr.row_ptr, sizeof(int64_t) * ((size_t)n_own + 1), hipMemcpyHostToDevice, st));
        pa.row_ptr = e->pairs_ptr.p, pa.n_pairs = total, pa.k = e->pairs_k.p, pa.r = e->pairs_val.p;
        pa.rd = e->pairs_val.p + T;
        for (const nldsc::AnnotBatch& b : batches)
            HIPCHK(nldsc::launch_band_f4_pairs(a, pa, b.ksplit, e->items.p + b.first, b.n, e->gram.p, true,
                                               batches.size() > 1));
        pr.emitted = true;
    }
    e->last_path = s.path;
    HIPCHK(hipEventRecord(e->ev[4], st));
    HIPCHK(e->sums.ensure(3));
    HIPCHK(e->h_sums.ensure(3 * sizeof(unsigned long long)));
    HIPCHK(hipStreamWaitEvent(cs, e->ev[3], 0));
    HIPCHK(hipMemsetAsync(e->sums.p + 2, 0, sizeof(unsigned long long), cs));
    HIPCHK(nldsc::launch_issued_products(e->items.p, n_items, nullptr, 0, m.gpu_plan ? e->plan_rows.p : nullptr,
                                         e->blk_miss.p, s.nblk, s.path, s.dom, 0, m.route_shift, e->sums.p + 2, cs));
    HIPCHK(hipMemcpyAsync(e->h_sums.p + 2 * sizeof(unsigned long long), e->sums.p + 2, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, cs));
    HIPCHK(hipEventRecord(e->ev_issued, cs));
    return NLDSC_OK;
}

// The band on the main stream (ev[3] .. ev[4]): the super-item launch, the wait for the compacted count, the
// single-block launches, the KC launches after the replay (ev_replay), or the fp32 launch; then the issued-product
// count on the side stream (ev_issued).
int enqueue_band(nldsc_engine* e, const nldsc_ld_params* p, const RunShape& s, const PlanMode& m, const Schedule& sc,
                 char* err, size_t errlen, const AnnotRun* an = nullptr, PairsRun* pr = nullptr,
                 const CovRun* cv = nullptr, const DomDomRun* dd = nullptr) {
    if (dd) return enqueue_band_dd(e, p, s, m, sc, err, errlen);
    if (cv) return enqueue_band_cov(e, p, s, m, sc, *cv, err, errlen);
    if (an) return enqueue_band_annot(e, p, s, m, sc, *an, err, errlen);
    if (pr) return enqueue_band_pairs(e, p, s, m, sc, *pr, err, errlen);
    hipStream_t st = e->stream, cs = e->copy_stream;
    const int n_items = sc.n_items;
    HIPCHK(hipEventRecord(e->ev[3], st));
    e->n_band_items = n_items;
    e->last_ksplit = sc.ksplit;
    e->last_band_kernel = nldsc::band_kernel_code(sc.use_t2, e->t2_mode, s.path, sc.ksplit, s.n_it);
    if (sc.ksplit > 1) HIPCHK(e->gram.ensure((size_t)n_items * sc.ksplit * 8192));
    const nldsc::BandArgs a = fill_band_args(e, p, s, m);
    // (column-block pair items: the compaction keeps an item while one of its blocks is unrouted, the kernel drops
    // the other)
    const uint8_t* single_miss = sc.use_t2 && m.routed && (!sc.compact || m.nc2) ? e->blk_miss.p : nullptr;
    SingleLaunch L = {e->items.p, n_items, {}, single_miss};
    const bool exact = n_items > 0 && (s.use_f4 || s.use_i8);
    const bool run_single = !sc.use_t2 || m.routed;  // (option t2 = 2: every block pair in the 2 x 2 workgroups)
    if (exact && sc.use_t2) HIPCHK(launch_super(e, a, m, sc.n_items2, 1));
    if (exact && e->debug_timing) HIPCHK(hipEventRecord(e->ev_dbg[0], st));
    const auto t_wait0 = Clock::now();
    if (exact && sc.compact) {  // the super-item kernel is queued: the host waits for the compacted count meanwhile
        // (polling the pinned word the copy lands in: a blocking event wait wakes the thread tens of
        // microseconds late, time the GPU would idle when the super-item kernel has nothing to do)
        volatile int* cnt = reinterpret_cast<volatile int*>(e->h_route.p);
        (void)spin_until_nonneg(cnt);
        HIPCHK(hipEventSynchronize(e->ev_route));  // (returns at once when the count has landed)
        L.n = *cnt;
        L.items = e->items_u.p;
    }  // (routed without compaction: every item listed, the routed ones return at once)
    // the single-block launches sized by their own work (nldsc::shape_single), and their buffers
    L.shape = nldsc::shape_single(L.n, s.n_it, e->n_cu, s.use_f4, sc.ksplit, e->band_rounds, m.nc2, e->ksplit_ok,
                                  s.replay && e->defer_rep, e->rep_gram_max_slots);
    e->last_round_items = L.shape.round_items;
    e->last_pair_items[0] = e->last_pair_items[1] = e->last_pair_items[2] = 0;
    e->last_tail_ksplit = L.shape.tail_p;
    if (L.shape.defer && L.shape.n_full > 0) {
        const size_t slots = (size_t)L.shape.n_full * (m.nc2 ? 2 : 1);
        HIPCHK(e->rep_gram.ensure(slots * 8192));
        HIPCHK(e->rep_items.ensure(slots));
    }
    if (L.shape.tail_p > 1) HIPCHK(e->gram.ensure((size_t)(L.n - L.shape.n_full) * L.shape.tail_p * 8192));
    // add+dom column-pair rounds: the host waits for the two counts of the pair plan (as for the compacted count) and
    // shapes the launches; with fewer pairs than the rounds need, the single-block plan runs as shaped above
    nldsc::ColpairShape cp = {};
    const int4 *cp_pairs = nullptr;
    int4* cp_rest = nullptr;
    const uint8_t* cp_miss = nullptr;
    int n_cp_pairs = 0, n_cp_singles = 0;
    // (routed runs: every kept pair holds an unrouted single block, so fewer of those than the rounds need pairs —
    // missing-free data leaves none — settles it without the pair lists)
    const int cp_round = e->colpair_round_items > 0 ? e->colpair_round_items : 4 * e->n_cu;
    const bool cp_possible = !sc.use_t2 || (int64_t)L.n >= (int64_t)(e->colpair_round_items > 0 ? 1 : nldsc::COLPAIR_ROUND_MIN) * cp_round;
    if (exact && sc.colpair && cp_possible) {
        volatile int* tot = reinterpret_cast<volatile int*>(e->h_meta.p) + 8;
        (void)spin_until_nonneg(tot);
        (void)spin_until_nonneg(tot + 1);
        HIPCHK(hipEventSynchronize(e->ev_route));
        cp_pairs = e->items_p.p, cp_rest = e->items_s.p, n_cp_pairs = tot[0], n_cp_singles = tot[1];
        if (sc.use_t2 && n_cp_pairs > 0) {
            // routed: both lists compacted in order on the plan stream (idle by now; the super-item kernel runs
            // meanwhile), so the rounds are sized by the pairs that keep a block; the main stream waits for the lists
            hipStream_t ps = e->plan_stream;
            const size_t cp_chunks = ((size_t)n_cp_pairs + 255) / 256, cs_chunks = ((size_t)n_cp_singles + 255) / 256;
            HIPCHK(e->items_pu.ensure((size_t)n_items));
            HIPCHK(e->items_su.ensure((size_t)n_items));
            HIPCHK(e->compact_tmp2.ensure(cp_chunks + cs_chunks + 2));
            int* tp = e->compact_tmp2.p;
            int* ts = tp + cp_chunks + 1;
            tot[2] = tot[3] = -1;
            HIPCHK(nldsc::launch_compact_items(cp_pairs, n_cp_pairs, e->blk_miss.p, m.route_shift, s.nblk, tp,
                                               tp + cp_chunks, e->items_pu.p, ps));
            HIPCHK(nldsc::launch_compact_items(cp_rest, n_cp_singles, e->blk_miss.p, m.route_shift, s.nblk, ts,
                                               ts + cs_chunks, e->items_su.p, ps));
            HIPCHK(hipMemcpyAsync(e->h_meta.p + 10 * sizeof(int), tp + cp_chunks, sizeof(int), hipMemcpyDeviceToHost, ps));
            HIPCHK(hipMemcpyAsync(e->h_meta.p + 11 * sizeof(int), ts + cs_chunks, sizeof(int), hipMemcpyDeviceToHost, ps));
            HIPCHK(hipEventRecord(e->ev_route, ps));
            (void)spin_until_nonneg(tot + 2);
            (void)spin_until_nonneg(tot + 3);
            HIPCHK(hipEventSynchronize(e->ev_route));
            HIPCHK(hipStreamWaitEvent(st, e->ev_route, 0));
            cp_pairs = e->items_pu.p, cp_rest = e->items_su.p, n_cp_pairs = tot[2], n_cp_singles = tot[3];
            cp_miss = e->blk_miss.p;
        }
        cp = nldsc::shape_colpair(n_cp_pairs, n_cp_singles, s.n_it, e->n_cu, e->colpair_round_items, e->ksplit_ok,
                                  s.replay && e->defer_rep, e->rep_gram_max_slots);
    }
    const bool colpair = cp.round_items > 0;
    const int ksplit = colpair ? 1 : sc.ksplit;
    if (colpair) {
        const nldsc::SingleShape& rs = cp.rest;
        e->last_ksplit = 1;
        e->last_band_kernel = nldsc::band_kernel_code(false, e->t2_mode, s.path, 1, s.n_it, true);
        e->last_round_items = 2 * cp.round_items;  // (in block pairs, the unit of band_items)
        e->last_pair_items[0] = cp.n_pair_full, e->last_pair_items[1] = n_cp_pairs, e->last_pair_items[2] = cp.n_rest;
        e->last_tail_ksplit = rs.tail_p;
        if (rs.defer) {
            const size_t slots = (size_t)cp.n_pair_full * 2 + (size_t)rs.n_full;
            HIPCHK(e->rep_gram.ensure(std::max<size_t>(slots, 1) * 8192));
            HIPCHK(e->rep_items.ensure(std::max<size_t>(slots, 1)));
        }
        if (rs.tail_p > 1) HIPCHK(e->gram.ensure((size_t)(cp.n_rest - rs.n_full) * rs.tail_p * 8192));
        // the pairs past the last full round, as single blocks behind the leftover singles
        HIPCHK(nldsc::launch_expand_pairs(cp_pairs + cp.n_pair_full, n_cp_pairs - cp.n_pair_full,
                                          cp_rest + n_cp_singles, st));
    }
    const auto t_wait1 = Clock::now();
    if (exact) {
        if (e->debug_timing) HIPCHK(hipEventRecord(e->ev_dbg[1], st));
        if (colpair) HIPCHK(launch_colpair(e, a, cp, cp_pairs, cp_rest, cp_miss, 1));
        else if (run_single) HIPCHK(launch_single(e, a, s, m, ksplit, L, 1));
        if (e->debug_timing) {
            HIPCHK(hipStreamSynchronize(st));
            float t_super = 0, t_gap = 0;
            HIPCHK(hipEventElapsedTime(&t_super, e->ev[3], e->ev_dbg[0]));
            HIPCHK(hipEventElapsedTime(&t_gap, e->ev_dbg[0], e->ev_dbg[1]));
            std::fprintf(stderr, "[nldsc debug] super %.3f ms, gap to single %.3f ms, host wait %.3f ms, n_single %d/%d\n",
                         t_super, t_gap, ms_between(t_wait0, t_wait1), L.n, n_items);
        }
    }
    if (s.replay) {  // the KC launches, and the fp32 path, read the replayed tables
        HIPCHK(hipStreamWaitEvent(st, e->ev_replay, 0));
        if (exact && sc.use_t2) HIPCHK(launch_super(e, a, m, sc.n_items2, 2));
        if (exact && colpair) HIPCHK(launch_colpair(e, a, cp, cp_pairs, cp_rest, cp_miss, 2));
        else if (exact && run_single) HIPCHK(launch_single(e, a, s, m, ksplit, L, 2));
    }
    if (n_items > 0 && !s.use_f4 && !s.use_i8) HIPCHK(nldsc::launch_band(a, 2, e->items.p, n_items));
    e->last_path = s.path;
    HIPCHK(hipEventRecord(e->ev[4], st));
    // matrix-core products the band kernels issued, counted on the GPU per work item as each kernel decides them
    // (missing-free blocks skip the m products, diagonal blocks the transposed ones, routed items run in the 2 x 2
    // kernel): sums[2], counted beside the band on the copy stream (after the work lists: ev[3]) and landed in
    // h_sums[2] (ev_issued); sums[0..1] are the device-table run's pair counts
    HIPCHK(e->sums.ensure(3));
    HIPCHK(e->h_sums.ensure(3 * sizeof(unsigned long long)));
    HIPCHK(hipStreamWaitEvent(cs, e->ev[3], 0));
    HIPCHK(hipMemsetAsync(e->sums.p + 2, 0, sizeof(unsigned long long), cs));
    HIPCHK(nldsc::launch_issued_products(L.items, run_single ? L.n : 0, sc.use_t2 ? e->items2.p : nullptr, sc.n_items2,
                                         m.gpu_plan ? e->plan_rows.p : nullptr, s.use_f4 ? e->blk_miss.p : nullptr,
                                         s.nblk, s.path, s.dom,
                                         (sc.use_t2 && m.routed ? 2 : 0) | (L.miss != nullptr ? 1 : 0), m.route_shift,
                                         e->sums.p + 2, cs));
    HIPCHK(hipMemcpyAsync(e->h_sums.p + 2 * sizeof(unsigned long long), e->sums.p + 2, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, cs));
    HIPCHK(hipEventRecord(e->ev_issued, cs));
    return NLDSC_OK;
}

// ms[0..3] of a run: count, statistics (GPU events), the host's wait for the schedule, the band (GPU events)
int record_band_timings(nldsc_engine* e, double host_plan_ms, char* err, size_t errlen) {
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, e->ev[0], e->ev[1])); e->ms[0] = f;
    HIPCHK(hipEventElapsedTime(&f, e->ev[1], e->ev[2])); e->ms[1] = f;
    e->ms[2] = host_plan_ms;
    HIPCHK(hipEventElapsedTime(&f, e->ev[3], e->ev[4])); e->ms[3] = f;
    return NLDSC_OK;
}

// the metrics of a run from its pair counts (sw = sum of positive WSA, sd = of WSD) and h_sums[2] (products issued)
void record_metrics(nldsc_engine* e, double sw, double sd, int N, int row_bytes) {
    e->flop_issued = (double)reinterpret_cast<const unsigned long long*>(e->h_sums.p)[2] * 2.0 * BLK * BLK *
                     (double)row_bytes * 4.0;
    e->pairs = sw;
    // BASELINE.md metric: FLOP_alg = 2N(1/2 sum WSA + sum WSD); additive-only 2N * 1/2 sum WSA
    e->flop_alg = 2.0 * (double)N * (0.5 * sw + sd);
    // exact formulation: 4 integer dot products per unordered additive pair (xx, xo, ox, oo) and
    // 2 per ordered dominance pair (xh, oh): 2N (4 * 1/2 sum WSA + 2 sum WSD) int8 ops
    e->ops_alg_i8 = 2.0 * (double)N * (2.0 * sw + 2.0 * sd);
}

// Device-table runs (e->split names the table): the owned slice stays on the device (the caller gathers it device to
// device); only the pair counts of the metric come back.  Finalize (.. ev[5]), pack, the sums copy, and the sync.
int finish_table(nldsc_engine* e, double* sw, double* sd, char* err, size_t errlen) {
    const nldsc_engine::SplitState& t = e->split;
    hipStream_t st = e->stream;
    HIPCHK(nldsc::launch_finalize(e->Lw.p, e->l2_acc.p, e->l2d_acc.p, e->ws_acc.p, t.M, t.own_lo, t.own_hi, t.dom,
                                  e->l2.p, e->l2d.p, e->ws3.p, st));
    HIPCHK(hipEventRecord(e->ev[5], st));
    HIPCHK(hipMemsetAsync(e->sums.p, 0, 2 * sizeof(unsigned long long), st));
    HIPCHK(nldsc::launch_pack_table(e->l2.p, e->l2d.p, e->maf.p, e->rstd.p, e->ws3.p, t.M, t.own_lo, t.own_hi, t.width,
                                    t.table, e->sums.p, st));
    HIPCHK(hipMemcpyAsync(e->h_sums.p, e->sums.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const unsigned long long* sums = reinterpret_cast<const unsigned long long*>(e->h_sums.p);
    *sw = (double)sums[0];
    *sd = t.dom ? (double)sums[1] : 0.0;
    return NLDSC_OK;
}

// Host results: finalize writes the owned slice's seven columns straight into host memory (o.d) with its
// per-workgroup pair-count sums — no pack kernel, no copy engine (the runtime moves device-to-pinned copies
// with blit kernels: a 0.6 MB RSTD copy beside the C2 band took ~1 ms of its CU slots); without `direct`, the
// host copies them from the landing buffer to the caller's arrays.
int finish_host(nldsc_engine* e, const RunShape& s, const HostOut& o, double* sw, double* sd, char* err,
                size_t errlen) {
    hipStream_t st = e->stream;
    HIPCHK(nldsc::launch_finalize_out(e->Lw.p, e->l2_acc.p, e->l2d_acc.p, e->ws_acc.p, e->maf.p, e->rstd.p, s.M,
                                      s.own_begin, s.own_end, s.dom, o.d.l2, o.d.l2d, o.d.maf, o.d.rstd, o.d.wsa,
                                      o.d.wsd, o.d.wsde, o.wsum_d, st));
    HIPCHK(hipEventRecord(e->ev[5], st));
    const auto t0 = Clock::now();
    HIPCHK(hipStreamSynchronize(st));
    const auto t1 = Clock::now();
    if (!o.direct) {
        const CopyPool::Seg segs[7] = {{o.callers.l2, o.h.l2, o.b8},     {o.callers.l2d, o.h.l2d, o.b8},
                                       {o.callers.maf, o.h.maf, o.b8},   {o.callers.rstd, o.h.rstd, o.b8},
                                       {o.callers.wsa, o.h.wsa, o.b4},   {o.callers.wsd, o.h.wsd, o.b4},
                                       {o.callers.wsde, o.h.wsde, o.b4}};
        e->copies.copy(segs, 7);
    }
    unsigned long long ta = 0, td = 0;
    for (int b = 0; b < o.n_wsum; ++b) {
        ta += o.wsum_h[2 * b];
        td += o.wsum_h[2 * b + 1];
    }
    *sw = (double)ta;
    *sd = s.dom ? (double)td : 0.0;
    if (e->debug_timing)
        std::fprintf(stderr, "[nldsc debug] host results (%s): band wait %.3f, copies and sums %.3f ms\n",
                     o.direct ? "direct" : "landing buffer", ms_between(t0, t1), ms_between(t1, Clock::now()));
    return NLDSC_OK;
}

// The hot path of one run.  Results go to the host arrays of `r`, or (table_dev != nullptr) stay in device memory
// as the owned slice of the score table (nldsc_engine_run_device).
// Split runs (nldsc_engine_run_device_split, export_n != nullptr): only the pairs whose lower SNP is owned are computed,
// the per-SNP sums of every SNP of the slice accumulate, the right halo's [own_end, M) go out to export_dev and the run
// stops before finalize; nldsc_engine_run_device_finish adds the left neighbour's export and finishes.
int run_impl(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end, nldsc_ld_result* r,
             double* table_dev, int32_t width, char* err, size_t errlen, long long* export_dev = nullptr,
             int32_t export_cap = 0, int32_t* export_n = nullptr, const AnnotRun* an = nullptr,
             PairsRun* pr = nullptr, const CovRun* cv = nullptr, const DomDomRun* dd = nullptr) {
    const bool split = export_n != nullptr;
    int rc = 0;
    if (dd && e && p && (rc = check_dd(e, p, *dd, an != nullptr || pr != nullptr || cv != nullptr, err, errlen)))
        return rc;
    rc = check_run_args(e, p, own_begin, own_end, r, table_dev, width, split, export_dev, export_cap, err, errlen);
    if (rc) return rc;
    if (cv && (rc = prepare_cov(e, p, run_shape(e, p, own_begin, own_end, split), *cv, an != nullptr || pr != nullptr,
                                err, errlen)))
        return rc;
    if (an && (rc = prepare_annot(e, p, run_shape(e, p, own_begin, own_end, split), *an, err, errlen))) return rc;
    if (pr && (rc = prepare_pairs(p, run_shape(e, p, own_begin, own_end, split), *pr, an != nullptr, err, errlen)))
        return rc;
    if (pr && own_begin == own_end) pr->row_ptr[0] = *pr->n_pairs = 0;
    if (own_begin == own_end) return run_nothing_owned(e, p->n_snp, own_begin, table_dev, width, err, errlen);
    HIPCHK(hipSetDevice(e->device));
    HostOut out = {};
    e->last_direct = -1;
    if (!table_dev && (rc = resolve_host_out(e, r, own_begin, own_end, &out, err, errlen))) return rc;
    const RunShape s = run_shape(e, p, own_begin, own_end, split);
    const PlanMode m = plan_mode(e, p, s, an != nullptr || pr != nullptr || cv != nullptr || dd != nullptr);
    if ((rc = ensure_run_buffers(e, s, m, err, errlen))) return rc;
    if (dd && (rc = prepare_dd(e, s, err, errlen))) return rc;

    const auto t_start = Clock::now();
    if ((rc = enqueue_prologue(e, p, s, m, err, errlen, cv))) return rc;
    // ---- window replay + schedule ----
    const auto t_host0 = Clock::now();
    Schedule sc;
    rc = m.gpu_plan ? schedule_on_gpu(e, s, m, &sc, err, errlen) : schedule_on_host(e, p, s, m, &sc, err, errlen);
    if (rc) return rc;
    // (l2_acc, l2d_acc and ws_acc were zeroed by snp_stats_kernel)
    const auto t_host1 = Clock::now();
    if ((rc = enqueue_band(e, p, s, m, sc, err, errlen, an, pr, cv, dd))) return rc;
    if (dd)  // L2DD of the owned slice, finalized beside the ordinary scores (.. ev[5])
        HIPCHK(nldsc::launch_finalize_dd(e->Lw.p, e->l2dd_acc.p, e->ws_acc.p, e->sflags.p, s.M, own_begin, own_end,
                                         e->l2dd_out.p, e->stream));
    if (an) {  // the per-annotation scores of the owned slice, finalized beside the ordinary ones (.. ev[5])
        double* o2 = e->annot_out.p;
        HIPCHK(nldsc::launch_finalize_annot(e->Lw.p, e->ws_acc.p, annot_args(e, s, *an), s.M, own_begin, own_end, s.dom,
                                            o2, an->l2d ? o2 + (size_t)an->n * (own_end - own_begin) : nullptr,
                                            e->stream));
    }

    if (table_dev) e->split = {false, s.M, s.N, s.row_bytes, width, own_begin, own_end, s.dom, table_dev, 0.0};
    if (split) {  // the right halo's sums out; finalize waits for the left neighbour's (run_device_finish)
        HIPCHK(nldsc::launch_export_acc(e->l2_acc.p, e->l2d_acc.p, e->ws_acc.p, s.M, own_end, s.M, export_dev,
                                        e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        *export_n = s.M - own_end;
        if ((rc = record_band_timings(e, ms_between(t_host0, t_host1), err, errlen))) return rc;
        e->split.ms1 = ms_between(t_start, Clock::now());
        e->split.pending = true;
        return NLDSC_OK;
    }
    double sw = 0, sd = 0;
    rc = table_dev ? finish_table(e, &sw, &sd, err, errlen) : finish_host(e, s, out, &sw, &sd, err, errlen);
    if (rc) return rc;
    if (an) {  // (the stream is drained) rows of the owned slice into the caller's [n_annot][M] arrays
        const size_t n_own = (size_t)(own_end - own_begin), row = sizeof(double) * n_own;
        HIPCHK(hipMemcpy2D(an->l2 + own_begin, sizeof(double) * (size_t)s.M, e->annot_out.p, row, row, (size_t)an->n,
                           hipMemcpyDeviceToHost));
        if (an->l2d)
            HIPCHK(hipMemcpy2D(an->l2d + own_begin, sizeof(double) * (size_t)s.M, e->annot_out.p + (size_t)an->n * n_own,
                               row, row, (size_t)an->n, hipMemcpyDeviceToHost));
    }
    if (dd)  // (the stream is drained) the owned slice into the caller's array
        HIPCHK(hipMemcpy(dd->l2dd + own_begin, e->l2dd_out.p, sizeof(double) * (size_t)(own_end - own_begin),
                         hipMemcpyDeviceToHost));
    if (pr && pr->emitted) {  // (the stream is drained) the table into the caller's arrays
        const size_t T = (size_t)*pr->n_pairs;
        HIPCHK(hipMemcpy(pr->k, e->pairs_k.p, sizeof(int32_t) * T, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pr->r, e->pairs_val.p, sizeof(double) * T, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pr->rd, e->pairs_val.p + T, sizeof(double) * T, hipMemcpyDeviceToHost));
    }
    {
        const auto t0 = Clock::now();
        HIPCHK(hipEventSynchronize(e->ev_issued));
        if (e->debug_timing)
            std::fprintf(stderr, "[nldsc debug] issued-count wait %.3f ms\n", ms_between(t0, Clock::now()));
    }
    const auto t_end = Clock::now();

    if ((rc = record_band_timings(e, ms_between(t_host0, t_host1), err, errlen))) return rc;
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, e->ev[4], e->ev[5])); e->ms[4] = f;
    e->ms[5] = ms_between(t_start, t_end);
    if (e->debug_timing) {  // where a run's wall time goes: GPU stages, the gap before the band, host tail
        float g23 = 0, g05 = 0;
        HIPCHK(hipEventElapsedTime(&g23, e->ev[2], e->ev[3]));
        HIPCHK(hipEventElapsedTime(&g05, e->ev[0], e->ev[5]));
        std::fprintf(stderr, "[nldsc debug] count %.3f stats %.3f gap-to-band %.3f band %.3f finalize %.3f | GPU span %.3f, "
                     "host total %.3f (host wait for the plan %.3f)\n", e->ms[0], e->ms[1], g23, e->ms[3], e->ms[4], g05,
                     e->ms[5], e->ms[2]);
    }
    record_metrics(e, sw, sd, s.N, s.row_bytes);
    if (cv) e->cov_n = cv->n, e->cov_M = s.M;  // (the projections of this run are on the device)
    return NLDSC_OK;
}

}  // namespace

extern "C" {

int nldsc_engine_run(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                     nldsc_ld_result* r, char* err, size_t errlen) {
    if (!r) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    return run_impl(e, p, own_begin, own_end, r, nullptr, 0, err, errlen);
}

int nldsc_engine_run_annot(nldsc_engine* e, const nldsc_ld_params* p, const double* annot, int32_t n_annot,
                           int32_t own_begin, int32_t own_end, nldsc_ld_result* r, double* l2_annot,
                           double* l2d_annot, char* err, size_t errlen) {
    if (!r) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    const AnnotRun an = {annot, n_annot, l2_annot, l2d_annot};
    return run_impl(e, p, own_begin, own_end, r, nullptr, 0, err, errlen, nullptr, 0, nullptr, &an);
}

int nldsc_engine_run_pairs(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                           nldsc_ld_result* r, double min_r2, int64_t* row_ptr, int32_t* k, double* rv, double* rdv,
                           int64_t cap, int64_t* n_pairs, char* err, size_t errlen) {
    if (!r) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    PairsRun pr = {min_r2, row_ptr, k, rv, rdv, cap, n_pairs, false};
    const int rc = run_impl(e, p, own_begin, own_end, r, nullptr, 0, err, errlen, nullptr, 0, nullptr, nullptr, &pr);
    if (rc) return rc;
    if (*n_pairs > 0 && !pr.emitted)
        return set_err(err, errlen, NLDSC_E_SPACE, "the pair table needs room for %lld pairs (capacity %lld)",
                       (long long)*n_pairs, (long long)(k ? cap : 0));
    return NLDSC_OK;
}

int nldsc_engine_run_covar(nldsc_engine* e, const nldsc_ld_params* p, const double* q_basis, int32_t n_covar,
                           int32_t own_begin, int32_t own_end, nldsc_ld_result* r, char* err, size_t errlen) {
    if (!r || !p) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    // the closed-form vectors of rare variants: the reference's fp32 rounding is not replayed for a model it lacks
    nldsc_ld_params q = *p;
    q.flags |= NLDSC_FLAG_EXACT_RARE;
    const CovRun cv = {q_basis, n_covar};
    return run_impl(e, &q, own_begin, own_end, r, nullptr, 0, err, errlen, nullptr, 0, nullptr, nullptr, nullptr, &cv);
}

int nldsc_engine_run_domdom(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                            nldsc_ld_result* r, double* l2dd, char* err, size_t errlen) {
    if (!r || !p) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    // the closed-form vectors of rare variants: the new statistic has no reference arithmetic to replay
    nldsc_ld_params q = *p;
    q.flags |= NLDSC_FLAG_EXACT_RARE;
    const DomDomRun dd = {l2dd};
    return run_impl(e, &q, own_begin, own_end, r, nullptr, 0, err, errlen, nullptr, 0, nullptr, nullptr, nullptr,
                    nullptr, &dd);
}

int nldsc_engine_covar_projections(nldsc_engine* e, double* u, double* w, double* v, double* wd) {
    if (!e || e->cov_n == 0) return NLDSC_E_ARG;
    if (hipSetDevice(e->device) != hipSuccess) return NLDSC_E_HIP;
    const size_t M = (size_t)e->cov_M, qm = (size_t)e->cov_n * M;
    hipError_t he = hipSuccess;
    if (u) he = hipMemcpy(u, e->cov_uw.p, sizeof(double) * qm, hipMemcpyDeviceToHost);
    if (he == hipSuccess && w) he = hipMemcpy(w, e->cov_uw.p + qm, sizeof(double) * qm, hipMemcpyDeviceToHost);
    if (he == hipSuccess && v) he = hipMemcpy(v, e->cov_sc.p + 3 * M, sizeof(double) * M, hipMemcpyDeviceToHost);
    if (he == hipSuccess && wd) he = hipMemcpy(wd, e->cov_sc.p + 4 * M, sizeof(double) * M, hipMemcpyDeviceToHost);
    if (he == hipSuccess && u && e->oriented) {  // the file's allele coding: a row stored flipped has U negated
        std::vector<uint8_t> fl(M);
        he = hipMemcpy(fl.data(), e->flip.p, M, hipMemcpyDeviceToHost);
        for (size_t c = 0; he == hipSuccess && c < (size_t)e->cov_n; ++c)
            for (size_t j = 0; j < M; ++j)
                if (fl[j]) u[c * M + j] = -u[c * M + j];
    }
    return he == hipSuccess ? NLDSC_OK : NLDSC_E_HIP;
}

int nldsc_engine_run_device(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                            double* table_dev, int32_t width, char* err, size_t errlen) {
    if (!table_dev) return set_err(err, errlen, NLDSC_E_ARG, "NULL table");
    return run_impl(e, p, own_begin, own_end, nullptr, table_dev, width, err, errlen);
}

int nldsc_engine_run_device_split(nldsc_engine* e, const nldsc_ld_params* p, int32_t own_begin, int32_t own_end,
                                  double* table_dev, int32_t width, int64_t* export_dev, int32_t export_cap,
                                  int32_t* export_n, char* err, size_t errlen) {
    if (!table_dev || !export_n) return set_err(err, errlen, NLDSC_E_ARG, "NULL table or export count");
    return run_impl(e, p, own_begin, own_end, nullptr, table_dev, width, err, errlen,
                    reinterpret_cast<long long*>(export_dev), export_cap, export_n);
}

int nldsc_engine_run_device_finish(nldsc_engine* e, const int64_t* import_dev, int32_t import_n, char* err,
                                   size_t errlen) {
    if (!e) return set_err(err, errlen, NLDSC_E_ARG, "NULL engine");
    if (!e->split.pending) return set_err(err, errlen, NLDSC_E_ARG, "no split run to finish");
    const int32_t own = e->split.own_hi - e->split.own_lo;
    if (import_n < 0 || import_n > own || (import_n > 0 && !import_dev))
        return set_err(err, errlen, NLDSC_E_ARG, "import of %d SNPs into an owned range of %d", import_n, own);
    e->split.pending = false;
    HIPCHK(hipSetDevice(e->device));
    const auto t0 = Clock::now();
    HIPCHK(nldsc::launch_import_acc(e->l2_acc.p, e->l2d_acc.p, e->ws_acc.p, e->split.M, e->split.own_lo, import_n,
                                    reinterpret_cast<const long long*>(import_dev), e->stream));
    HIPCHK(hipEventRecord(e->ev[4], e->stream));
    double sw = 0, sd = 0;
    const int rc = finish_table(e, &sw, &sd, err, errlen);
    if (rc) return rc;
    HIPCHK(hipEventSynchronize(e->ev_issued));  // (h_sums[2]: the first call's issued-product count)
    float f = 0;
    HIPCHK(hipEventElapsedTime(&f, e->ev[4], e->ev[5])); e->ms[4] = f;
    // (total: both calls' host time, without the exchange between them)
    e->ms[5] = e->split.ms1 + ms_between(t0, Clock::now());
    record_metrics(e, sw, sd, e->split.N, e->split.row_bytes);
    return NLDSC_OK;
}

int nldsc_engine_timings(const nldsc_engine* e, double* ms6, double* flop_alg, double* flop_issued,
                         double* pairs, int32_t* n_band_items) {
    if (!e) return NLDSC_E_ARG;
    if (ms6) for (int k = 0; k < 6; ++k) ms6[k] = e->ms[k];
    if (flop_alg) *flop_alg = e->flop_alg;
    if (flop_issued) *flop_issued = e->flop_issued;
    if (pairs) *pairs = e->pairs;
    if (n_band_items) *n_band_items = e->n_band_items;
    return NLDSC_OK;
}

int nldsc_engine_path(const nldsc_engine* e, int32_t* exact_i8, double* ops_alg_i8) {
    if (!e) return NLDSC_E_ARG;
    if (exact_i8) *exact_i8 = e->last_path;
    if (ops_alg_i8) *ops_alg_i8 = e->ops_alg_i8;
    return NLDSC_OK;
}

int nldsc_engine_ksplit(const nldsc_engine* e) { return e ? e->last_ksplit : NLDSC_E_ARG; }
int nldsc_engine_band_round_items(const nldsc_engine* e) { return e ? e->last_round_items : NLDSC_E_ARG; }
int nldsc_engine_band_tail_ksplit(const nldsc_engine* e) { return e ? e->last_tail_ksplit : NLDSC_E_ARG; }
int nldsc_engine_band_pair_items(const nldsc_engine* e, int32_t out[3]) {
    if (!e || !out) return NLDSC_E_ARG;
    for (int k = 0; k < 3; ++k) out[k] = e->last_pair_items[k];
    return NLDSC_OK;
}
int nldsc_engine_band_kernel(const nldsc_engine* e) { return e ? e->last_band_kernel : NLDSC_E_ARG; }

int nldsc_engine_result_direct(const nldsc_engine* e) { return e ? e->last_direct : NLDSC_E_ARG; }

int nldsc_ld_calculate(const nldsc_ld_params* p, nldsc_ld_result* r, char* err, size_t errlen) {
    if (!p || !r || !p->bedfile) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    nldsc_engine* e = nullptr;
    int rc = nldsc_engine_create(p->device, &e, err, errlen);
    if (rc) return rc;
    rc = nldsc_engine_load_bed_file(e, p->bedfile, p->n_snp, p->n_org, err, errlen);
    if (!rc) rc = nldsc_engine_run(e, p, 0, p->n_snp, r, err, errlen);
    nldsc_engine_destroy(e);
    return rc;
}

int nldsc_ld_calculate_keep(const nldsc_ld_params* p, const int32_t* idx, int32_t n_keep, nldsc_ld_result* r,
                            char* err, size_t errlen) {
    if (!p || !r || !p->bedfile) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    nldsc_engine* e = nullptr;
    int rc = nldsc_engine_create(p->device, &e, err, errlen);
    if (rc) return rc;
    rc = nldsc_engine_set_keep(e, idx, n_keep, p->n_org, err, errlen);
    if (!rc) rc = nldsc_engine_load_bed_file(e, p->bedfile, p->n_snp, p->n_org, err, errlen);
    if (!rc) {
        nldsc_ld_params q = *p;
        q.n_org = e->n_org;  // the kept count (p->n_org without a list)
        rc = nldsc_engine_run(e, &q, 0, p->n_snp, r, err, errlen);
    }
    nldsc_engine_destroy(e);
    return rc;
}

int nldsc_ld_calculate_annot(const nldsc_ld_params* p, const int32_t* keep_idx, int32_t n_keep, const double* annot,
                             int32_t n_annot, nldsc_ld_result* r, double* l2_annot, double* l2d_annot, char* err,
                             size_t errlen) {
    if (!p || !r || !p->bedfile) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    nldsc_engine* e = nullptr;
    int rc = nldsc_engine_create(p->device, &e, err, errlen);
    if (rc) return rc;
    if (keep_idx) rc = nldsc_engine_set_keep(e, keep_idx, n_keep, p->n_org, err, errlen);
    if (!rc) rc = nldsc_engine_load_bed_file(e, p->bedfile, p->n_snp, p->n_org, err, errlen);
    if (!rc) {
        nldsc_ld_params q = *p;
        q.n_org = e->n_org;  // the kept count (p->n_org without a list)
        rc = nldsc_engine_run_annot(e, &q, annot, n_annot, 0, p->n_snp, r, l2_annot, l2d_annot, err, errlen);
    }
    nldsc_engine_destroy(e);
    return rc;
}

int nldsc_ld_calculate_covar(const nldsc_ld_params* p, const int32_t* keep_idx, int32_t n_keep, const double* q_basis,
                             int32_t n_covar, nldsc_ld_result* r, char* err, size_t errlen) {
    if (!p || !r || !p->bedfile) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    nldsc_engine* e = nullptr;
    int rc = nldsc_engine_create(p->device, &e, err, errlen);
    if (rc) return rc;
    if (keep_idx) rc = nldsc_engine_set_keep(e, keep_idx, n_keep, p->n_org, err, errlen);
    if (!rc) rc = nldsc_engine_load_bed_file(e, p->bedfile, p->n_snp, p->n_org, err, errlen);
    if (!rc) {
        nldsc_ld_params q = *p;
        q.n_org = e->n_org;  // the kept count (p->n_org without a list)
        q.flags |= NLDSC_FLAG_STRICT_PLINK_ORDER;  // (q_basis rows are .fam lines)
        rc = nldsc_engine_run_covar(e, &q, q_basis, n_covar, 0, p->n_snp, r, err, errlen);
    }
    nldsc_engine_destroy(e);
    return rc;
}

int nldsc_ld_calculate_domdom(const nldsc_ld_params* p, const int32_t* keep_idx, int32_t n_keep, nldsc_ld_result* r,
                              double* l2dd, char* err, size_t errlen) {
    if (!p || !r || !p->bedfile) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    nldsc_engine* e = nullptr;
    int rc = nldsc_engine_create(p->device, &e, err, errlen);
    if (rc) return rc;
    if (keep_idx) rc = nldsc_engine_set_keep(e, keep_idx, n_keep, p->n_org, err, errlen);
    if (!rc) rc = nldsc_engine_load_bed_file(e, p->bedfile, p->n_snp, p->n_org, err, errlen);
    if (!rc) {
        nldsc_ld_params q = *p;
        q.n_org = e->n_org;  // the kept count (p->n_org without a list)
        rc = nldsc_engine_run_domdom(e, &q, 0, p->n_snp, r, l2dd, err, errlen);
    }
    nldsc_engine_destroy(e);
    return rc;
}

int nldsc_synth_bed_device(int32_t device, void* bed_dev, int32_t n_snp, int32_t n_org, const float* thr_host,
                           float rho, float missing, uint64_t seed, char* err, size_t errlen) {
    if (!bed_dev || !thr_host) return set_err(err, errlen, NLDSC_E_ARG, "NULL argument");
    int rc = check_dims(n_snp, n_org, err, errlen);
    if (rc) return rc;
    int d = 0;
    rc = use_device(device, &d, err, errlen);
    if (rc) return rc;
    const int nb = n_org / 4 + (n_org % 4 > 0);
    float* thr = nullptr;
    HIPCHK(hipMalloc(&thr, sizeof(float) * n_snp));
    hipError_t he = hipMemcpy(thr, thr_host, sizeof(float) * n_snp, hipMemcpyHostToDevice);
    const uint8_t magic[3] = {0x6c, 0x1b, 0x01};
    if (he == hipSuccess) he = hipMemcpy(bed_dev, magic, 3, hipMemcpyHostToDevice);
    if (he == hipSuccess)
        he = nldsc::launch_synth_bed((uint8_t*)bed_dev + 3, n_snp, n_org, nb, thr, rho, missing, seed, nullptr);
    if (he == hipSuccess) he = hipDeviceSynchronize();
    (void)hipFree(thr);
    if (he != hipSuccess) return set_err(err, errlen, NLDSC_E_HIP, "HIP error %s in synth", hipGetErrorString(he));
    return NLDSC_OK;
}

}  // extern "C"
