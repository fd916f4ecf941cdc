"""The GPU band schedule at production SNP counts, on short rows.

The schedule (ld_kernels.hip plan_*: window edges, right pointers, per-row-block offset ranges, tile counts, their
prefix scans, the items, the super-item plans and the routed-item compaction) depends on the positions, the owned range
and M only, never on the row length.  With N = 67 a row is one 64-byte pitch (n_it == 2: no K-split, no round launches),
so a 100 000-SNP wide band is milliseconds of GPU time and the single-workgroup scans (chunked_scan_excl, `per` values
per thread) run multi-chunk: more than 256 scan tiles, more than 256 tile counts, more than 65 536 items to compact.

Truth that depends on no plan: for sorted positions the window counts WSA / WSD of every SNP are closed-form from the
positions and the oracle's per-SNP pass flags (window_counts); they change whenever a block pair is dropped or run
twice.  On top of that a set of target SNPs at the edges the scans split at is compared with oracle.run_f64_targets, the
option sets with each other, and band_items with a vectorised restatement of the schedule (schedule_restated; the
quadratic test_plan.gpu_schedule_restated is its reference at small n).

The tests without the gpu mark check the helpers and that every geometry really reaches the sizes it is here for, from
the restatement alone.

The add+dom column-pair plan (plan_*_split, expand_pairs_kernel, the second compaction of its two lists under routing,
launch_colpair) runs on the same geometries through the engine option colpair_round_items at the production round of
4 pairs per CU: on these short rows the option stands in for the row-length gate only (test_gpu_colpair_long.py runs
the gate itself), the rounds, the list sizes and the launches are production's.  The lists' sizes as the engine
reports them (nldsc_engine_band_pair_items) are held to the restatement (split_totals, split_kept).

Out of scope: K-split, round launches of the single-block kernel and segmented rows (long rows: test_gpu_parity.py,
test_gpu_saturation.py), unsorted or negative positions (the host plan), split-halo runs.
"""
import functools
import os

import numpy as np
import pytest

from conftest import assert_ld_close
from oracle import oracle as O
from test_gpu_parity import MODES, _lib_flag, missing_free_blocks, same_gram
from test_plan import covered, gpu_schedule_restated

N_ORG = 67                    # N % 4 == 3; 17 bytes -> one 64-byte row pitch, n_it == 2
MAF, STD_THR = 0.05, 1e-5     # p ~ U(0.02, 0.5): a real share of SNPs fails MAF 0.05 at N = 67
EXACT = dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12), residuals_std=(1e-12, 1e-10), maf=(0.0, 0.0))  # the exact-path bar
RSQ_GAP = 1e-9                # no target pair's exact r2d within this of rsq_thr: WSDE compared exactly
PLAN_WG, PLAN_SMALL_WG, PLAN_SMALL_N = 256, 1024, 32768  # ld_kernels.hip / ld_kernels.h
THREADS = min(16, len(os.sched_getaffinity(0)))

# name: (M, what it is here for)
GEOMS = {
    "fused_full": 32_768,    # the fused plan at capacity: 1 024 blocks, 64 x 64 tile counts, every block pair
    "chain_first": 32_769,   # the first chain size: 1 025 blocks, the last of 1 SNP
    "narrow_65k": 65_537,    # 257 scan tiles: plan_tile_scan's first per == 2
    "wide_100k": 100_003,    # ~8 tile columns: plan_scan / plan_qscan / scan_counts multi-chunk, q_rounds
    "ragged_100k": 100_003,  # density 100-fold apart, gaps beyond the window, long tie runs, exact window ties
}
OWNED = ["wide_100k", "ragged_100k"]


def own_ranges(M):
    return [(M // 3 + 5, 2 * M // 3 - 7), (M - 1, M), (0, 1)]


# ---------------------------------------------------------------------------------------------------------------
# helpers: closed-form window counts, the schedule restated, the genotype generator
# ---------------------------------------------------------------------------------------------------------------

def window_edges(pos, w):
    """(A, E) of sorted non-negative positions: A[j] = the first k <= j with pos_j - pos_k <= w, E[j] = the first
    k > j with pos_k - pos_j > w (n: none).  searchsorted on pos -+ w proposes, the two predicates the engine and the
    oracle evaluate decide (pos + w rounds differently from pos_k - pos_j)."""
    pos = np.asarray(pos, np.float64)
    n = len(pos)
    assert n > 0 and pos[0] >= 0 and (np.diff(pos) >= 0).all()
    j = np.arange(n)
    E = np.maximum(np.searchsorted(pos, pos + w, side="right"), j + 1)
    while True:  # up while SNP E is still inside the window
        m = E < n
        m[m] = ~(pos[E[m]] - pos[j[m]] > w)
        if not m.any():
            break
        E[m] += 1
    while True:  # down while SNP E - 1 is already outside
        m = E - 1 > j
        m[m] = pos[E[m] - 1] - pos[j[m]] > w
        if not m.any():
            break
        E[m] -= 1
    A = np.minimum(np.searchsorted(pos, pos - w, side="left"), j)
    while True:
        m = A > 0
        m[m] = pos[j[m]] - pos[A[m] - 1] <= w
        if not m.any():
            break
        A[m] -= 1
    while True:
        m = A < j
        m[m] = ~(pos[j[m]] - pos[A[m]] <= w)
        if not m.any():
            break
        A[m] += 1
    return A, E


def window_counts(pos, passed, rpass, w):
    """(WSA, WSD) of every SNP, -1 where it is not computed (it fails MAF): the MAF-passing SNPs of its window
    [A_j, E_j) but itself, and those of them with a residual."""
    A, E = window_edges(pos, w)
    passed = np.asarray(passed, bool)
    pd = passed & np.asarray(rpass, bool)
    cp = np.concatenate([[0], np.cumsum(passed)])
    cd = np.concatenate([[0], np.cumsum(pd)])
    wsa = np.where(passed, cp[E] - cp[A] - 1, -1).astype(np.int32)
    wsd = np.where(passed, cd[E] - cd[A] - pd, -1).astype(np.int32)
    return wsa, wsd


def _ceil(a, b):
    return -(-a // b)


def _split_pieces(d0, d1):
    """Per 16-offset tile column c: (a, b, run) of every row's piece [a, b] of its offsets [d0, d1] (run 0: none)."""
    top = int(np.where(d0 <= d1, d1 + 1, 0).max(initial=0))
    for c in range(_ceil(top, 16)):
        a, b = np.maximum(d0, 16 * c), np.minimum(d1, 16 * c + 15)
        yield a, b, np.where(a <= b, b - a + 1, 0)


def split_totals(d0, d1):
    """(pairs, singles, odd pieces per row) of the add+dom split plan on these row ranges."""
    pairs, singles, odd = 0, 0, np.zeros(len(d0), np.int64)
    for _, _, run in _split_pieces(d0, d1):
        pairs += int((run // 2).sum())
        singles += int((run & 1).sum())
        odd += run & 1
    return pairs, singles, odd


def blocks_with_missing(rows, n_org):
    """bool per 32-SNP block: it holds a missing call among the slots the reference reads (the engine's blk_miss;
    test_gpu_parity.missing_free_blocks counts the others)."""
    rows = np.asarray(rows, np.uint8)
    M, nb = rows.shape
    miss = np.stack([((rows >> (2 * k)) & 3) == 1 for k in range(4)], axis=-1)
    r = n_org % 4
    keep = [k >= 4 - r for k in range(4)] if r else [True] * 4
    row_miss = miss[:, :nb - 1, :].any(axis=(1, 2)) | miss[:, nb - 1, keep].any(axis=1)
    pad = np.zeros(_ceil(M, 32) * 32, bool)
    pad[:M] = row_miss
    return pad.reshape(-1, 32).any(axis=1)


def split_kept(s, blk_miss, shift=2):
    """(pairs, singles) the routing compaction keeps of the split plan's lists (ld_kernels.hip keep_item): block pair
    (I, J) is routed to the super-item kernel when the 2^shift (clamped) blocks of its super-row and of its
    super-column are all missing-free; a pair stays while one of its two block pairs is unrouted, a single while its
    own is."""
    nblk, F = s["nblk"], 1 << shift
    g = np.arange(_ceil(nblk, F))
    free = ~np.stack([blk_miss[np.minimum(F * g + k, nblk - 1)] for k in range(F)]).any(axis=0)
    I = np.arange(nblk)

    def routed(J):
        return free[I >> shift] & free[np.clip(J, 0, nblk - 1) >> shift]
    pairs = singles = 0
    for a, b, run in _split_pieces(s["d0"], s["d1"]):
        for k in range(8):
            d = a + 2 * k
            pairs += int(((d + 1 <= b) & (run > 0) & ~(routed(I + d) & routed(I + d + 1))).sum())
        singles += int((((run & 1) == 1) & ~routed(I + b)).sum())
    return pairs, singles


def schedule_restated(pos, w, own=None):
    """The GPU schedule (ld_kernels.hip plan_edges / plan_right / plan_rows and the kernels counting on their rows)
    restated on whole arrays: edges A, E, right pointers R, per row block the useful offsets [d0, d1] (d0 > d1: none),
    and from them the sizes every scan of the plan sees."""
    n = len(pos)
    own = (0, n) if own is None else own
    A, E = window_edges(pos, w)
    j = np.arange(n)
    R = np.minimum(n - 1, j + np.maximum.accumulate(E - j))
    nblk = _ceil(n, 32)
    I = np.arange(nblk)
    jmax = np.minimum(nblk - 1, (E[np.minimum(n, 32 * I + 32) - 1] - 1) // 32)
    ob0, ob1 = own[0] // 32, (own[1] - 1) // 32
    own_row = (I >= ob0) & (I <= ob1)
    J0 = np.where(own_row, I, np.maximum(I, ob0))
    J1 = np.where(own_row, jmax, np.minimum(jmax, ob1))
    active = (I >= A[own[0]] // 32) & (32 * I < own[1]) & (J0 <= J1)
    d0, d1 = np.where(active, J0 - I, 1), np.where(active, J1 - I, 0)
    s = dict(n=n, nblk=nblk, A=A, E=E, R=R, d0=d0, d1=d1)
    s["items"] = int(np.maximum(0, d1 - d0 + 1).sum())
    maxd = int((d1 + 1)[active].max(initial=0))
    s["tile_counts"] = _ceil(nblk, 16) * _ceil(maxd, 16)          # plan_count / plan_scan: 16 x 16 tiles
    pair = 0                                                      # additive-only: (I, J, 2) items, cut at tile edges
    for c in range(_ceil(maxd, 16)):
        a, b = np.maximum(d0, 16 * c), np.minimum(d1, 16 * c + 15)
        pair += int(np.where(a <= b, (b - a + 2) // 2, 0).sum())
    s["pair_items"] = pair
    # add+dom (plan_count_split / plan_emit_split): each row's run in a tile column split into floor(run / 2) pairs
    # (I, J, 2) and, for an odd run, one single; odd_pieces: per row, its pieces of odd length
    s["split_pairs"], s["split_singles"], s["odd_pieces"] = split_totals(d0, d1)
    for shift, key, tr, tc in ((1, "t2", 16, 16), (2, "quad", 4, 8)):  # plan_rows2 and its count kernels
        F = 1 << shift
        nblk2 = _ceil(nblk, F)
        lo = np.full(nblk2 * F, np.iinfo(np.int64).max)
        hi = np.full(nblk2 * F, -1)
        lo[:nblk][active], hi[:nblk][active] = (I + d0)[active], (I + d1)[active]
        lo, hi = lo.reshape(nblk2, F).min(1), hi.reshape(nblk2, F).max(1)
        some = hi >= 0
        I2 = np.arange(nblk2)
        e0, e1 = np.where(some, (lo >> shift) - I2, 1), np.where(some, (hi >> shift) - I2, 0)
        s[key + "_rows"] = (e0, e1)
        s[key + "_items"] = int(np.maximum(0, e1 - e0 + 1).sum())
        s[key + "_counts"] = _ceil(nblk2, tr) * _ceil(int((e1 + 1)[some].max(initial=0)), tc)
    return s


def scan_sizes(s, fused):
    """name -> (values scanned, values per thread) of every single-workgroup scan a run on this schedule does."""
    wg = PLAN_SMALL_WG if fused else PLAN_WG
    right = s["n"] if fused else _ceil(s["n"], PLAN_WG)  # fused: the SNPs themselves; chain: the scan tiles' maxima
    sizes = {"right_pointer": right, "tile_counts": s["tile_counts"]}
    out = {k: (v, _ceil(v, wg)) for k, v in sizes.items()}
    for k, v in (("quad_counts", s["quad_counts"]), ("t2_counts", s["t2_counts"]),
                 ("compact_chunks", _ceil(s["items"], 256)), ("compact_chunks_pair", _ceil(s["pair_items"], 256))):
        out[k] = (v, _ceil(v, PLAN_WG))
    return out


def block_pairs(s):
    return {(int(I), int(I + d)) for I in range(s["nblk"]) for d in range(s["d0"][I], s["d1"][I] + 1)}


@functools.lru_cache(maxsize=None)
def _clean_genotypes(M, N, seed, rho=0.9):
    from scipy.signal import lfilter
    from scipy.special import ndtri
    rng = np.random.default_rng(seed)
    thr = ndtri(rng.uniform(0.02, 0.5, size=M))[:, None]
    x = rng.standard_normal((M, 2 * N))
    x[1:] *= np.sqrt(1.0 - rho ** 2)
    z = lfilter([1.0], [1.0, -rho], x, axis=0)  # z_j = rho z_{j-1} + sqrt(1 - rho^2) e_j along the SNP axis
    g = (z[:, :N] < thr).astype(np.int8) + (z[:, N:] < thr).astype(np.int8)
    g.setflags(write=False)
    return g


def fast_genotypes(M, N, seed, missing=None):
    """int8 genotypes [M][N] of the project's model (nldsc_amd.synth: p ~ U(0.02, 0.5), two haplotypes thresholding a
    latent AR(1) process over SNPs, rho = 0.9), the recursion run as a filter along the SNP axis.  missing: a rate
    (calls set missing independently: every 32-SNP block gets some), None (no missing call), or "mixed4" (20 missing
    calls in one SNP of every third group of four blocks, as test_gpu_parity.T2_CASES)."""
    g = _clean_genotypes(M, N, seed).copy()
    rng = np.random.default_rng(seed + 77)
    if missing == "mixed4":
        for b in range(0, _ceil(M, 128), 3):
            g[128 * b + rng.integers(0, min(128, M - 128 * b)), rng.choice(N, 20, replace=False)] = -1
    elif missing:
        g[rng.random(g.shape) < missing] = -1
    return g


# ---------------------------------------------------------------------------------------------------------------
# geometries and data sets (built once per process, shared by every case)
# ---------------------------------------------------------------------------------------------------------------

def _ragged_positions(M, w, rng):
    """Clusters (30 bp per SNP) and deserts (3 000 bp per SNP) in turn; jumps of 3 w (one before a block edge, two
    around a single SNP); 230 SNPs at one position across a 256-SNP tile edge; exact ties pos_b = pos_a + w."""
    gaps = np.empty(M)
    k, cluster = 0, True
    while k < M:
        n = int(rng.integers(4000, 9000) if cluster else rng.integers(300, 1500))
        gaps[k:k + n] = np.round(rng.exponential(30.0 if cluster else 3000.0, size=len(gaps[k:k + n])))
        k, cluster = k + n, not cluster
    lone = 50_001
    for at in (32 * 1000, lone, lone + 1, 32 * 2500 + 7):
        gaps[at] = 3 * w
    pos = np.cumsum(gaps)
    run = (256 * 100 - 40, 256 * 100 + 190)
    pos[run[0]:run[1]] = pos[run[0]]
    ties = []
    for a in (1234, 20_000, 61_003, 90_001):
        b = int(np.searchsorted(pos, pos[a] + w, side="left"))
        if b < M and pos[b] - pos[a] < 2 * w:  # (not across one of the jumps)
            pos[b] = pos[a] + w
            ties.append((a, b))
    assert (np.diff(pos) >= 0).all() and len(ties) >= 2
    return pos, dict(tie_run=run, ties=ties, lone=lone)


@functools.lru_cache(maxsize=None)
def geometry(name):
    """dict(M, pos, w, ...): integer-valued bp positions (float64), sorted, with ties."""
    M = GEOMS[name]
    rng = np.random.default_rng(sorted(GEOMS).index(name) + 4000)
    extra = {}
    if name in ("fused_full", "chain_first"):
        pos = np.cumsum(rng.integers(0, 600, size=M)).astype(np.float64)
        w = float(pos[-1])  # the window holds the whole chromosome
    elif name == "narrow_65k":
        pos = np.cumsum(rng.integers(0, 201, size=M)).astype(np.float64)
        w = 28_500.0        # ~285 neighbours a side
    elif name == "wide_100k":
        pos = np.cumsum(np.round(rng.exponential(288.0, size=M)))
        w = 1.0e6           # ~3 470 neighbours a side
    else:
        w = 1.0e5
        pos, extra = _ragged_positions(M, w, rng)
    pos.setflags(write=False)
    return dict(M=M, pos=pos, w=w, **extra)


@functools.lru_cache(maxsize=None)
def restated(name, own=None):
    g = geometry(name)
    return schedule_restated(g["pos"], g["w"], own)


def target_snps(name):
    """>= 64 SNPs: both edges of blocks and of 256-SNP scan tiles, the first and last tile of scan chunks (plan_tile_scan:
    `per` tiles per thread), block 1 024's edge, the chromosome ends, the owned ranges' ends, a tie run, the interior."""
    g = geometry(name)
    M, pos = g["M"], g["pos"]
    ntile = _ceil(M, PLAN_WG)
    chunk = PLAN_WG * _ceil(ntile, PLAN_WG)  # SNPs in one thread's chunk of scan tiles
    last_blk, last_tile = 32 * ((M - 1) // 32), 256 * ((M - 1) // 256)
    t = {0, 1, 31, 32, 255, 256, M - 2, M - 1, last_blk - 1, last_blk, last_tile - 1, last_tile, 32767, 32768,
         M // 3 + 4, M // 3 + 5, 2 * M // 3 - 8, 2 * M // 3 - 7}
    n_chunk = _ceil(M, chunk)
    for c in sorted({1, 2, n_chunk // 4, n_chunk // 2, 3 * n_chunk // 4, n_chunk - 2, n_chunk - 1}):
        s = c * chunk
        t |= {s - 256, s - 1, s, s + 255, s + chunk - 256, s + chunk - 1}
    if "tie_run" in g:
        a, b = g["tie_run"]
        t |= {a - 1, a, (a + b) // 2, b - 1, b, g["lone"] - 1, g["lone"], g["lone"] + 1}
        t |= {x for ab in g["ties"] for x in ab}
    else:
        k = int(np.flatnonzero(np.diff(pos) == 0)[5])
        t |= {k, k + 1}
    t |= set(np.random.default_rng(M).choice(M, 56, replace=False).tolist())
    t = np.array(sorted(x for x in t if 0 <= x < M), np.int64)
    assert len(t) >= 64
    return t


class Data:
    """One data set of a geometry: rows, the oracle's per-SNP half, the closed-form counts; the targets' truth and
    the rsq_thr it is valid for on demand."""

    def __init__(self, name, missing):
        from nldsc_amd import synth
        g = geometry(name)
        self.name, self.missing, self.M, self.pos, self.w = name, missing, g["M"], g["pos"], g["w"]
        geno = fast_genotypes(self.M, N_ORG, seed=sorted(GEOMS).index(name) + 10,
                              missing={"rate": 0.02, "none": None, "mixed4": "mixed4"}[missing])
        self.rows = synth.pack_bed_rows(geno)
        self.bed = synth.bed_bytes(self.rows)
        O.code_counts(self.bed, self.M, N_ORG, threads=THREADS)  # (sets the team size of the oracle's C helpers)
        self.setup = O.f64_setup(self.rows, N_ORG, self.w, MAF, STD_THR, self.pos, bed=self.bed)
        self.passed, self.rpass = self.setup["passed"], self.setup["rpass"]
        self.maf = self.setup["st"]["maf"].astype(np.float64)
        self.wsa, self.wsd = window_counts(self.pos, self.passed, self.rpass, self.w)
        self.free = missing_free_blocks(self.rows, N_ORG)
        self.targets = target_snps(name)
        self._truth = None

    def truth(self):
        """(rsq_thr, oracle.run_f64_targets at the targets): rsq_thr is the first of 0.01, 0.010001, ... that no
        target pair's exact r2d comes within 10 RSQ_GAP of, so the WSDE comparison needs no tie budget."""
        if self._truth is None:
            args = (self.rows, N_ORG, self.w, MAF, STD_THR)
            pairs = O.pair_r2_f64(*args, self.pos, self.targets, bed=self.bed, setup=self.setup)
            r2d = np.concatenate([p[3] for p in pairs if p is not None])
            rsq = next(c for c in 0.01 + 1e-6 * np.arange(100) if np.abs(r2d - c).min(initial=1.0) > 10 * RSQ_GAP)
            assert np.abs(r2d - rsq).min(initial=1.0) > RSQ_GAP
            exp = O.run_f64_targets(*args, rsq, self.pos, self.targets, bed=self.bed, setup=self.setup)
            self._truth = (float(rsq), exp)
        return self._truth


@functools.lru_cache(maxsize=None)
def dataset(name, missing):
    return Data(name, missing)


@pytest.fixture(scope="module")
def data():
    """dataset(name, missing) -> Data, built once and shared by the GPU cases of this module."""
    import torch
    torch.cuda.init()  # before libnldsc_amd.so binds to a HIP runtime (tests/test_gpu_parity.py)
    yield dataset
    for f in (dataset, restated, geometry, _clean_genotypes):
        f.cache_clear()


# ---------------------------------------------------------------------------------------------------------------
# CPU self-checks
# ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(4))
def test_window_counts_equal_run_f64(seed):
    """The closed form equals the oracle's per-pair loop at every SNP: cM positions (rounding of pos +- w matters) and
    integer bp positions with ties, more than 5 % of the SNPs failing MAF."""
    rng = np.random.default_rng(300 + seed)
    M = int(rng.integers(400, 701))
    from nldsc_amd import synth
    rows = synth.pack_bed_rows(fast_genotypes(M, N_ORG, seed, missing=0.02))
    if seed % 2:
        pos, w = np.cumsum(rng.integers(0, 4, size=M)).astype(np.float64), float(rng.choice([7.0, 40.0]))
        assert (np.diff(pos) == 0).any()
    else:
        pos, w = np.cumsum(rng.exponential(0.02, size=M)), float(rng.choice([0.1, 1.0]))
        for a in (M // 5, M // 2):  # pos_b = fl(pos_a + w): whether pos_b - pos_a <= w is the predicate's to decide
            pos[np.searchsorted(pos, pos[a] + w)] = pos[a] + w
    maf = 0.08  # (above the geometries' 0.05: at least 5 % of these few hundred SNPs fail it whatever the seed)
    exp = O.run_f64(rows, N_ORG, w, maf, STD_THR, 0.01, pos)
    s = O.f64_setup(rows, N_ORG, w, maf, STD_THR, pos)
    assert (~s["passed"]).mean() >= 0.05
    wsa, wsd = window_counts(pos, s["passed"], s["rpass"], w)
    np.testing.assert_array_equal(wsa, exp["l2_ws"])
    np.testing.assert_array_equal(wsd, exp["l2d_ws"])
    assert (wsd < wsa).any()


def _emit_loops(d0, d1, nblk, pair):
    """plan_count / plan_emit as loops: the items of every 16 x 16 tile, row by row."""
    items = []
    n_c = _ceil(int(max((b + 1 for a, b in zip(d0, d1) if a <= b), default=0)), 16)
    for T in range(_ceil(nblk, 16)):
        for c in range(n_c):
            for I in range(16 * T, min(nblk, 16 * T + 16)):
                a, b = max(d0[I], 16 * c), min(d1[I], 16 * c + 15)
                for d in range(a, b + 1, 1 + pair):
                    items.append((I, I + d, min(2, b - d + 1) if pair else 1, 0))
    return items


@pytest.mark.parametrize("seed", range(5))
def test_restatement_equals_quadratic_restatement(seed):
    """schedule_restated equals test_plan.gpu_schedule_restated (A, R, the block-pair set) for whole runs and owned
    ranges, its pair-item count the tile loops', its super-item rows plan_rows2 as a loop."""
    rng = np.random.default_rng(900 + seed)
    n = int(rng.integers(40, 700))
    pos = np.cumsum(rng.exponential(0.02, n))
    if seed % 2:
        pos = np.round(pos, 2)
    w = float(rng.choice([0.1, 0.25, 1.0]))
    for own in ((0, n), (n // 4, n // 2), (n // 3 + 5, 2 * n // 3 - 7), (n - 1, n), (0, 1)):
        A, R, pairs = gpu_schedule_restated(pos, w, own)
        s = schedule_restated(pos, w, own)
        np.testing.assert_array_equal(s["A"], A)
        np.testing.assert_array_equal(s["R"], R)
        assert block_pairs(s) == pairs and s["items"] == len(pairs)
        for pair in (0, 1):
            items = _emit_loops(s["d0"], s["d1"], s["nblk"], pair)
            assert covered(items) == pairs and len(set(items)) == len(items)
            assert len(items) == (s["pair_items"] if pair else s["items"])
        # the add+dom split plan, block pair by block pair: a row's needed offsets of one tile column, in order, are
        # taken two at a time; the pairs and the singles together cover every block pair once
        n_pair = n_single = 0
        odd = np.zeros(s["nblk"], np.int64)
        split = []
        for I in range(s["nblk"]):
            for c in range(_ceil(s["nblk"], 16) + 1):
                piece = [J - I for (i, J) in sorted(pairs) if i == I and (J - I) // 16 == c]
                for k in range(0, len(piece) - 1, 2):
                    assert piece[k + 1] == piece[k] + 1
                    split.append((I, I + piece[k], 2, 0))
                if len(piece) % 2:
                    split.append((I, I + piece[-1], 1, 0))
                n_pair, n_single, odd[I] = n_pair + len(piece) // 2, n_single + len(piece) % 2, odd[I] + len(piece) % 2
        assert covered(split) == pairs and sum(z for _, _, z, _ in split) == len(pairs)
        assert (s["split_pairs"], s["split_singles"]) == (n_pair, n_single)
        np.testing.assert_array_equal(s["odd_pieces"], odd)
        assert s["split_pairs"] == s["items"] - s["pair_items"]
        assert s["split_singles"] == 2 * s["pair_items"] - s["items"]
        # ... and what the routing compaction keeps of both lists, for missing calls in a third of the blocks
        blk_miss = rng.random(s["nblk"]) < 1.0 / 3.0
        for shift in (1, 2):
            def routed(I, J):
                F = 1 << shift
                return not any(blk_miss[min(F * (b // F) + k, s["nblk"] - 1)] for b in (I, J) for k in range(F))
            kept_p = sum(not (routed(I, J) and routed(I, J + 1)) for I, J, z, _ in split if z == 2)
            kept_s = sum(not routed(I, J) for I, J, z, _ in split if z == 1)
            assert split_kept(s, blk_miss, shift) == (kept_p, kept_s)
        for shift, key in ((1, "t2"), (2, "quad")):
            F, cnt = 1 << shift, 0
            for I2 in range(_ceil(s["nblk"], F)):
                cols = [J for b in range(F * I2, min(s["nblk"], F * I2 + F)) for (I, J) in pairs if I == b]
                rng2 = ((min(cols) >> shift) - I2, (max(cols) >> shift) - I2) if cols else (1, 0)
                assert (s[key + "_rows"][0][I2], s[key + "_rows"][1][I2]) == rng2
                cnt += max(0, rng2[1] - rng2[0] + 1)
            assert s[key + "_items"] == cnt


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_geometries_reach_the_scans_they_are_here_for(name):
    """From the restatement alone: the scan sizes, item and super-item counts each geometry is in the table for; the
    restated count is at least the host plan's; SNPs fail MAF; the three missing settings gate the kernels as meant."""
    from nldsc_amd import _lib
    g, s = geometry(name), restated(name)
    M, nblk = g["M"], _ceil(g["M"], 32)
    assert (g["pos"] == np.round(g["pos"])).all() and (np.diff(g["pos"]) == 0).any()
    sz = scan_sizes(s, fused=M <= PLAN_SMALL_N)
    if name == "fused_full":
        assert (nblk, s["tile_counts"], s["items"]) == (1024, 4096, 1024 * 1025 // 2)  # == plan_small_items(M)
        assert sz["right_pointer"] == (32768, 32) and sz["tile_counts"] == (4096, 4)
    if name == "chain_first":
        assert nblk == 1025 and M - 32 * (nblk - 1) == 1 and s["items"] == 1025 * 1026 // 2
        assert sz["tile_counts"][1] > 1 and sz["compact_chunks"][1] > 1
    if name == "narrow_65k":
        assert sz["right_pointer"] == (257, 2)
        assert 8 <= s["items"] / nblk <= 12  # (C3-like: ~10 column blocks per row block)
    if name in ("wide_100k", "ragged_100k"):
        assert sz["right_pointer"][0] > 256 and sz["tile_counts"][0] > 256 and sz["quad_counts"][0] > 256
        assert s["items"] > 65536 and s["pair_items"] > 65536 and s["quad_items"] >= 4096
        for own in own_ranges(M):
            so = restated(name, own)
            assert 0 < so["items"] < s["items"]
    if name == "wide_100k":
        assert _ceil(int((s["d1"] + 1).max()), 16) in (7, 8)
    if name == "ragged_100k":
        d = dataset(name, "rate")
        a, b = g["tie_run"]
        assert b - a >= 200 and a // 256 != (b - 1) // 256 and (g["pos"][a:b] == g["pos"][a]).all()
        assert all(g["pos"][y] - g["pos"][x] == g["w"] for x, y in g["ties"])
        assert (d.wsa == 0).any() and d.wsa[g["lone"]] in (0, -1)
        n_row = s["d1"] - s["d0"] + 1
        assert (n_row == 1).any() and n_row.max() > 50 * max(1, n_row[n_row > 0].min())
        gap = np.diff(g["pos"])
        assert np.median(gap[gap > 0]) * 100 < np.quantile(gap, 0.99) and (gap > g["w"]).sum() >= 4
    assert s["items"] / 2 <= s["pair_items"] < s["items"]
    # the add+dom split plan (test_add_dom_column_pair_rounds and the cases after it), at the MI355X's 256 CUs: at
    # least two rounds of 4 pairs per CU, and a last partial round whose pairs expand_pairs_kernel turns back into
    # single-block items
    rnd = 4 * 256
    assert s["split_pairs"] == s["items"] - s["pair_items"] and s["split_singles"] == 2 * s["pair_items"] - s["items"]
    assert s["split_pairs"] >= 2 * rnd and s["split_singles"] > 0
    if name == "fused_full":
        # every block pair of 1 024 blocks: sum floor(n / 2) = 2^18 pairs, exactly 256 rounds — the edge without a
        # partial round (nothing to expand); chain_first, one block more, has the same band with one
        assert s["split_pairs"] == 256 * rnd
    else:
        assert s["split_pairs"] % rnd != 0
    if name in ("wide_100k", "fused_full"):
        assert s["split_pairs"] > 65536  # (launch_compact_items over more than 256 chunks of pairs under routing)
    if name == "wide_100k":
        assert _ceil(int((s["d1"] + 1).max()), 16) > 1  # more than one tile column
    # a whole run's rows start at offset 0, so every tile-column edge falls on an even offset and only a row's last
    # piece can be odd; an owned range's left halo rows start at J0 - I > 0: there a run is cut into two odd pieces,
    # two singles, where pairing from the row's first block (the host planner's) leaves none
    assert s["odd_pieces"].max() == 1
    if name in OWNED:
        so = restated(name, own_ranges(M)[0])
        two = (so["odd_pieces"] == 2) & ((so["d1"] - so["d0"] + 1) % 2 == 0)
        assert two.any() and so["split_pairs"] >= 2 * rnd and so["split_pairs"] % rnd != 0
        assert so["split_singles"] > int(((so["d1"] - so["d0"] + 1)[so["d0"] <= so["d1"]] % 2).sum())
    if name == "narrow_65k":
        assert s["items"] <= 1 << 16  # the deferred-epilogue slots hold a default-flags run's block pairs
    if name == "wide_100k":
        assert s["items"] > 1 << 16   # ... and here they do not: the KC launch after the replay
    _, _, host = _lib.plan_band(g["pos"], np.ones(M, np.uint8), g["w"], max_nc=1)
    assert len(host) <= s["items"]
    n_fail = {}
    for missing in ("rate", "none", "mixed4"):
        d = dataset(name, missing)
        n_fail[missing] = int((~d.passed).sum())
        assert n_fail[missing] >= 0.03 * M and (d.wsd < d.wsa).any()
        assert {"rate": d.free == 0, "none": d.free == nblk, "mixed4": 0 < d.free < nblk}[missing]
        bm = blocks_with_missing(d.rows, N_ORG)
        assert len(bm) == nblk and int((~bm).sum()) == d.free
        kept = split_kept(s, bm)
        if missing == "rate":
            assert kept == (s["split_pairs"], s["split_singles"])
        if missing == "none":
            assert kept == (0, 0)
        if missing == "mixed4":  # routed runs still fill pair rounds, and not in whole rounds
            assert rnd <= kept[0] < s["split_pairs"] and kept[0] % rnd != 0 and 0 < kept[1] <= s["split_singles"]


def test_target_truth_guards_its_threshold():
    """The targets' truth on a cheap geometry: at least 64 targets, most computed, and rsq_thr clear of every exact r2d
    (Data.truth asserts the gap; every GPU case goes through it)."""
    d = dataset("narrow_65k", "rate")
    rsq, exp = d.truth()
    assert len(d.targets) >= 64 and (exp["l2_ws"] >= 0).sum() >= 48 and 0.01 <= rsq < 0.0101
    np.testing.assert_array_equal(exp["l2_ws"], d.wsa[d.targets])
    np.testing.assert_array_equal(exp["l2d_ws"], d.wsd[d.targets])
    assert (exp["l2d_wse"][exp["l2_ws"] >= 0] < exp["l2d_ws"][exp["l2_ws"] >= 0]).any()


# ---------------------------------------------------------------------------------------------------------------
# GPU runs
# ---------------------------------------------------------------------------------------------------------------

def gpu_run(d, options, want, *, mode="f4", dom=True, own=None, round_items=0):
    """One run on a fresh engine with these options; the kernel it took is the one the data and options dictate
    (`want`: the super-item kernels only with routing candidates, test_gpu_parity's missing_free_blocks rule), in
    launches of `round_items` block pairs (0: one launch)."""
    from nldsc_amd.engine import Engine
    rsq, _ = d.truth()
    flags = MODES[mode] | _lib_flag("FLAG_EXACT_RARE") | (0 if dom else _lib_flag("FLAG_ADDITIVE_ONLY"))
    with Engine(0, options=options) as e:
        e.load_bed_bytes(d.bed, d.M, N_ORG)
        got = e.run(d.w, MAF, STD_THR, rsq, d.pos, flags=flags, own=own)
        t = e.timings()
    assert t["band_kernel"] == want, (d.name, d.missing, options, t["band_kernel"], want, d.free)
    assert t["ksplit"] == 1 and t["band_round_items"] == round_items, (t["ksplit"], t["band_round_items"], round_items)
    check_run(d, got, own=own, dom=dom, label=f"{d.name} {d.missing} {options} {mode} own {own}")
    return got, t


def check_run(d, got, *, own, dom, label):
    lo, hi = (0, d.M) if own is None else own
    o = slice(lo, hi)
    # 1. the window counts of every owned SNP: a dropped or doubled block pair changes them
    for k, exp in (("l2_ws", d.wsa), ("l2d_ws", d.wsd if dom else np.full(d.M, -1, np.int32))):
        bad = lo + np.flatnonzero(got[k][o] != exp[o])
        print(f"{label}: {k} differs at {bad.size} SNPs")
        assert bad.size == 0, (f"{label}: {k} differs at {bad.size} SNPs, first {bad[:8]} (blocks {bad[:8] // 32}): "
                               f"got {got[k][bad[:8]]}, closed form {exp[bad[:8]]}")
    # 2. MAF and the NaN patterns against the oracle's per-SNP statistics
    np.testing.assert_array_equal(got["maf"][o], d.maf[o], err_msg=f"{label} maf")
    np.testing.assert_array_equal(np.isnan(got["l2"][o]), ~d.passed[o], err_msg=f"{label} l2 NaN")
    np.testing.assert_array_equal(np.isnan(got["l2d"][o]), ~d.passed[o] | (not dom), err_msg=f"{label} l2d NaN")
    np.testing.assert_array_equal(np.isnan(got["residuals_std"][o]), ~d.passed[o], err_msg=f"{label} rstd NaN")
    # 3. the targets against oracle.run_f64_targets: scores at the exact-path bar, WSDE equal
    _, exp = d.truth()
    m = (d.targets >= lo) & (d.targets < hi)
    sub = {k: v[d.targets[m]] for k, v in got.items()}
    ref = {k: v[m] for k, v in exp.items()}
    if not dom:
        n = int(m.sum())
        ref = dict(ref, l2d=np.full(n, np.nan), l2d_ws=np.full(n, -1, np.int32), l2d_wse=np.full(n, -1, np.int32))
    assert m.any()
    assert_ld_close(sub, ref, tol=EXACT, label=label)
    np.testing.assert_array_equal(sub["l2d_wse"], ref["l2d_wse"], err_msg=f"{label} l2d_wse")


def owned(r, own):
    return r if own is None else {k: v[own[0]:own[1]] for k, v in r.items()}


def bitwise(a, b, label):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label} {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_missing_calls_in_every_block(data, name):
    """Single-block kernel from the whole item list: the default plan (fused up to 32 768 SNPs, else the chain), the
    chain (plan_fused 0) and the host plan (gpu_plan 0) as the full-array second opinion."""
    from nldsc_amd import _lib
    d, s = data(name, "rate"), restated(name)
    assert d.free == 0
    got, t = gpu_run(d, {}, "f4")
    chain, tc = gpu_run(d, {"plan_fused": 0}, "f4")
    host, th = gpu_run(d, {"gpu_plan": 0}, "f4")
    assert t["band_items"] == tc["band_items"] == s["items"], (t["band_items"], tc["band_items"], s["items"])
    _, _, items = _lib.plan_band(d.pos, np.ones(d.M, np.uint8), d.w, max_nc=1)
    assert th["band_items"] == len(items) <= s["items"]
    same_gram(got, host, f"{name} default vs host plan")
    same_gram(chain, host, f"{name} chain vs host plan")
    same_gram(got, chain, f"{name} default vs chain")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_missing_free_super_items(data, name):
    """Missing-free data: the quad kernel from the 4 x 4 super-item plan, in CU-wide rounds (q_rounds, from 4 096
    super-items) and in one launch, the 2 x 2 kernel from its plan (t2 2), and routing with every item routed (t2 1)."""
    d, s = data(name, "none"), restated(name)
    assert d.free == s["nblk"]
    q1, t1 = gpu_run(d, {}, "f4_quad")
    q0, t0 = gpu_run(d, {"q_rounds": 0}, "f4_quad")
    bitwise(q1, q0, f"{name} q_rounds 1 vs 0")
    x2, t2 = gpu_run(d, {"t2": 2}, "f4_2x2")
    x1, tr = gpu_run(d, {"t2": 1}, "f4_routed")
    for t in (t1, t0, t2, tr):
        assert t["band_items"] == s["items"]
    same_gram(q1, x2, f"{name} quad vs 2x2")
    same_gram(q1, x1, f"{name} quad vs routed")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_mixed_groups_quad_beside_compacted_single_items(data, name):
    """Missing calls in every third group of four blocks: quad super-items beside the single-block items the
    compaction keeps (compact_count / scan_counts / compact_scatter over the whole item list)."""
    d, s = data(name, "mixed4"), restated(name)
    got, t = gpu_run(d, {}, "f4_quad")
    assert t["band_items"] == s["items"]
    ref, _ = gpu_run(d, {"gpu_plan": 0}, "f4")
    same_gram(got, ref, f"{name} mixed4 quad vs host plan")


@pytest.mark.gpu
@pytest.mark.parametrize("missing", ["rate", "mixed4"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_additive_only_column_block_pairs(data, name, missing):
    """Additive-only: the pair plan's (I, J, 2) items with their (I, J, 1) leftovers at tile edges (f4_nc2 1) against
    single-block items (f4_nc2 0): the same issued products, bitwise the same arrays."""
    d, s = data(name, missing), restated(name)
    want = "f4" if d.free == 0 else "f4_quad"
    a, ta = gpu_run(d, {"f4_nc2": 1}, want, dom=False)
    b, tb = gpu_run(d, {"f4_nc2": 0}, want, dom=False)
    assert (ta["band_items"], tb["band_items"]) == (s["pair_items"], s["items"])
    assert ta["flop_issued"] == tb["flop_issued"] > 0, (ta["flop_issued"], tb["flop_issued"])
    bitwise(a, b, f"{name} {missing} f4_nc2 1 vs 0")


@pytest.mark.gpu
def test_int8_band_on_the_wide_geometry(data):
    d, s = data("wide_100k", "rate"), restated("wide_100k")
    i8, t = gpu_run(d, {}, "i8", mode="i8")
    f4, _ = gpu_run(d, {}, "f4")
    assert t["band_items"] == s["items"]
    same_gram(i8, f4, "wide_100k i8 vs f4")


@pytest.mark.gpu
@pytest.mark.parametrize("missing", ["rate", "mixed4"])
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("name", OWNED)
def test_owned_ranges(data, name, k, missing):
    """Owned ranges whose ends lie inside blocks, the last SNP alone and the first alone: every owned SNP's counts,
    the item count of the restated schedule for that range, the host plan's run as the second opinion."""
    d = data(name, missing)
    own = own_ranges(d.M)[k]
    s = restated(name, own)
    got, t = gpu_run(d, {}, "f4" if d.free == 0 else "f4_quad", own=own)
    assert t["band_items"] == s["items"] > 0, (t["band_items"], s["items"])
    host, th = gpu_run(d, {"gpu_plan": 0}, "f4", own=own)
    assert 0 < th["band_items"] <= s["items"]
    same_gram(owned(got, own), owned(host, own), f"{name} {missing} own {own} vs host plan")


# ---------------------------------------------------------------------------------------------------------------
# the add+dom column-pair plan (plan_*_split, expand_pairs_kernel, the second compaction under routing,
# launch_colpair) in rounds of the production size, 4 pairs per CU
# ---------------------------------------------------------------------------------------------------------------

def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def expected_pair_rounds(d, s, rnd):
    """(band kernel, band_round_items, (pairs launched, pairs emitted, single-block items of the rest)) of an add+dom
    run of data set d on the restated schedule s with rounds of rnd pairs.  The rule: the split plan's pairs — under
    super-item routing (missing-free blocks: d.free > 0) those the compaction keeps, split_kept — run in pair rounds
    when they fill one round (the round option's minimum) and the band holds two rounds of block pairs; whole rounds
    only, every pair past them back as two single-block items behind the (kept) leftover singles.  Otherwise no pair
    item runs and the run reports the kernel it took before."""
    plain = "f4" if d.free == 0 else "f4_quad"
    pairs, singles = (s["split_pairs"], s["split_singles"]) if d.free == 0 else \
        split_kept(s, blocks_with_missing(d.rows, N_ORG))
    if pairs < rnd or s["items"] < 2 * rnd:
        return plain, 0, (0, 0, 0)
    return "f4_colpair", 2 * rnd, (pairs // rnd * rnd, pairs, singles + 2 * (pairs % rnd))


def pair_rounds_ab(d, s, options, *, own=None):
    """The add+dom run in pair rounds of 4 per CU against the same run with f4_nc2_dom 0: the kernel, the round and
    the three list sizes the restatement gives, everything check_run checks on both, bitwise equal arrays, equal
    flop_issued and band_items."""
    rnd = 4 * cu_count()
    want, round_items, lists = expected_pair_rounds(d, s, rnd)
    opts = dict(options, colpair_round_items=rnd)
    a, ta = gpu_run(d, dict(opts, f4_nc2_dom=1), want, own=own, round_items=round_items)
    b, tb = gpu_run(d, dict(opts, f4_nc2_dom=0), "f4" if d.free == 0 else "f4_quad", own=own)
    got = (ta["band_pair_items"], ta["band_pairs"], ta["band_pair_rest"])
    assert got == lists, (d.name, d.missing, options, own, got, lists)
    assert (tb["band_pair_items"], tb["band_pairs"], tb["band_pair_rest"]) == (0, 0, 0), tb
    assert ta["band_items"] == tb["band_items"] == s["items"], (ta["band_items"], tb["band_items"], s["items"])
    assert ta["flop_issued"] == tb["flop_issued"] > 0, (ta["flop_issued"], tb["flop_issued"])
    bitwise(a, b, f"{d.name} {d.missing} {options} own {own}: f4_nc2_dom 1 vs 0")
    return want, lists


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0], ids=["default_plan", "chain"])
@pytest.mark.parametrize("missing", ["rate", "mixed4"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_add_dom_column_pair_rounds(data, name, missing, fused):
    """Add+dom in pair rounds of the production size at production SNP counts: the split plan over many tile columns
    and multi-chunk scans of both count arrays (behind the fused plan up to 32 768 SNPs, behind the chain with
    plan_fused 0), the last pairs through expand_pairs_kernel, and with missing-free groups of blocks ("mixed4") the
    second compaction of both lists beside the quad kernel."""
    d, s = data(name, missing), restated(name)
    want, lists = pair_rounds_ab(d, s, {} if fused else {"plan_fused": 0})
    if cu_count() == 256:  # (test_geometries_reach_the_scans_they_are_here_for asserts these sizes for 256 CUs)
        assert want == "f4_colpair" and lists[0] >= 1024, (want, lists)
        assert (lists[1] % 1024 == 0) == ((name, missing) == ("fused_full", "rate")), lists


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("name", OWNED)
def test_add_dom_column_pair_rounds_on_owned_ranges(data, name, k):
    """Owned ranges: the left halo's rows start at offset J0 - I > 0, so their runs are cut at tile-column edges into
    pieces the host planner's pairing does not have (two singles where it has none); the one-SNP ranges hold fewer
    pairs than a round and run no pair item."""
    d = data(name, "rate")
    own = own_ranges(d.M)[k]
    s = restated(name, own)
    want, lists = pair_rounds_ab(d, s, {}, own=own)
    if cu_count() == 256:
        assert (want == "f4_colpair") == (k == 0), (want, lists)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["narrow_65k", "wide_100k"])
def test_add_dom_column_pair_rounds_with_replayed_snps(data, name):
    """Default flags: the rare variants (at N = 67 nearly every SNP) are replayed, so the pair items run their K loops
    in the pair launch with the Gram tiles kept for the deferred epilogue (narrow_65k: its block pairs fit the 2^16
    slots) or wait for the KC instantiation after the replay (wide_100k: they do not).  Bitwise f4_nc2_dom 0 only:
    the replay arithmetic is held to the oracle in test_gpu_parity.py and test_gpu_colpair_dom.py."""
    from nldsc_amd.engine import Engine
    d, s = data(name, "rate"), restated(name)
    rnd = 4 * cu_count()
    want, round_items, lists = expected_pair_rounds(d, s, rnd)
    out = {}
    with Engine(0, options={"colpair_round_items": rnd}) as e:
        e.load_bed_bytes(d.bed, d.M, N_ORG)
        for on in (1, 0):
            e.set_option("f4_nc2_dom", on)
            out[on] = (e.run(d.w, MAF, STD_THR, 0.01, d.pos, flags=MODES["f4"]), e.timings())
    (a, ta), (b, tb) = out[1], out[0]
    assert (ta["band_kernel"], ta["band_round_items"], tb["band_kernel"], tb["band_round_items"]) == \
        (want, round_items, "f4", 0), (ta, tb)
    assert (ta["band_pair_items"], ta["band_pairs"], ta["band_pair_rest"]) == lists, (ta, lists)
    assert ta["band_items"] == tb["band_items"] == s["items"] and ta["flop_issued"] == tb["flop_issued"] > 0
    assert (s["items"] <= 1 << 16) == (name == "narrow_65k")
    bitwise(a, b, f"{name} default flags: f4_nc2_dom 1 vs 0")
    assert np.isfinite(a["l2"]).sum() > 0.5 * d.M
