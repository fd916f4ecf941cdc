"""The exact fp4 Gram where its accumulators fill up, on rows whose head misleads the allele flip.

The fp4 band's first plane holds v = m + 2x in {0, 1, 2, 4} for the codes (00, 01, 10, 11), so a product is at most
16 and an fp32 accumulator holds an exact integer up to N = 2^19 (entry <= 2^23); longer rows run in segments that are
folded into int32 accumulators (add+dom) or into packed 16-bit counters plus an fp32 remainder (additive-only), and
small launches sum K-split partial fp32 tiles (ld_kernels.hip band_f4_body, band_f4_epi_kernel).  Stationary random
rows, oriented minor-homozygote-as-00 at load, leave every entry at about a tenth of those bounds.  The rows here are
code-11 dominant in the RESIDENT image: load_orient_kernel decides a row's flip from its first LOAD_ORIENT_BYTES =
1024 bytes (4 096 samples) only, and the head of these rows says the opposite of their body.  So one data set drives
the Gram entries to their bounds and loads rows whose stored orientation is the "wrong" one.

The generator's properties are asserted on the truth, not on the engine (the tests outside TestGpu, no GPU needed):
the largest post-orientation entry vv(j, k) = sum_gh v_g v_h C_jk[g][h] from the oracle's integer contingency tables,
that one unit of error in such an entry moves the pair's r2adj by >= 1e-7 (100 x the 1e-9 bar the results are held
to), and that no exact r2d lies within 1e-6 of rsq_thr (so WSDE is compared exactly, without a tie budget).

Two things differ from a literal reading of the kernel comments, both read from the code: (1) n_it, the row length in
128-sample chunks, is always even (rows are padded to 64 bytes), so N = 2^19 + 128 and 2^19 + 132 both run 4 098
chunks: a final segment of 2 chunks, of which the second is all padding (N = 2^19 + 128) or holds 4 samples;
(2) launches of one round of wave slots (option band_rounds) need 8 items per CU, far more than the 6 items of 70
SNPs: test_round_launches_on_saturated_rows repeats the 70 rows to 2 048 SNPs for that path (its truth by multiplicity,
multiplicity_truth, is test_gpu_colpair_long.py's too).  The add+dom column-pair tile (16 accumulator tiles, one wave
per SIMD) takes the same 70 rows through the round option colpair_round_items: PATHS colpair*.

Out of scope: N near 2^27, the int32 limit of an entry (16 N < 2^31) — a data set there is gigabytes and its truth
takes minutes.
"""
import os

import numpy as np
import pytest

from conftest import record
from oracle import oracle as O

HEAD = 4096          # samples in the bytes load_orient_kernel reads (LOAD_ORIENT_BYTES = 1024)
V = np.array([0.0, 1.0, 2.0, 4.0])  # first-plane value of the codes 00, 01 (missing), 10 (het), 11
PERTURBED = 0.08     # fraction of a saturated row's body that differs from its dominant genotype
# share of those positions that all rows of a data set have in common (the rest are the row's own): measured at
# N = 2^19, |r| between saturated rows is 0.38 .. 0.48 and the largest entry 0.907 x 2^23
SHARED = 0.5
STD_THR, LD_WIND = 1e-5, 1.0
F_STRICT, F_ADD, F_I8, F_F4, F_RARE = 1, 2, 4, 16, 32  # nldsc_amd._lib.FLAG_*
EXACT = dict(l2=(1e-9, 1e-12), l2d=(1e-9, 1e-12))  # test_random_small_configs_vs_f64's exact-path bar
# the oracle's OpenMP team size is process-wide and tests before these leave it at 1 (threads=1): the counting
# helpers here get the CPUs this process may use
THREADS = min(16, len(os.sched_getaffinity(0)))

# name: (N, M, missing calls, lower bound on the largest in-window entry, rsq_thr)
CASES = {
    "n2p19": (1 << 19, 70, True, 0.9 * 2 ** 23, 0.02),
    "n2p19_free": (1 << 19, 70, False, 0.9 * 2 ** 23, 0.02),  # no missing call at all: the t2 / quad routing
    "seg_p128": ((1 << 19) + 128, 40, True, 0.9 * 2 ** 23, 0.02),
    "seg_p132": ((1 << 19) + 132, 40, True, 0.9 * 2 ** 23, 0.02),
    "n1500001": (1_500_001, 70, True, 2.0 ** 24, 0.02),
    "n2p22_3": ((1 << 22) + 3, 40, True, 2.0 ** 24, 0.02),
}
SEGMENTED = [c for c in CASES if CASES[c][0] > 1 << 19]


def saturating_genotypes(N, M, missing, seed):
    """int8 genotypes [M][N]; row kinds A, B, C, D in turn (j % 4), so every 32-SNP block mixes them:
    A head (samples 0..4095) hom-A1, body hom-A2: not flipped, the image is 11-dominant;
    B head hom-A2, body hom-A1: flipped, the image is 11-dominant again;
    C head het, body hom-A2: c2 = c0 = 0 in the head, not flipped whatever a tie does;
    D synth.genotypes rows, the unsaturated control.
    A / B / C bodies differ from their dominant genotype at PERTURBED of the positions — SHARED of them common to all
    rows, the rest the row's own — by a draw per row and position: het, the other homozygote or missing."""
    from nldsc_amd import synth
    rng = np.random.default_rng(seed)
    body = N - HEAD
    shared_pos = HEAD + rng.choice(body, int(round(PERTURBED * SHARED * body)), replace=False)
    n_own = int(round(PERTURBED * (1.0 - SHARED) * body))
    ctrl = synth.genotypes(synth.SynthSpec(n_org=N, n_snp=(M + 1) // 4 + 1, seed=seed,
                                           missing=0.01 if missing else 0.0))
    g = np.empty((M, N), np.int8)
    for j in range(M):
        if j % 4 == 3:
            g[j] = ctrl[j // 4]
            continue
        head, dom = ((0, 2), (2, 0), (1, 2))[j % 4]
        row = np.full(N, dom, np.int8)
        row[:HEAD] = head
        at = np.concatenate([shared_pos, HEAD + rng.integers(0, body, n_own)])
        row[at] = rng.choice(np.array([1, 2 - dom, -1], np.int8), at.size,
                             p=(0.5, 0.3, 0.2) if missing else (0.6, 0.4, 0.0))
        g[j] = row
    return g


def stored_flip(rows):
    """load_orient_kernel's rule in numpy: a row is stored 00 <-> 11 swapped when its first LOAD_ORIENT_BYTES bytes
    hold more 11 than 00 codes."""
    head = rows[:, :1024]
    codes = np.stack([(head >> s) & 3 for s in (0, 2, 4, 6)], axis=-1)
    return (codes == 3).sum(axis=(1, 2)) > (codes == 0).sum(axis=(1, 2))


_data: dict = {}
_truth: dict = {}


def dataset(case):
    """(rows, bed image, positions, N, M, rsq_thr) of a case, generated once.  The window covers all pairs."""
    if case not in _data:
        from nldsc_amd import synth
        N, M, missing, _, rsq = CASES[case]
        rows = synth.pack_bed_rows(saturating_genotypes(N, M, missing, seed=sorted(CASES).index(case)))
        _data[case] = (rows, synth.bed_bytes(rows), np.arange(M, dtype=np.float64) * 0.01, N, M, rsq)
    return _data[case]


def truth(case, strict=False):
    """O.run_f64_targets at every SNP: the integer-contingency truth in binary64 (maf 0, std_thr 1e-5)."""
    if (case, strict) not in _truth:
        rows, bed, pos, N, M, rsq = dataset(case)
        O.code_counts(bed, M, N, threads=THREADS)  # (sets the team size of the table counts below)
        _truth[case, strict] = O.run_f64_targets(rows, N, LD_WIND, 0.0, STD_THR, rsq, pos, np.arange(M), strict=strict,
                                                 bed=bed)
    return _truth[case, strict]


def pair_truth(case):
    """Per unordered pair j < k, from O.code_tables and O.stats_from_counts alone: the resident image's entry vv, the
    exact additive correlation r, |d r2adj| of one unit of vv, and every ordered pair's exact dominance r2adj (r2d_of:
    the SNP whose score it enters)."""
    rows, bed, pos, N, M, rsq = dataset(case)
    cnt = O.code_counts(bed, M, N, threads=THREADS)
    st = O.stats_from_counts(cnt, N)
    la, lr, rpass = st["lut_a"], st["lut_r"], st["rstd"] > STD_THR
    flip = stored_flip(rows)
    v = np.where(flip[:, None], V[[3, 1, 2, 0]][None, :], V[None, :])  # [M][file code]: the stored row's plane value
    sd = 2.0 / np.abs(la[:, 3] - la[:, 0])  # additive sd in genotype units: lut_a = (a - mean) / sd, a = 0, 1, 2
    adj = (N - 1.0) / (N - 2.0)
    jj, kk, vv, r, moved, r2d, r2d_of = [], [], [], [], [], [], []
    for j in range(M - 1):
        ks = np.arange(j + 1, M)
        C = O.code_tables(bed, M, N, j, ks).astype(np.float64)
        jj.append(np.full(len(ks), j))
        kk.append(ks)
        vv.append(np.einsum("g,kgh,kh->k", v[j], C, v[ks]))
        rj = np.einsum("g,kgh,kh->k", la[j], C, la[ks]) / N
        r.append(rj)
        # x = (v - m) / 2 on the called samples, so vv enters sum_s a_j a_k with the weight 1 / (4 sd_j sd_k):
        # one unit of vv moves r by d and r2adj = 1 - (1 - r^2) (N - 1) / (N - 2) by at least (2 |r| d - d^2) adj
        d = 1.0 / (4.0 * sd[j] * sd[ks] * N)
        moved.append((2.0 * np.abs(rj) * d - d * d) * adj)
        jk = np.einsum("g,kgh,kh->k", la[j], C, lr[ks]) / N   # pair (j, k): j's additive, k's residual vector
        kj = np.einsum("g,kgh,kh->k", lr[j], C, la[ks]) / N   # pair (k, j)
        r2d.append((1.0 - (1.0 - jk ** 2) * adj)[rpass[ks]])
        r2d_of.append(np.full(int(rpass[ks].sum()), j))
        if rpass[j]:
            r2d.append(1.0 - (1.0 - kj ** 2) * adj)
            r2d_of.append(ks)
    cat = np.concatenate
    return dict(j=cat(jj), k=cat(kk), vv=cat(vv), r=cat(r), moved=cat(moved), r2d=cat(r2d), r2d_of=cat(r2d_of),
                counts=cnt, flip=flip)


@pytest.mark.parametrize("case", sorted(CASES))
def test_generator_saturates_and_the_bar_bites(case):
    """The two generator conditions and the rsq_thr gap, from the oracle alone."""
    rows, bed, pos, N, M, rsq = dataset(case)
    _, _, missing, vv_min, _ = CASES[case]
    p = pair_truth(case)
    cnt, flip, kind = p["counts"], p["flip"], np.arange(M) % 4
    # the flip rule sees the head: A and C rows keep the file coding, B rows are swapped — every A / B / C row is
    # stored with 11 as its dominant code — and the control rows are stored 00-dominant
    assert not flip[kind == 0].any() and flip[kind == 1].all() and not flip[kind == 2].any()
    stored11 = np.where(flip, cnt[:, 0], cnt[:, 3])
    assert (stored11[kind != 3] > 0.9 * (1.0 - PERTURBED) * N).all()
    assert (stored11[kind == 3] < 0.35 * N).all()
    # no row is a replayed rare variant; the missing-free variant has no missing call
    assert cnt[:, [0, 2, 3]].min() > 16
    assert (cnt[:, 1] > 16).all() if missing else (cnt[:, 1] == 0).all()
    print(f"{case}: largest entry {p['vv'].max():.0f} = {p['vv'].max() / 2 ** 23:.4f} x 2^23 (16 N = {16 * N})")
    assert p["vv"].max() >= vv_min and p["vv"].max() <= 16.0 * N
    if vv_min >= 2.0 ** 24:
        assert p["vv"].max() > 2.0 ** 24  # unfolded fp32 would round
    sat = (p["j"] % 4 != 3) & (p["k"] % 4 != 3)
    big = np.abs(p["r"][sat]) >= 0.3
    bites = p["moved"][sat] >= 1e-7
    print(f"{case}: {sat.sum()} saturated pairs, |r| >= 0.3 on {big.mean():.3f}, one unit of vv moves r2adj by >= "
          f"1e-7 on {bites.mean():.3f} (median {np.median(p['moved'][sat]):.3g})")
    assert big.mean() >= 0.5 and bites.mean() >= 0.5
    # saturated x saturated, saturated x ordinary and ordinary x ordinary pairs, in diagonal and off-diagonal tiles
    # (a last block of fewer than 8 SNPs holds one control row: no ordinary pair on its diagonal)
    nblk = (M + 31) // 32
    blocks = {(a, b) for a in range(nblk) for b in range(a, nblk)}
    short = {(nblk - 1, nblk - 1)} if 0 < M % 32 < 8 else set()
    for sel, want in ((sat, blocks), ((p["j"] % 4 != 3) ^ (p["k"] % 4 != 3), blocks),
                      ((p["j"] % 4 == 3) & (p["k"] % 4 == 3), blocks - short)):
        assert {(int(a), int(b)) for a, b in zip(p["j"][sel] // 32, p["k"][sel] // 32)} == want
    gap = np.abs(p["r2d"] - rsq).min()
    above = int((p["r2d"] > rsq).sum())
    print(f"{case}: closest exact r2d to rsq_thr = {rsq}: {gap:.3g}; {above} of {p['r2d'].size} above it")
    assert gap > 1e-6 and 0 < above < p["r2d"].size
    # ... and the pairwise restatement above is the truth's, at a SNP of each block
    t = np.array(sorted({0, 33 % M, M - 1}))
    exp = O.run_f64_targets(rows, N, LD_WIND, 0.0, STD_THR, rsq, pos, t, bed=bed)
    for q, j in enumerate(t):
        mine = p["r2d"][p["r2d_of"] == j]
        assert exp["l2d_ws"][q] == mine.size and exp["l2d_wse"][q] == (mine > rsq).sum()
        assert abs(exp["l2d"][q] - mine.sum()) < 1e-12


def check_exact(got, exp, label, dom=True):
    """The issue's assertions: L2 / L2D within the exact-path bar, MAF and the window counts exact, residual std at
    rtol 1e-12, equal NaN patterns.  Returns the worst errors (L2 / L2D in units of the bound)."""
    rec = {}
    if not dom:
        assert np.isnan(got["l2d"]).all() and (got["l2d_ws"] == -1).all() and (got["l2d_wse"] == -1).all(), label
    for k in ("l2", "l2d") if dom else ("l2",):
        assert np.array_equal(np.isnan(got[k]), np.isnan(exp[k])), f"{label} {k}: NaN pattern"
        m = ~np.isnan(exp[k])
        err = np.abs(got[k][m] - exp[k][m])
        lim = EXACT[k][0] + EXACT[k][1] * np.abs(exp[k][m])
        rec[k] = dict(max_abs=float(err.max(initial=0)), worst_bound_units=float((err / lim).max(initial=0)))
    for k in ("l2_ws", "l2d_ws", "l2d_wse") if dom else ("l2_ws",):
        rec[k] = dict(mismatches=int((got[k] != exp[k]).sum()))
    m = ~np.isnan(exp["residuals_std"])
    rel = np.abs(got["residuals_std"][m] - exp["residuals_std"][m]) / np.abs(exp["residuals_std"][m])
    rec["residuals_std"] = dict(max_rel=float(rel.max(initial=0)))
    print(f"{label}: {rec}")
    assert np.isfinite(exp["l2"]).all() and (exp["l2_ws"] == len(exp["l2"]) - 1).all(), label
    np.testing.assert_array_equal(got["maf"], exp["maf"], err_msg=f"{label} maf")
    for k in ("l2_ws", "l2d_ws", "l2d_wse") if dom else ("l2_ws",):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=f"{label} {k}")
    assert np.array_equal(np.isnan(got["residuals_std"]), ~m), f"{label} residuals_std: NaN pattern"
    np.testing.assert_allclose(got["residuals_std"][m], exp["residuals_std"][m], rtol=1e-12, atol=0.0,
                               err_msg=f"{label} residuals_std")
    for k in ("l2", "l2d") if dom else ("l2",):
        assert rec[k]["worst_bound_units"] <= 1.0, f"{label} {k}: {rec[k]}"
    return rec


def bitwise(got, ref, label):
    for k in ref:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=f"{label} {k}")


def exact_pairs(rows, N):
    """(pairs, own) of a few distinct rows: O.pair_r2_f64 of every row against all others (one window), and of every
    row beside a copy of itself — a copy of row j has r = 1 and the dominance pair r2d(j, j)."""
    M = len(rows)
    pairs = O.pair_r2_f64(rows, N, LD_WIND, 0.0, STD_THR, np.arange(M) * 0.01, np.arange(M))
    # (rows beside their copies, every other SNP out of the window)
    own = O.pair_r2_f64(np.repeat(rows, 2, axis=0), N, LD_WIND, 0.0, STD_THR,
                        np.repeat(np.arange(M) * 10.0, 2), 2 * np.arange(M))
    return pairs, own


def exact_r2d(pairs_own):
    """Every exact dominance r2adj that enters a score of the repeated rows."""
    pairs, own = pairs_own
    return np.concatenate([p[3] for p in pairs] + [p[3] for p in own])


def multiplicity_truth(pairs_own, reps, rsq, per_snp):
    """The truth of `reps` SNPs that repeat M distinct rows in turn (SNP j holds row j % M), all in one window, from
    the rows' exact pairs: SNP j's neighbours are mult[k] copies of every other row and mult[j] - 1 of its own.
    per_snp: the M rows' own truth (maf, residuals_std; the arrays' dtypes)."""
    pairs, own = pairs_own
    M = len(pairs)
    mult = np.bincount(np.arange(reps) % M, minlength=M)
    exp = {k: np.empty(reps, v.dtype) for k, v in per_snp.items()}
    for j in range(M):
        ks, r2a, kds, r2d = pairs[j]
        assert len(ks) == M - 1 and len(kds) == M - 1
        ks2, r2a2, kds2, r2d2 = own[j]
        assert list(ks2) == [2 * j + 1] and list(kds2) == [2 * j + 1]
        a_self, d_self = r2a2[0], r2d2[0]
        sel = np.arange(j, reps, M)
        exp["l2"][sel] = 1.0 + (mult[ks] * r2a).sum() + (mult[j] - 1) * a_self
        exp["l2d"][sel] = (mult[kds] * r2d).sum() + (mult[j] - 1) * d_self
        exp["l2d_wse"][sel] = (mult[kds] * (r2d > rsq)).sum() + (mult[j] - 1) * (d_self > rsq)
        assert abs(d_self - rsq) > 1e-6
        for k in ("maf", "residuals_std"):
            exp[k][sel] = per_snp[k][j]
    exp["l2_ws"][:] = exp["l2d_ws"][:] = reps - 1
    return exp


def check_multiplicity(got, exp, label):
    """The exact-path bar per SNP: L2 / L2D within 1e-9 + 1e-12 |x|, MAF and the counts equal, residual std at rtol
    1e-12."""
    for k in ("l2", "l2d"):
        err = np.abs(got[k] - exp[k])
        lim = 1e-9 + 1e-12 * np.abs(exp[k])
        print(f"{label} {k}: worst |d| {err.max():.3g}, {(err / lim).max():.3g} x the bound")
        assert (err <= lim).all(), k
    for k in ("maf", "l2_ws", "l2d_ws", "l2d_wse"):
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
    np.testing.assert_allclose(got["residuals_std"], exp["residuals_std"], rtol=1e-12, atol=0.0)


_runs: dict = {}


def run(case, flags, opts=None, want_kernel=None):
    """(results, timings) of a fresh engine with these options (nldsc_engine_set_option, as test_gpu_parity._opt_run
    selects them) on the case's rows; cached per (case, flags, options)."""
    from nldsc_amd.engine import Engine
    key = (case, flags, tuple(sorted((opts or {}).items())))
    if key not in _runs:
        rows, bed, pos, N, M, rsq = dataset(case)
        with Engine(0, options=opts) as e:
            e.load_bed_bytes(bed, M, N)
            got = e.run(LD_WIND, 0.0, STD_THR, rsq, pos, flags=flags)
            _runs[key] = (got, e.timings())
    got, t = _runs[key]
    if want_kernel is not None:
        assert t["band_kernel"] == want_kernel, (case, opts, t["band_kernel"], want_kernel)
    return got, t


SINGLE = {"ksplit": 0, "t2": 0, "f4_nc2": 0}  # one launch of single-block items: the kernel the others are held to

def pair_lists(t):
    """(pair items launched as pairs, pairs the plan emitted, single-block items of the rest) of a run's timings."""
    return t["band_pair_items"], t["band_pairs"], t["band_pair_rest"]


# the unsegmented paths at N = 2^19: (case, additive-only, options, band kernel, timings that must hold)
PATHS = {
    "ksplit": ("n2p19", False, {"t2": 0}, "f4_ksplit", lambda t: t["ksplit"] > 1),
    "ksplit_additive": ("n2p19", True, {"t2": 0, "f4_nc2": 0}, "f4_ksplit", lambda t: t["ksplit"] > 1),
    "ksplit_missing_free": ("n2p19_free", False, {"t2": 0}, "f4_ksplit", lambda t: t["ksplit"] > 1),
    "nc2": ("n2p19", True, {"ksplit": 0, "t2": 0, "f4_nc2": 1}, "f4", lambda t: t["band_items"] < 6),
    "nc2_missing_free": ("n2p19_free", True, {"ksplit": 0, "t2": 0, "f4_nc2": 1}, "f4", lambda t: t["band_items"] < 6),
    "band_rounds_off": ("n2p19", False, {"ksplit": 0, "t2": 0, "band_rounds": 0}, "f4", lambda t: True),
    "band_rounds_off_ksplit": ("n2p19", False, {"t2": 0, "band_rounds": 0}, "f4_ksplit", lambda t: t["ksplit"] > 1),
    "t2_routed": ("n2p19_free", False, {"ksplit": 0, "t2": 1}, "f4_routed", lambda t: True),
    "t2_2x2": ("n2p19_free", False, {"ksplit": 0, "t2": 2}, "f4_2x2", lambda t: True),
    "t2_quad": ("n2p19_free", False, {"ksplit": 0, "t2": 3}, "f4_quad", lambda t: True),
    "t2_quad_additive": ("n2p19_free", True, {"ksplit": 0, "t2": 3}, "f4_quad", lambda t: True),
    # add+dom column-pair rounds (the one-wave 32 x 64 tile, 16 accumulator tiles, 4 096 chunks): the 3 blocks' 6 block
    # pairs are the pair items (0, 0)+(0, 1) and (1, 1)+(1, 2) — both diagonal, the second with the 6-SNP last block —
    # and the leftover singles (0, 2) and (2, 2); in one round of 2 pairs and in two of 1
    "colpair": ("n2p19", False, {"t2": 0, "colpair_round_items": 2}, "f4_colpair",
                lambda t: t["band_round_items"] == 4 and pair_lists(t) == (2, 2, 2) and t["ksplit"] == 1),
    "colpair_one_per_round": ("n2p19", False, {"t2": 0, "colpair_round_items": 1}, "f4_colpair",
                              lambda t: t["band_round_items"] == 2 and pair_lists(t) == (2, 2, 2) and t["ksplit"] == 1),
    "colpair_missing_free": ("n2p19_free", False, {"t2": 0, "colpair_round_items": 2}, "f4_colpair",
                             lambda t: t["band_round_items"] == 4 and pair_lists(t) == (2, 2, 2)),
    # every block routed to the quad kernel: no pair keeps a block, and the run reports the quad kernel
    "colpair_routed": ("n2p19_free", False, {"ksplit": 0, "t2": 3, "colpair_round_items": 2}, "f4_quad",
                       lambda t: t["band_round_items"] == 0 and pair_lists(t) == (0, 0, 0)),
    "defaults": ("n2p19", False, {}, None, lambda t: True),
    "defaults_missing_free": ("n2p19_free", False, {}, None, lambda t: True),
}


class TestGpu:
    pytestmark = pytest.mark.gpu

    @pytest.fixture(scope="class", autouse=True)
    def one_hip_runtime(self):
        import torch
        torch.cuda.init()  # before libnldsc_amd.so binds to a HIP runtime (tests/test_gpu_parity.py)
        yield
        for cache in (_runs, _truth, _data):  # (~200 MB of rows and results)
            cache.clear()

    @pytest.mark.parametrize("dom", [True, False], ids=["dom", "additive"])
    @pytest.mark.parametrize("case", ["n2p19", "n2p19_free"])
    def test_largest_unsegmented_rows_vs_truth(self, case, dom):
        """N = 2^19, 4 096 chunks: the last length the fp32 accumulators take whole, entries above 0.9 x 2^23, in one
        launch of single-block items."""
        flags = F_F4 | F_RARE | (0 if dom else F_ADD)
        got, t = run(case, flags, SINGLE, "f4")
        assert t["ksplit"] == 1 and t["band_round_items"] == 0 and t["band_items"] == 6, t
        record(f"saturation_{case}_{'dom' if dom else 'additive'}",
               check_exact(got, truth(case), f"{case} single-block dom={dom}", dom))

    @pytest.mark.parametrize("path", sorted(PATHS))
    def test_unsegmented_paths_bitwise_single_block(self, path):
        """The same rows under each other unsegmented path the engine offers at this size — the K-split (partial fp32
        tiles summed by band_f4_epi_kernel; 6 items never fill the wave slots, so it is the default), column-block
        pairs, one launch against round launches, and on the missing-free rows the 2 x 2, routed and quad super-item
        kernels — bitwise the single-block launch, which test_largest_unsegmented_rows_vs_truth holds to the truth."""
        case, add, opts, kernel, holds = PATHS[path]
        flags = F_F4 | F_RARE | (F_ADD if add else 0)
        ref, _ = run(case, flags, SINGLE, "f4")
        got, t = run(case, flags, opts, kernel)
        assert holds(t), t
        bitwise(got, ref, path)

    @pytest.mark.parametrize("dom", [True, False], ids=["dom", "additive"])
    @pytest.mark.parametrize("case", SEGMENTED)
    def test_segmented_rows_vs_truth(self, case, dom):
        """N > 2^19: the first segmented lengths (4 098 chunks: a final segment of 2), three segments with entries
        above 2^24 and nine with entries near 2^26; add+dom folds into int32, additive-only into packed 16-bit
        counters whose quotients grow with N."""
        got, t = run(case, F_F4 | F_RARE | (0 if dom else F_ADD), None, "f4_seg")
        assert t["path"] == "f4" and t["ksplit"] == 1, t
        record(f"saturation_{case}_{'dom' if dom else 'additive'}",
               check_exact(got, truth(case), f"{case} dom={dom}", dom))

    @pytest.mark.parametrize("case", ["n2p19", "n1500001"])
    def test_int8_gram_is_the_same(self, case):
        """The int8 path (int32 accumulators throughout, an independent route) gives the same Gram."""
        from test_gpu_parity import same_gram
        a, t = run(case, F_I8 | F_RARE, None, "i8")
        b, _ = run(case, F_F4 | F_RARE, SINGLE if CASES[case][0] <= 1 << 19 else None)
        same_gram(a, b, case)
        record(f"saturation_{case}_i8", check_exact(a, truth(case), f"{case} int8"))

    def test_plink_order_on_misleading_heads(self):
        """FLAG_STRICT_PLINK_ORDER on the N = 2^19 rows: the run recounts the oriented rows and rewrites their last
        byte for its sample order; then the reference's order again on the same resident image."""
        from nldsc_amd.engine import Engine
        case = "n2p19"
        rows, bed, pos, N, M, rsq = dataset(case)
        args = (LD_WIND, 0.0, STD_THR, rsq, pos)
        with Engine(0) as e:
            e.load_bed_bytes(bed, M, N)
            strict = e.run(*args, flags=F_F4 | F_RARE | F_STRICT)
            compat = e.run(*args, flags=F_F4 | F_RARE)
        record(f"saturation_{case}_strict", check_exact(strict, truth(case, strict=True), f"{case} strict"))
        check_exact(compat, truth(case), f"{case} after a strict run")

    def test_round_launches_on_saturated_rows(self):
        """Launches of one round of wave slots need 8 single-block items per CU (2 048 on the MI355X); the 70 rows of
        the N = 2^19 case repeated to 2 048 SNPs give 2 080 — one full round and a tail — with the same saturated
        entries in every tile.  Bitwise one launch of all items (option band_rounds 0), and SNP j's scores follow from
        the 70-SNP truth: its neighbours are 29 or 30 copies of each row (one fewer of its own residue)."""
        from nldsc_amd.engine import Engine
        from nldsc_amd import synth
        case, reps = "n2p19", 2048
        rows, _, _, N, M, rsq = dataset(case)
        big = synth.bed_bytes(np.tile(rows, (reps // M + 1, 1))[:reps])
        pos = np.arange(reps, dtype=np.float64) * 1e-4
        out = {}
        for rounds in (1, 0):  # (without round launches the cost model would K-split the whole band: ksplit 0)
            with Engine(0, options={"t2": 0} if rounds else {"t2": 0, "band_rounds": 0, "ksplit": 0}) as e:
                e.load_bed_bytes(big, reps, N)
                out[rounds] = e.run(LD_WIND, 0.0, STD_THR, rsq, pos, flags=F_F4 | F_RARE)
                t = e.timings()
                assert (t["band_round_items"] > 0) == bool(rounds) and t["band_items"] == 2080, t
                assert t["band_kernel"] == "f4" and t["ksplit"] == 1, t
        bitwise(out[1], out[0], "round launches")
        exp = multiplicity_truth(exact_pairs(rows, N), reps, rsq, truth(case))
        # the same exact-path bar per SNP, over 2 047 neighbours here
        check_multiplicity(out[1], exp, "round launches")
