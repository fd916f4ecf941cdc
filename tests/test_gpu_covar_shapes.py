"""Covariate-adjusted LD scores past 16 covariates and 1 000-sample rows: the scores of nldsc_engine_run_covar where
tests/test_gpu_covar.py checks the projections only.

band_f4_epi_cov_kernel stages U and W' through LDS in chunks of COV_CHUNK = 16 covariates; the score tests of
test_gpu_covar.py have at most 7, so its chunk loop runs once in each of them.  Here the scores are compared with the
truth at q = 16, 17, 33, 48, 64 (whole chunks, one covariate in the last chunk, the cap), on rows of 67, 4 099, 32 773
and 2^19 - 1 samples, on missing-free blocks beside blocks with missing calls, on both stored orientations, on rare
variants whose exact residual std is 0, and with std_thr inside the range of the residual stds.

Truth and bars are test_gpu_covar.py's: cov_truth on explicit N-vectors with the basis of np.linalg.qr (the same basis
goes to the engine, so U and W compare column by column), scores within 1e-9 + 1e-12 |expected| under the condition
v, w >= 0.25 on every computed SNP (asserted on the truth before comparing), projections within projection_bounds.

Covariates (covariates()): q - 3 standard-normal columns, then the top two principal components of the standardised
genotype matrix, then SNP 17's additive vector plus unit normal noise.  np.linalg.qr keeps the column order, so the
structured columns — the ones that move r by more than sqrt(q) / N — are the last of the basis and land in the last,
partial chunk of the epilogue; at q = 17 the second chunk holds the SNP-17 column alone.  Every score case asserts that
the plain run misses the truth by more than 1e-4 in L2.
"""
import ctypes
import os
import shutil
import time

import numpy as np
import pytest

from conftest import GOLDEN, rare_variant_set, record
from oracle import oracle as O
from test_gpu_covar import (ADDITIVE_ONLY, E_ARG, EXACT_RARE, KEYS, STRICT, _ld, assert_bitwise, assert_projections,
                            assert_scores, bitwise, cov_truth, dataset, engines, forget_set, load,  # noqa: F401
                            projection_bounds, qr_basis, random_set, register_set, vectors)
from test_gpu_parity import missing_free_blocks

pytestmark = pytest.mark.gpu

FLOOR = 0.25        # the condition the 1e-9 bar was derived under: v, w of every computed SNP
SNP = 17            # the SNP whose additive vector (plus noise) is the last covariate
CAP_N = 2 ** 19 - 1  # the longest rows a covariate run takes


# ---- data sets ------------------------------------------------------------------------------------------------------
def blocks_set(missing_free):
    """N = 4 099, M = 352 (11 blocks): allele frequencies uniform in 0.08 .. 0.92, 2 % missing calls but in every third
    32-SNP block (missing_free "third") or nowhere ("all"); the same genotypes otherwise."""
    from nldsc_amd import synth
    M, N = 352, 4099
    rng = np.random.default_rng(4099)
    f = rng.uniform(0.08, 0.92, M)
    g = ((rng.random((M, N)) < f[:, None]).astype(np.int8) + (rng.random((M, N)) < f[:, None]).astype(np.int8))
    miss = rng.random((M, N)) < 0.02
    pos = np.cumsum(rng.exponential(0.05, M))
    if missing_free == "third":
        miss[(np.arange(M) // 32) % 3 == 0] = False
    else:
        miss[:] = False
    g[miss] = -1
    return synth.pack_bed_rows(g), pos, (1.0, 0.01, 1e-5, 1.0 / M), N


def cap_rows():
    """(rows of 2^19 - 1 individuals, the same rows with one more individual, positions, arguments): M = 40, allele
    frequencies 0.7 .. 0.95 (code 11 dominant in the file's coding), 1 % missing, every pair inside the window."""
    from nldsc_amd import synth
    M, N = 40, CAP_N + 1
    rng = np.random.default_rng(19)
    f = rng.uniform(0.7, 0.95, M)
    g = np.empty((M, N), np.int8)
    for j in range(M):
        g[j] = (rng.random(N) < f[j]).astype(np.int8) + (rng.random(N) < f[j]).astype(np.int8)
        g[j, rng.random(N) < 0.01] = -1
    return synth.pack_bed_rows(g[:, :CAP_N]), synth.pack_bed_rows(g), 0.01 * np.arange(M), (1.0, 0.01, 1e-5, 1.0 / M)


def registered(name):
    """dataset(name) for the sets of this module too."""
    if name in ("blocks_mixed", "blocks_free"):
        register_set(name, *blocks_set("third" if name == "blocks_mixed" else "all"))
    elif name.startswith("rare"):
        N = int(name[4:])
        rows, pos = rare_variant_set(N, 400, 5)
        register_set(name, rows, pos, (1.0, 0.0, 1e-5, 1.0 / 400), N)
    return dataset(name)


SEEDS = {("n67", 17): 3}  # (the default seed, 1000 + q, leaves v_17 = 0.39 at N = 67: below the 0.4 asserted at q = 17)


def covariates(name, q, seed=None):
    """[N, q]: q - 3 standard normal columns; the top two principal components of the standardised genotype matrix;
    SNP 17's additive coding plus unit normal noise (test_gpu_covar.seven_covariates at any q).  The rare-variant
    sets take the components of their common SNPs (the odd ones, MAF >= 0.05), as a PCA of real data would: rare
    alleles that share a carrier make that one individual a top component of the whole matrix, which leaves v = 0.21
    at SNP 216 of rare1003 whatever the seed — below the floor the bar is derived under."""
    A = vectors(name)[0]
    N = A.shape[1]
    rng = np.random.default_rng(SEEDS.get((name, q), 1000 + q) if seed is None else seed)
    pcs = np.linalg.svd(A[1::2] if name.startswith("rare") else A, full_matrices=False)[2][:2].T
    return np.concatenate([rng.standard_normal((N, q - 3)), pcs, (A[SNP] + rng.standard_normal(N))[:, None]], axis=1)


_truth: dict = {}


def truth(name, q):
    """(Q, cov_truth(name, Q), seconds it took), once per data set and q; the floor asserted."""
    if (name, q) not in _truth:
        t0 = time.perf_counter()
        registered(name)
        Q = qr_basis(covariates(name, q))
        exp = cov_truth(name, Q)
        comp = exp["l2_ws"] >= 0
        res = comp & (exp["residuals_std"] > 0)
        assert comp.sum() >= 30 and res.any()
        assert (exp["v"][comp] >= FLOOR).all() and (exp["w"][res] >= FLOOR).all(), \
            (name, q, exp["v"][comp].min(), exp["w"][res].min())
        exp["floor"] = (float(exp["v"][comp].min()), float(exp["w"][res].min()))
        _truth[(name, q)] = (Q, exp, time.perf_counter() - t0)
    return _truth[(name, q)]


def plain_gap(engine, name, exp):
    """The plain run's distance from the covariate truth in L2 (more than 1e-4: the adjustment is no rounding-level
    effect, a no-op cannot pass) and the plain run."""
    rows, pos, args, N, bed = dataset(name)
    plain = engine.run(*args, pos, flags=STRICT | EXACT_RARE)
    gap = float(np.nanmax(np.abs(plain["l2"] - exp["l2"])))
    assert gap > 1e-4, (name, gap)
    return gap, plain


def score_case(engines, name, q, orients, additive=False, label=None):
    """The covariate run of (name, q) on engines[orient] for every orient: scores and projections against the truth,
    additive-only too when asked.  Returns (record, orient -> the run)."""
    rows, pos, args, N, bed = registered(name)
    Q, exp, t_truth = truth(name, q)
    label = label or f"{name} q={q}"
    gots = {}
    bounds = projection_bounds(name, Q)
    rec = dict(N=N, M=len(rows), q=q, truth_s=t_truth, min_v=exp["floor"][0], min_w=exp["floor"][1], v_snp=float(exp["v"][SNP]))
    for orient in orients:
        e = engines[orient]
        load(e, name)
        if "plain_gap" not in rec:
            rec["plain_gap"], plain = plain_gap(e, name, exp)
        got = gots[orient] = e.run(*args, pos, covar=Q)
        rec[f"orient {orient}"] = assert_scores(got, exp, args[3], f"{label} orient {orient}")
        rec[f"orient {orient}"]["projections"] = assert_projections(e.covar_projections(q), bounds,
                                                                    f"{label} orient {orient}")
        assert bitwise(got["maf"], plain["maf"]) and bitwise(got["l2_ws"], plain["l2_ws"])
        if additive:
            add = e.run(*args, pos, flags=ADDITIVE_ONLY, covar=Q)
            rec[f"orient {orient} additive_only"] = assert_scores(add, exp, args[3], f"{label} orient {orient} additive-only",
                                                                  dom=False)
    return rec, gots


# ---- 1. the chunk edges of the epilogue -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,q", [("n1001", 16), ("n1001", 17), ("n1003", 33), ("n1000", 48), ("n1002", 64)])
def test_chunk_edges(engines, name, q):
    """q = 16: one whole chunk; 17: one covariate in the second; 33: one in the third; 48: three whole; 64: the cap."""
    t0 = time.perf_counter()
    Q, exp, _ = truth(name, q)
    if q == 17:
        assert 0.4 < exp["v"][SNP] < 0.6, exp["v"][SNP]
    rec, _ = score_case(engines, name, q, (0, 1), additive=q in (17, 64))
    rec["seconds"] = time.perf_counter() - t0
    record(f"covar_shapes_chunk_{name}_q{q}", rec)


# ---- 2. row lengths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,q", [("n67", 17), ("n32773", 33)])
def test_row_lengths(engines, name, q):
    """Rows shorter than one 128-sample chunk of the projection kernel; rows the band splits into several K pieces."""
    t0 = time.perf_counter()
    Q, exp, _ = truth(name, q)
    if q == 17:
        assert 0.4 < exp["v"][SNP] < 0.6, exp["v"][SNP]
    rec, _ = score_case(engines, name, q, (0, 1))
    t = engines[1].timings()
    rec.update(band_kernel=t["band_kernel"], ksplit=t["ksplit"])
    if name == "n32773":
        assert t["band_kernel"] == "f4_ksplit" and t["ksplit"] > 1, (t["band_kernel"], t["ksplit"])
    else:
        assert t["ksplit"] == 1, t["ksplit"]
    rec["seconds"] = time.perf_counter() - t0
    record(f"covar_shapes_rows_{name}_q{q}", rec)


# ---- 3. missing-free blocks beside blocks with missing calls --------------------------------------------------------
@pytest.mark.parametrize("name", ["blocks_mixed", "blocks_free"])
def test_missing_free_and_mixed_blocks(engines, name):
    """Blocks whose m-products the Gram skips (their missing plane sum is 0) beside blocks with missing calls, and a
    set without any missing call."""
    t0 = time.perf_counter()
    rows, pos, args, N, bed = registered(name)
    M = len(rows)
    miss = (O.unpack_codes(rows, N, strict=True) == 1).any(axis=1)
    per_block = np.array([miss[32 * b:32 * b + 32].any() for b in range((M + 31) // 32)])
    if name == "blocks_mixed":
        assert (per_block == (np.arange(len(per_block)) % 3 != 0)).all()
        assert missing_free_blocks(rows, N) == 4 and miss[(np.arange(M) // 32) % 3 != 0].all()
    else:
        assert not per_block.any() and missing_free_blocks(rows, N) == len(per_block) == 11
    rec, _ = score_case(engines, name, 19, (0, 1))
    # (score_case: the covariate run's WSA and MAF equal the plain run's, bitwise)
    rec["seconds"] = time.perf_counter() - t0
    record(f"covar_shapes_{name}_q19", rec)


# ---- 4. the row-length limit ----------------------------------------------------------------------------------------
def test_row_length_limit(engines):
    """N = 2^19 - 1 on the file's orientation (code 11 dominant: the partial Gram tiles sum to ~0.8 x 2^23 in fp32);
    the same rows with one more individual are rejected, and the engine runs on."""
    from nldsc_amd._lib import NLDSCError
    t0 = time.perf_counter()
    name, q, e = "cap", 18, engines[0]
    rows, rows_over, pos, args = cap_rows()
    M = len(rows)
    register_set(name, rows, pos, args, CAP_N)
    try:
        codes = O.unpack_codes(rows, CAP_N, strict=True)
        assert ((codes == 3).sum(1) > 0.45 * CAP_N).all()  # 16 x (count of 11 . 11) ~ 0.8 x 2^23 at f ~ 0.95
        rec, gots = score_case(engines, name, q, (0,))
        got = gots[0]
        Q = truth(name, q)[0]
        t = e.timings()
        rec.update(band_kernel=t["band_kernel"], ksplit=t["ksplit"], largest_gram=float(16 * (codes == 3).sum(1).max()) / 2 ** 23)
        del codes
        e.load_bed_bytes(b"\x6c\x1b\x01" + rows_over.tobytes(), M, CAP_N + 1)
        with pytest.raises(NLDSCError) as ex:
            e.run(*args, pos, covar=np.concatenate([Q, np.zeros((1, q))]))
        assert ex.value.code == E_ARG and "n_org < 2^19" in str(ex.value), str(ex.value)
        load(e, name)
        assert_bitwise(e.run(*args, pos, covar=Q), got, "the run after the rejection")
    finally:
        forget_set(name)
        _truth.pop((name, q), None)
    rec["seconds"] = time.perf_counter() - t0
    record("covar_shapes_cap_q18", rec)


# ---- 5. rare variants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 1003])
def test_rare_variants(engines, N):
    """A covariate run takes the closed-form vectors of rare variants: the SNPs whose exact residual std is 0 (at most
    two observed genotypes) report RSTD 0, count in no WSD and add nothing to a neighbour's L2D."""
    t0 = time.perf_counter()
    name, q = f"rare{N}", 20
    rows, pos, args, _, bed = registered(name)
    Q, exp, _ = truth(name, q)
    st = vectors(name)[2]
    comp = exp["l2_ws"] >= 0
    zero = comp & (st["rstd"] == 0)
    assert zero.sum() >= 100 and (comp & ~zero).sum() >= 100, (int(zero.sum()), int(comp.sum()))
    assert (exp["residuals_std"][zero] == 0).all() and (exp["l2d_ws"][comp] < exp["l2_ws"][comp]).any()
    ld_wind, std_thr = args[0], args[2]
    assert (exp["residuals_std"][comp & ~zero] > std_thr).all()  # (so WSD = WSA minus the neighbours of residual std 0)
    s = O.f64_setup(rows, N, ld_wind, args[1], std_thr, pos, strict=True)
    nb_zero = np.zeros(len(rows), np.int64)
    for j in np.flatnonzero(comp):
        ks = np.arange(s["L"][j], s["R"][j] + 1)
        ks = ks[s["passed"][ks] & (np.abs(pos[ks] - pos[j]) <= ld_wind) & (ks != j)]
        nb_zero[j] = zero[ks].sum()
    assert (nb_zero[comp] > 0).all()
    rec, gots = score_case(engines, name, q, (0, 1))
    for orient, got in gots.items():
        assert (got["residuals_std"][zero] == 0).all(), orient
        assert np.array_equal(got["l2d_ws"][comp], got["l2_ws"][comp] - nb_zero[comp]), orient
        # a neighbour of residual std 0 that were counted would add r2adj(0) = -1 / (n' - 2) ~ -1e-3 to L2D: the 1e-9
        # bar of assert_scores excludes it; the sum of every L2D against the truth's once more, as one number
        m = ~np.isnan(exp["l2d"])
        assert abs(got["l2d"][m].sum() - exp["l2d"][m].sum()) <= 1e-9 * m.sum(), orient
    rec.update(zero_rstd=int(zero.sum()), computed=int(comp.sum()), seconds=time.perf_counter() - t0)
    record(f"covar_shapes_rare{N}_q20", rec)


# ---- 6. the residual-pass flag at its threshold ---------------------------------------------------------------------
def test_residual_flag_near_its_threshold(engines):
    """covar_finish_kernel re-takes flag bit 1 on the residual std scaled by sqrt(w).  std_thr between the adjusted and
    the plain residual std of several SNPs: WSD, L2D and WSDE follow the adjusted value."""
    t0 = time.perf_counter()
    name, q = "n1001", 17
    rows, pos, args, N, bed = dataset(name)
    Q, exp, _ = truth(name, q)
    comp = exp["l2_ws"] >= 0
    adj, plain_std = exp["residuals_std"], vectors(name)[2]["rstd"]
    s = np.sort(adj[comp & (adj > 0)])
    # the middle of the first gap from the median on that is 1e-9 relative wide and as far from every plain std
    thr = next(t for t, lo, hi in zip(0.5 * (s[:-1] + s[1:])[len(s) // 2:], s[len(s) // 2:-1], s[len(s) // 2 + 1:])
               if hi - lo >= 2e-9 * t and np.abs(plain_std[comp] - t).min() >= 1e-9 * t)
    assert (np.abs(adj[comp] - thr) >= 1e-9 * thr).all()
    flips = comp & (plain_std > thr) & ~(adj > thr)
    assert flips.sum() >= 5, int(flips.sum())
    register_set(name + "_std", rows, pos, (args[0], args[1], float(thr), args[3]), N)
    args = dataset(name + "_std")[2]
    exp = cov_truth(name + "_std", Q)
    assert (exp["l2d_ws"][comp] < _truth[(name, q)][1]["l2d_ws"][comp]).sum() >= 5
    rec = dict(std_thr=float(thr), flips=int(flips.sum()), below=int((comp & ~(adj > thr)).sum()))
    for orient, e in engines.items():
        load(e, name + "_std")
        plain = e.run(*args, pos, flags=STRICT | EXACT_RARE)
        got = e.run(*args, pos, covar=Q)
        rec[f"orient {orient}"] = assert_scores(got, exp, args[3], f"{name} std_thr {thr:.6g} orient {orient}")
        # the plain run's flag is the unadjusted one: it counts the flipped SNPs, the covariate run must not
        assert (plain["l2d_ws"] >= got["l2d_ws"]).all() and (plain["l2d_ws"] > got["l2d_ws"]).sum() >= 5
        assert np.array_equal(np.isnan(got["residuals_std"]), np.isnan(plain["residuals_std"]))
    rec["seconds"] = time.perf_counter() - t0
    record("covar_shapes_residual_flag", rec)


# ---- 7. schedule independence at q = 40, bitwise --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["blocks_mixed", "n32773"])
def test_schedule_independence(name):
    from nldsc_amd.engine import Engine
    t0 = time.perf_counter()
    q = 40
    rows, pos, args, N, bed = registered(name)
    Q, exp, _ = truth(name, q)
    M = len(rows)

    def run(options, owns=None):
        with Engine(0, options=options) as e:
            e.load_bed_bytes(bed, M, N)
            if owns is None:
                return e.run(*args, pos, covar=Q), e.timings()
            out = None
            for own in owns:
                r = e.run(*args, pos, covar=Q, own=own)
                if out is None:
                    out = r
                else:
                    for k in KEYS:
                        out[k][own[0]:own[1]] = r[k][own[0]:own[1]]
            return out, None

    base, t = run({})
    rec = dict(scores=assert_scores(base, exp, args[3], f"{name} q={q} default schedule"), ksplit=t["ksplit"])
    for options in ({"cov_batch_items": 1}, {"cov_batch_items": 7}, {"ksplit": 0}, {"gpu_plan": 0}, {"plan_fused": 0}):
        got, to = run(options)
        assert_bitwise(got, base, f"{name} {options}")
        if "ksplit" in options:
            assert to["ksplit"] == 1
            rec["ksplit_off"] = to["ksplit"]
    cut = 32 * (M // 64) + 13  # inside a 32-SNP block
    for owns in ([(0, 1), (1, M - 1), (M - 1, M)], [(0, cut), (cut, M)]):
        assert_bitwise(run({}, owns=owns)[0], base, f"{name} owned ranges {owns}")
    rec["seconds"] = time.perf_counter() - t0
    record(f"covar_shapes_schedule_{name}_q{q}", rec)


# ---- 8. the one-shot entry ------------------------------------------------------------------------------------------
def test_one_shot_entry(engines):
    """nldsc_ld_calculate_covar (engine.calculate(covar=...)) against Engine.run on the same file, without and with a
    keep list; the caller's flags 0 in both (each sets PLINK's sample order itself)."""
    from nldsc_amd.engine import calculate
    t0 = time.perf_counter()
    name, q, e = "n1001", 17, engines[1]
    rows, pos, args, N, bed = dataset(name)
    Q, exp, _ = truth(name, q)
    M, path = len(rows), os.path.join(GOLDEN, name + ".bed")
    try:
        e.set_keep(None)
        e.load_bed_file(path, M, N)
        ref = e.run(*args, pos, covar=Q, flags=0)
        one = calculate(path, M, N, *args, pos, flags=0, device=0, covar=Q)
        assert_bitwise(one, ref, "calculate(covar) against Engine.run(covar)")
        rec = dict(scores=assert_scores(one, exp, args[3], f"{name} one-shot"))
        idx = np.sort(np.random.default_rng(21).choice(N, N // 2, replace=False)).astype(np.int32)
        Qk = qr_basis(covariates(name, q)[idx])
        e.set_keep(idx, N)
        e.load_bed_file(path, M, N)
        assert e.n_org == len(idx)
        kept = e.run(*args, pos, covar=Qk, flags=0)
        one = calculate(path, M, N, *args, pos, flags=0, device=0, keep=idx, covar=Qk)
        assert np.isfinite(kept["l2"]).sum() > 1000 and not bitwise(kept["l2"], ref["l2"])
        assert_bitwise(one, kept, "calculate(keep, covar) against the keep-loaded Engine.run(covar)")
    finally:
        e.set_keep(None)
    rec["seconds"] = time.perf_counter() - t0
    record("covar_shapes_one_shot", rec)


# ---- 9. the whole genome from the CLI -------------------------------------------------------------------------------
def test_cli_whole_genome(tmp_path):
    """`ld --bfile chr@ --covar FILE --out out@.L2` on two chromosomes with one .fam: each table byte-equal to the
    single-chromosome run's; a second chromosome whose .fam has two lines swapped fails the run before any table."""
    t0 = time.perf_counter()
    sets = {"1": "n1000", "2": "allmiss"}  # both 1 000 individuals, cM positions
    fam = open(os.path.join(GOLDEN, "n1000.fam")).read()
    assert fam == open(os.path.join(GOLDEN, "allmiss.fam")).read()
    for sub in ("ok", "bad"):
        (tmp_path / sub).mkdir()
        for c, name in sets.items():
            for ext in (".bed", ".bim"):
                shutil.copy(os.path.join(GOLDEN, name + ext), tmp_path / sub / f"chr{c}{ext}")
            (tmp_path / sub / f"chr{c}.fam").write_text(fam)
    lines = fam.splitlines(keepends=True)
    lines[3], lines[500] = lines[500], lines[3]
    (tmp_path / "bad" / "chr2.fam").write_text("".join(lines))
    ids = [line.split()[:2] for line in fam.splitlines() if line.strip()]
    C = covariates("n1000", 20)
    assert len(ids) == C.shape[0]
    covar = tmp_path / "pcs.covar"
    covar.write_text("".join(f"{f} {i} " + " ".join(repr(float(x)) for x in row) + "\n" for (f, i), row in zip(ids, C)))
    common = ["--ld-wind-cm", "1", "-maf", "0.01", "-std", "1e-5", "--extra", "--quiet", "--covar", str(covar)]
    p = _ld(common + ["--bfile", str(tmp_path / "ok" / "chr@"), "--out", str(tmp_path / "out@.L2")])
    assert "q = 20" in p.stderr, p.stderr[-2000:]
    for c in sets:
        _ld(common + ["--bfile", str(tmp_path / "ok" / f"chr{c}"), "--out", str(tmp_path / f"single{c}.L2")])
        whole, single = (tmp_path / f"out{c}.L2").read_bytes(), (tmp_path / f"single{c}.L2").read_bytes()
        assert len(single) > 10_000 and whole == single, f"chromosome {c}"
    assert (tmp_path / "out1.L2").read_bytes() != (tmp_path / "out2.L2").read_bytes()
    p = _ld(common + ["--bfile", str(tmp_path / "bad" / "chr@"), "--out", str(tmp_path / "bad@.L2")], expect_ok=False)
    assert "crashed" in p.stderr and "lists other individuals" in p.stderr, (p.stderr + p.stdout)[-2000:]
    assert not (tmp_path / "bad2.L2").exists() and not (tmp_path / "bad1.L2").exists()
    record("covar_shapes_cli_genome", dict(seconds=time.perf_counter() - t0))


# ---- 10. the rejections test_gpu_covar.py leaves out ----------------------------------------------------------------
def raw_call(engine, args, pos, basis, n_covar, flags):
    """nldsc_engine_run_covar itself (Engine.run sets NLDSC_FLAG_STRICT_PLINK_ORDER and never passes NULL):
    (return code, message, result arrays); basis: [n_covar][n_org] float64 or None."""
    from nldsc_amd import _lib
    n = engine.n_snp
    p, _keep = _lib.make_params(n, engine.n_org, args[0], args[1], args[2], args[3], pos, flags=flags)
    arrs, res = _lib.alloc_result(n)
    err = _lib.errbuf()
    rc = engine._L.nldsc_engine_run_covar(engine._h, ctypes.byref(p), None if basis is None else basis.ctypes.data,
                                          int(n_covar), 0, n, ctypes.byref(res), err, len(err))
    return rc, err.value.decode(), arrs


def test_rejections(engines):
    from nldsc_amd import synth
    from nldsc_amd._lib import NLDSCError
    e = engines[1]
    rng = np.random.default_rng(10)
    rows, pos = random_set(64, 20, 20)  # 20 individuals
    e.set_keep(None)
    e.load_bed_bytes(synth.bed_bytes(rows), 64, 20)
    with pytest.raises(NLDSCError) as ex:
        e.run(1.0, 0.01, 1e-5, 1.0 / 64, pos, covar=qr_basis(rng.standard_normal((20, 18))))
    assert ex.value.code == E_ARG and "n_covar 18 leaves fewer than 3 degrees of freedom of 20 individuals" in \
        str(ex.value), str(ex.value)
    name = "n1000"
    pos, args = load(e, name)
    N = dataset(name)[3]
    Q = qr_basis(rng.standard_normal((N, 4)))
    basis = np.ascontiguousarray(Q.T)
    rc, msg, _ = raw_call(e, args, pos, basis, 4, flags=0)
    assert rc == E_ARG and "NLDSC_FLAG_STRICT_PLINK_ORDER" in msg and "PLINK's sample order" in msg, (rc, msg)
    rc, msg, _ = raw_call(e, args, pos, None, 4, flags=STRICT)
    assert rc == E_ARG and "q_basis is NULL" in msg, (rc, msg)
    rc, msg, got = raw_call(e, args, pos, basis, 4, flags=STRICT)  # (the same call, complete: and the engine still runs)
    assert rc == 0, (rc, msg)
    assert np.isfinite(got["l2"]).sum() > 1000
    assert_bitwise(got, e.run(*args, pos, covar=Q), "the raw call against Engine.run")
