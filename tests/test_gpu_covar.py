"""Covariate-adjusted LD scores (nldsc_engine_run_covar, --covar): every genotype vector residualised on the run's
covariates before the correlations (cov-LDSC, here also for the dominance scores).

Truth: explicit N-vectors in numpy.  A_j, R_j from oracle.unpack_codes(strict=True) and oracle.stats_from_counts
(missing calls 0), an orthonormal basis Q of the centred covariates from np.linalg.qr, U_j = Q^T A_j, W_j = Q^T R_j,
v_j = 1 - |U_j|^2 / N, gamma_j = -(W_j . U_j) / (N v_j), w_j = 1 - |W_j|^2 / N - gamma_j^2 v_j,
A~_j = (A_j - Q U_j) / sqrt(v_j), R~_j = (R_j - Q W_j - gamma_j (A_j - Q U_j)) / sqrt(w_j); the window sets of
oracle.f64_setup; r2adj with n' = N - q.

Bars.  Scores: the project's exact-path bar |d| <= 1e-9 + 1e-12 |expected|: with v_j, w_j >= 0.25 (asserted on the
truth before comparing; the deliberately collinear SNPs excepted) a pair's error is a few ulps of N eps / (N 0.25) ~
1e-15, and a window of at most ~10^3 neighbours stays three orders below 1e-9.  Projections: U_jc is a sum over the
individuals of Q_ic times one of four values; the engine forms it from three plane sums (the fourth class follows from
sum_i Q_ic = 0), each with a worst-case fp64 summation error of N 2^-53 sum_i |Q_ic| and a coefficient that is a
difference of two of the four values, at most 2 max |value|; numpy's own sum errs by as much.  Hence
|d| <= N 2^-52 sum_i |Q_ic| * 2 max_code |lut_j| (+ 8 eps |expected| for the final scaling)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, golden_sets, load_set, record
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")
STRICT, ADDITIVE_ONLY, EXACT_I8, FP32, EXACT_RARE = 1, 2, 4, 8, 32  # _lib.FLAG_*
E_ARG = -4
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def engines():
    """engines[orient]: rows stored as in the file (0) or minor-homozygote-as-00 (1, the default)."""
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)
    from nldsc_amd.engine import Engine
    es = {0: Engine(0, options={"orient": 0}), 1: Engine(0)}
    yield es
    for e in es.values():
        e.close()


@pytest.fixture(scope="module")
def engine(engines):
    return engines[1]


_sets: dict = {}


def random_set(M, N, seed, missing=0.02):
    """Independent SNPs with allele frequencies on both sides of 1/2 (rows stored flipped and unflipped)."""
    from nldsc_amd import synth
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.08, 0.92, M)
    g = ((rng.random((M, N)) < f[:, None]).astype(np.int8) + (rng.random((M, N)) < f[:, None]).astype(np.int8))
    g[rng.random((M, N)) < missing] = -1
    return synth.pack_bed_rows(g), np.cumsum(rng.exponential(0.05, M))


def dataset(name):
    """(rows, positions, run arguments (ld_wind, maf, std_thr, rsq_thr), n_org, bed bytes), made once."""
    if name not in _sets:
        from nldsc_amd import synth
        if name == "n67":  # rows shorter than one 128-sample chunk
            rows, pos = random_set(200, 67, 67)
            args, N, bed = (1.0, 0.01, 1e-5, 1.0 / 200), 67, synth.bed_bytes(rows)
        elif name == "n32773":  # N = 2^15 + 5: several K pieces, a ragged tail
            rows, pos = random_set(96, 2 ** 15 + 5, 32773)
            args, N, bed = (1.0, 0.01, 1e-5, 1.0 / 96), 2 ** 15 + 5, synth.bed_bytes(rows)
        else:
            bed, pos, meta, _, _ = load_set(name)
            rows = np.frombuffer(bed, np.uint8, offset=3).reshape(meta["n_snp"], -1)
            args, N = (meta["ld_wind"], meta["maf"], meta["std_thr"], meta["rsq_thr"]), meta["n_org"]
        _sets[name] = (rows, pos, args, N, bed)
    return _sets[name]


def register_set(name, rows, pos, args, N):
    """A data set of another module (tests/test_gpu_covar_shapes.py) under `name`: dataset, vectors and cov_truth then
    take it like the ones above."""
    from nldsc_amd import synth
    assert name not in golden_sets()
    if name not in _sets:
        _sets[name] = (rows, np.asarray(pos, np.float64), tuple(args), int(N), synth.bed_bytes(rows))
    return _sets[name]


def forget_set(name):
    """Drops a registered set and its vectors (a set whose N-vectors take hundreds of megabytes)."""
    _sets.pop(name, None)
    _vec.pop(name, None)


def load(engine, name):
    rows, pos, args, N, bed = dataset(name)
    engine.set_keep(None)
    engine.load_bed_bytes(bed, len(rows), N)
    return pos, args


def bitwise(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_bitwise(got, exp, label):
    for k in KEYS:
        assert bitwise(got[k], exp[k]), f"{label}: {k} differs at {np.flatnonzero(~((got[k] == exp[k]) | ((got[k] != got[k]) & (exp[k] != exp[k]))))[:10]}"


def qr_basis(C):
    """An orthonormal basis of the centred columns of C (full column rank), by np.linalg.qr."""
    C = np.asarray(C, dtype=np.float64)
    C = C - C.mean(axis=0)
    q, _ = np.linalg.qr(C)
    return np.ascontiguousarray(q - q.mean(axis=0))


_vec: dict = {}


def vectors(name):
    """(A, R, st): the standardised additive / dominance-residual N-vectors of every SNP (missing calls 0; rows of
    an all-missing SNP 0; R = 0 where the residual std is 0) and oracle.stats_from_counts."""
    if name not in _vec:
        rows, pos, args, N, bed = dataset(name)
        codes = O.unpack_codes(rows, N, strict=True).astype(np.int64)
        cnt = np.stack([(codes == k).sum(1) for k in range(4)], 1)
        st = O.stats_from_counts(cnt, N)
        la, lr = st["lut_a"].copy(), st["lut_r"].copy()
        lr[~(st["rstd"] > 0)] = 0.0
        la[np.isnan(la).any(axis=1)] = 0.0
        lr[np.isnan(lr).any(axis=1)] = 0.0
        la[:, 1] = lr[:, 1] = 0.0
        _vec[name] = (np.take_along_axis(la, codes, 1), np.take_along_axis(lr, codes, 1), st, (la, lr))
    return _vec[name]


def projections(A, R, Q, N, zero_a=1e-6):
    """U, W, v, gamma, w of the definition (v < zero_a: gamma := 0)."""
    U, W = A @ Q, R @ Q
    v = 1.0 - (U * U).sum(1) / N
    gam = np.where(v < zero_a, 0.0, -(W * U).sum(1) / (N * np.where(v < zero_a, 1.0, v)))
    w = 1.0 - (W * W).sum(1) / N - gam * gam * v
    return U, W, v, gam, w


def cov_truth(name, Q, dom=True):
    """The seven arrays of a covariate run from explicit N-vectors, plus v, w and per SNP the exact dominance r2adj of
    its counted neighbours ("r2d")."""
    rows, pos, args, N, bed = dataset(name)
    ld_wind, maf, std_thr, rsq_thr = args
    A, R, st, _ = vectors(name)
    s = O.f64_setup(rows, N, ld_wind, maf, std_thr, pos, strict=True)
    M, q = len(rows), Q.shape[1]
    U, W, v, gam, w = projections(A, R, Q, N)
    za, zr = v < 1e-6, (w < 1e-6) | ~(st["rstd"] > 0)
    At = np.where(za[:, None], 0.0, (A - U @ Q.T) / np.sqrt(np.where(za, 1.0, v))[:, None])
    Rt = np.where(zr[:, None], 0.0, (R - W @ Q.T - gam[:, None] * (A - U @ Q.T)) / np.sqrt(np.where(zr, 1.0, w))[:, None])
    rstd = np.where(zr, 0.0, st["rstd"] * np.sqrt(np.where(zr, 1.0, w)))
    rpass = rstd > std_thr
    n2 = float(N - q)
    adj = lambda r: 1.0 - (1.0 - r * r) * ((n2 - 1.0) / (n2 - 2.0))  # noqa: E731
    o = dict(l2=np.full(M, np.nan), l2d=np.full(M, np.nan), maf=np.where(s["used"], st["maf"].astype(np.float64), np.nan),
             residuals_std=np.where(s["passed"], rstd, np.nan), l2_ws=np.full(M, -1, np.int32),
             l2d_ws=np.full(M, -1, np.int32), l2d_wse=np.full(M, -1, np.int32), v=v, w=w, r2d=[None] * M)
    L, Rp, passed = s["L"], s["R"], s["passed"]
    for j in range(M):
        if L[j] < 0:
            continue
        ks = np.arange(L[j], Rp[j] + 1)
        ks = ks[passed[ks] & (np.abs(pos[ks] - pos[j]) <= ld_wind) & (ks != j)]
        o["l2"][j] = 1.0 + adj(At[ks] @ At[j] / N).sum()
        o["l2_ws"][j] = len(ks)
        if dom:
            kd = ks[rpass[ks]]
            r2d = adj(Rt[kd] @ At[j] / N)
            o["l2d"][j], o["l2d_ws"][j], o["l2d_wse"][j] = r2d.sum(), len(kd), int((r2d > rsq_thr).sum())
            o["r2d"][j] = r2d
    return o


def assert_scores(got, exp, rsq_thr, label, dom=True):
    """L2, L2D, residual std within 1e-9 + 1e-12 |expected| with equal NaN patterns; l2_ws, l2d_ws equal; l2d_wse equal
    but where a pair's exact r2adj lies within 1e-9 of rsq_thr (asserted per difference).  Returns the worst errors."""
    worst = {}
    for k in ("l2", "l2d", "residuals_std") if dom else ("l2", "residuals_std"):
        g, e = got[k], exp[k]
        assert np.array_equal(np.isnan(g), np.isnan(e)), f"{label} {k}: NaN pattern"
        m = ~np.isnan(e)
        err = np.abs(g[m] - e[m])
        lim = 1e-9 + 1e-12 * np.abs(e[m])
        worst[k] = float(err.max(initial=0))
        print(f"{label} {k}: worst |d| {worst[k]:.3g} ({int(m.sum())} values)")
        assert (err <= lim).all(), f"{label} {k}: {int((err > lim).sum())} out of tolerance, worst {worst[k]:.3g}"
    assert np.array_equal(got["l2_ws"], exp["l2_ws"]), f"{label}: l2_ws"
    if dom:
        assert np.array_equal(got["l2d_ws"], exp["l2d_ws"]), f"{label}: l2d_ws"
        diff = np.flatnonzero(got["l2d_wse"] != exp["l2d_wse"])
        for j in diff:
            ties = int((np.abs(exp["r2d"][j] - rsq_thr) <= 1e-9).sum())
            assert abs(int(got["l2d_wse"][j]) - int(exp["l2d_wse"][j])) <= ties, \
                f"{label}: l2d_wse[{j}] {got['l2d_wse'][j]} vs {exp['l2d_wse'][j]} with {ties} pairs at the threshold"
        worst["wse_ties"] = int(len(diff))
    else:
        assert np.isnan(got["l2d"]).all() and (got["l2d_ws"] == -1).all() and (got["l2d_wse"] == -1).all()
    return worst


def seven_covariates(name, seed=7):
    """four standard normal; the top two principal components of the standardised genotype matrix (its singular
    vectors over the individuals); SNP 17's additive coding plus unit normal noise (v_17 ~ 0.5)"""
    A, _, _, _ = vectors(name)
    N = A.shape[1]
    rng = np.random.default_rng(seed)
    pcs = np.linalg.svd(A, full_matrices=False)[2][:2].T
    return np.concatenate([rng.standard_normal((N, 4)), pcs, (A[17] + rng.standard_normal(N))[:, None]], axis=1)


# ---- 1. projections -------------------------------------------------------------------------------------------------
def projection_bounds(name, Q):
    """key -> (expected, bound) of Engine.covar_projections ("u", "w", "v", "wd") for the basis Q: the module
    docstring's bound on U and W, propagated into v and w."""
    rows, pos, args, N, bed = dataset(name)
    A, R, st, (la, lr) = vectors(name)
    U, W, v, gam, w = projections(A, R, Q, N)
    s = O.f64_setup(rows, N, args[0], args[1], args[2], pos, strict=True)
    live = s["passed"] & (st["counts"][:, [0, 2, 3]].sum(1) > 0)  # computed, not all-missing: the others report 0 / 1
    U, W = np.where(live[:, None], U, 0.0), np.where(live[:, None], W, 0.0)
    v, w = np.where(live, v, 1.0), np.where(live, w, 1.0)
    absq = np.abs(Q).sum(0)
    bU = N * 2.0 ** -52 * absq[None, :] * 2 * np.abs(la).max(1)[:, None] + 8 * EPS * np.abs(U)
    bW = N * 2.0 ** -52 * absq[None, :] * 2 * np.abs(lr).max(1)[:, None] + 8 * EPS * np.abs(W)
    # first-order propagation of those bounds into v and w (doubled for the second order), plus a few roundings
    bv = 2 * ((2 * np.abs(U) + bU) * bU).sum(1) / N + 16 * EPS
    bw = 2 * ((np.abs(-2 * W + 2 * gam[:, None] * U) * bW + np.abs(2 * gam[:, None] * W - 2 * (gam ** 2)[:, None] * U) * bU)
              .sum(1) / N + ((bW * bW).sum(1) + (bU * bU).sum(1)) / N) / np.minimum(np.maximum(v, 1e-6), 1.0) + 64 * EPS
    return {"u": (U, bU), "w": (W, bW), "v": (v, bv), "wd": (w, bw)}


def assert_projections(p, bounds, label):
    """Every array of p = Engine.covar_projections(q) finite and within its bound; key -> the worst error in units
    of the bound."""
    units = {}
    for key, (exp, b) in bounds.items():
        err = np.abs(p[key] - exp)
        units[key] = float((err / np.maximum(b, 1e-300)).max())  # (b = 0 with err = 0: an all-missing SNP's zeros)
        assert np.isfinite(p[key]).all() and (err <= b).all(), \
            f"{label} {key}: worst {units[key]:.3g} x the bound at {np.argwhere(err > b)[:5]}"
    return units


@pytest.mark.parametrize("q", [1, 5, 17, 40, 64])  # 1, 1, 2, 3 and 4 groups of 16 covariates; across a chunk edge; the cap
@pytest.mark.parametrize("name", ["n1000", "n1001", "n1002", "n1003", "allmiss", "n67", "n32773"])
def test_projections(engines, name, q):
    rows, pos, args, N, bed = dataset(name)
    A, R, st, (la, lr) = vectors(name)
    Q = qr_basis(np.random.default_rng(100 + q).standard_normal((N, q)))
    bounds = projection_bounds(name, Q)
    bU, bW = bounds["u"][1], bounds["w"][1]
    if name == "allmiss":
        s = O.f64_setup(rows, N, args[0], args[1], args[2], pos, strict=True)
        assert (st["counts"][:, [0, 2, 3]].sum(1) == 0).any() and s["passed"][st["counts"][:, [0, 2, 3]].sum(1) == 0].any()
    rec, got = {}, {}
    for orient, e in engines.items():
        load(e, name)
        e.run(*args, pos, covar=Q)
        p = got[orient] = e.covar_projections(q)
        for key, units in assert_projections(p, bounds, f"{name} q={q} orient={orient}").items():
            rec[f"{key} orient {orient}"] = units
        if name == "allmiss":
            dead = st["counts"][:, [0, 2, 3]].sum(1) == 0
            assert (p["u"][dead] == 0).all() and (p["w"][dead] == 0).all()
    assert (np.abs(got[0]["u"] - got[1]["u"]) <= 2 * bU).all() and (np.abs(got[0]["w"] - got[1]["w"]) <= 2 * bW).all()
    print(f"{name} q={q}: worst error in units of the bound {rec}")
    record(f"covar_projections_{name}_q{q}", rec)


# ---- 2. scores against the truth ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seven():
    out = {}

    def get(name):
        if name not in out:
            from nldsc_amd.ldscore.common import covar_basis
            C = seven_covariates(name)
            Qe, dropped = covar_basis(C)
            assert Qe.shape[1] == 7 and not dropped
            out[name] = (C, Qe, cov_truth(name, qr_basis(C)))
        return out[name]
    return get


@pytest.mark.parametrize("name", ["n1001", "n1003"])
def test_scores_against_truth(engine, seven, name):
    C, Qe, exp = seven(name)
    pos, args = load(engine, name)
    comp = exp["l2_ws"] >= 0
    assert comp.sum() > 1000 and (exp["v"][comp] >= 0.25).all() and (exp["w"][comp & (exp["residuals_std"] > 0)] >= 0.25).all()
    assert 0.4 < exp["v"][17] < 0.6
    plain = engine.run(*args, pos, flags=STRICT | EXACT_RARE)
    got = engine.run(*args, pos, covar=Qe)
    rec = dict(dom=assert_scores(got, exp, args[3], f"{name} covar"))
    assert bitwise(got["maf"], plain["maf"]) and bitwise(got["l2_ws"], plain["l2_ws"])
    # the adjustment is no rounding-level effect: a no-op (the plain run) misses the truth
    gap = np.nanmax(np.abs(plain["l2"] - exp["l2"]))
    assert gap > 1e-4, gap
    add = engine.run(*args, pos, flags=ADDITIVE_ONLY, covar=Qe)
    rec["additive_only"] = assert_scores(add, exp, args[3], f"{name} covar additive-only", dom=False)
    rec["plain_gap"] = float(gap)
    record(f"covar_truth_{name}", rec)


# ---- 3. basis invariance --------------------------------------------------------------------------------------------
def test_basis_invariance(engine, seven):
    from nldsc_amd.ldscore.common import covar_basis
    name = "n1001"
    C, Qe, exp = seven(name)
    pos, args = load(engine, name)
    rng = np.random.default_rng(3)
    N = C.shape[0]
    variants = {"mixed": C @ rng.standard_normal((7, 7)),
                "scaled_shifted": 1000.0 * C + rng.uniform(-50, 50, 7)[None, :],
                "duplicate_and_constant": np.concatenate([C, C[:, 2:3], np.full((N, 1), 3.5)], axis=1)}
    rec = {}
    for label, Cv in variants.items():
        Q, dropped = covar_basis(Cv)
        assert Q.shape[1] == 7, (label, Q.shape)  # the original rank
        if label == "duplicate_and_constant":
            assert dropped == [7, 8]
        rec[label] = assert_scores(engine.run(*args, pos, covar=Q), exp, args[3], f"{name} {label}")
    record("covar_basis_invariance", rec)


# ---- 4. a SNP collinear with the covariates -------------------------------------------------------------------------
def test_collinear_snp(engine):
    name = "n1003"
    rows, pos, args, N, bed = dataset(name)
    A, R, st, _ = vectors(name)
    s = O.f64_setup(rows, N, args[0], args[1], args[2], pos, strict=True)
    j = int(np.flatnonzero(s["L"] >= 0)[40])  # a computed SNP (its additive vector, 0 at its missing calls)
    C = np.concatenate([np.random.default_rng(9).standard_normal((N, 2)), A[j][:, None]], axis=1)
    Q = qr_basis(C)
    exp = cov_truth(name, Q)
    assert exp["v"][j] < 1e-6
    others = (exp["l2_ws"] >= 0) & (np.arange(len(rows)) != j)
    assert (exp["v"][others] >= 0.25).all() and (exp["w"][others & (exp["residuals_std"] > 0)] >= 0.25).all()
    pos, args = load(engine, name)
    plain = engine.run(*args, pos, flags=STRICT | EXACT_RARE)
    got = engine.run(*args, pos, covar=Q)
    rec = assert_scores(got, exp, args[3], f"{name} collinear SNP {j}")
    n2 = float(N - 3)
    r0 = 1.0 - (n2 - 1.0) / (n2 - 2.0)  # r2adj(0)
    assert got["l2_ws"][j] > 0 and abs(got["l2"][j] - (1.0 + got["l2_ws"][j] * r0)) <= 1e-9
    assert engine.covar_projections(3)["v"][j] < 1e-6
    for k in ("l2", "l2d", "residuals_std"):  # no NaN anywhere new
        assert np.array_equal(np.isnan(got[k]), np.isnan(plain[k])), k
    record("covar_collinear", rec)


# ---- 5. schedule independence, bitwise ------------------------------------------------------------------------------
def test_schedule_independence(seven):
    from nldsc_amd.engine import Engine
    name = "n1003"
    C, Qe, exp = seven(name)
    rows, pos, args, N, bed = dataset(name)
    M = len(rows)

    def run(options, owns=None):
        with Engine(0, options=options) as e:
            e.load_bed_bytes(bed, M, N)
            if owns is None:
                return e.run(*args, pos, covar=Qe)
            out = None
            for own in owns:
                r = e.run(*args, pos, covar=Qe, own=own)
                if out is None:
                    out = r
                else:
                    for k in KEYS:
                        out[k][own[0]:own[1]] = r[k][own[0]:own[1]]
            return out

    base = run({})
    assert_scores(base, exp, args[3], f"{name} default schedule")
    for options in ({"cov_batch_items": 7}, {"cov_batch_items": 1}, {"ksplit": 0}, {"gpu_plan": 0}, {"plan_fused": 0},
                    {"ksplit": 0, "gpu_plan": 0, "cov_batch_items": 7}):
        assert_bitwise(run(options), base, f"{name} {options}")
    a, b = M // 3, 2 * M // 3
    assert_bitwise(run({}, owns=[(0, a), (a, b), (b, M)]), base, f"{name} owned thirds")


# ---- 6. stateless ---------------------------------------------------------------------------------------------------
def test_stateless(engine, seven):
    name = "n1001"
    _, Qe, _ = seven(name)
    pos, args = load(engine, name)
    for flags in (0, STRICT, STRICT | EXACT_RARE):
        before = engine.run(*args, pos, flags=flags)
        cov = engine.run(*args, pos, covar=Qe)
        assert not bitwise(cov["l2"], before["l2"])
        assert_bitwise(engine.run(*args, pos, flags=flags), before, f"plain run after a covariate run, flags {flags}")


# ---- 7. keep --------------------------------------------------------------------------------------------------------
def test_keep_equals_the_subset_file(engine):
    from nldsc_amd import synth
    name = "n1001"
    rows, pos, args, N, bed = dataset(name)
    idx = np.sort(np.random.default_rng(12).choice(N, N // 2, replace=False)).astype(np.int32)

    def subset_rows(rows, n_org, idx):  # the .bed rows `plink --keep` writes
        geno_of_code = np.array([0, -1, 1, 2], np.int8)  # bit pair -> A2 count (01: missing)
        return synth.pack_bed_rows(geno_of_code[O.unpack_codes(rows, n_org, strict=True)[:, idx]])

    Q = qr_basis(np.random.default_rng(13).standard_normal((len(idx), 6)))
    engine.set_keep(idx, N)
    engine.load_bed_bytes(bed, len(rows), N)
    assert engine.n_org == len(idx)
    kept = engine.run(*args, pos, covar=Q)
    engine.set_keep(None)
    engine.load_bed_bytes(synth.bed_bytes(subset_rows(rows, N, idx)), len(rows), len(idx))
    sub = engine.run(*args, pos, covar=Q)
    assert np.isfinite(sub["l2"]).sum() > 1000
    assert_bitwise(kept, sub, "keep-load with Q against the subset file with Q")


# ---- 8. rejections --------------------------------------------------------------------------------------------------
def test_rejections(engine):
    from nldsc_amd._lib import NLDSCError
    name = "n1000"
    pos, args = load(engine, name)
    N, M = 1000, len(pos)
    rng = np.random.default_rng(5)
    Q = qr_basis(rng.standard_normal((N, 4)))

    def rejected(reason, covar, **kw):
        with pytest.raises(NLDSCError) as ex:
            engine.run(*args, pos, covar=covar, **kw)
        assert ex.value.code == E_ARG and reason in str(ex.value), (reason, str(ex.value))

    rejected("n_covar 0 outside [1, 64]", np.zeros((N, 0)))
    rejected("n_covar 65 outside [1, 64]", qr_basis(rng.standard_normal((N, 65))))
    bad = Q.copy()
    bad[17, 2] = np.nan
    rejected("not finite", bad)
    rejected("not orthonormal", Q * np.array([1.0, 1.0, 1.0 + 1e-6, 1.0]))
    skew = Q.copy()
    skew[:, 1] = 0.8 * Q[:, 1] + 0.6 * Q[:, 3]
    rejected("not orthonormal", skew)
    one = np.linalg.qr(np.concatenate([np.ones((N, 1)), rng.standard_normal((N, 2))], axis=1))[0]
    rejected("not centred", one)
    rejected("exact fp4 path only", Q, flags=FP32)
    rejected("exact fp4 path only", Q, flags=EXACT_I8)
    rejected("covariates with annotations", Q, annot=np.ones(M))
    ok = engine.run(*args, pos, covar=Q)  # (and the engine still runs)
    assert np.isfinite(ok["l2"]).sum() > 1000


# ---- 9. the CLI end to end ------------------------------------------------------------------------------------------
def _ld(args, expect_ok=True):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, "-m", "nldsc_amd", "ld"] + args, cwd=REPO, env=env, capture_output=True,
                       text=True, timeout=300)
    if expect_ok:
        assert p.returncode == 0 and "crashed" not in p.stderr, p.stderr[-3000:]
    return p


def test_cli_end_to_end(tmp_path, seven):
    import pandas as pd
    name = "n1001"
    C, Qe, exp = seven(name)
    ids = [line.split()[:2] for line in open(os.path.join(GOLDEN, name + ".fam")) if line.strip()]
    assert len(ids) == C.shape[0]
    order = np.random.default_rng(2).permutation(len(ids))
    lines = [f"{ids[i][0]} {ids[i][1]} " + " ".join(repr(float(x)) for x in C[i]) for i in order]
    lines.insert(400, "NOBODY NOBODY " + " ".join(["1.5"] * C.shape[1]))  # an individual the .fam lacks
    header = "FID IID " + " ".join(f"C{k}" for k in range(C.shape[1]))
    (tmp_path / "with.covar").write_text("\n".join([header] + lines) + "\n")
    (tmp_path / "without.covar").write_text("\n".join(lines) + "\n")
    common = ["--bfile", os.path.join(GOLDEN, name), "--ld-wind-cm", "1", "-maf", "0.01", "-std", "1e-5", "--extra",
              "--quiet"]
    tables = {}
    for which in ("with", "without"):
        out = tmp_path / f"{which}.L2"
        p = _ld(common + ["--covar", str(tmp_path / f"{which}.covar"), "--out", str(out)])
        assert "c = 7 columns" in p.stderr and "q = 7" in p.stderr, p.stderr[-2000:]
        tables[which] = df = pd.read_csv(out, sep="\t")
        assert len(df) == len(exp["l2"])
        for col, key in (("L2", "l2"), ("L2D", "l2d"), ("RSTD", "residuals_std")):
            g, e = df[col].to_numpy(dtype=np.float64), exp[key]
            assert np.array_equal(np.isnan(g), np.isnan(e)), (which, col)
            m = ~np.isnan(e)
            assert (np.abs(g[m] - e[m]) <= 0.5e-5 + 1e-9).all(), (which, col, np.abs(g[m] - e[m]).max())
        assert np.array_equal(df["WSA"].to_numpy(), exp["l2_ws"]) and np.array_equal(df["WSD"].to_numpy(), exp["l2d_ws"])
    assert (tmp_path / "with.L2").read_bytes() == (tmp_path / "without.L2").read_bytes()
    annot = tmp_path / "x.annot"
    annot.write_text("A\n" + "1\n" * len(exp["l2"]))
    p = _ld(common + ["--covar", str(tmp_path / "with.covar"), "--annot", str(annot), "--out", str(tmp_path / "x.L2")],
            expect_ok=False)
    # (the CLI reports a failure as the reference does: "The program crashed with ...", exit status 0)
    assert "crashed" in p.stderr and "covariates with annotations or a pair table in one run are not supported" in \
        p.stderr, (p.stderr + p.stdout)[-2000:]
    assert not (tmp_path / "x.L2").exists()
