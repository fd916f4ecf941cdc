"""Dominance-by-dominance LD scores (nldsc_engine_run_domdom, --dom-dom): L2DD_j = 1 + sum_k r2adj(R_j . R_k / N) over
the pairs WSD_j counts, for SNPs j whose own dominance residual is not constant.

Truth: explicit N-vectors in numpy.  Codes from oracle.unpack_codes(strict=True), lut_r from
oracle.stats_from_counts with missing calls 0 and R = 0 where rstd <= std_thr, G = R R^T / N, the window sets of
oracle.f64_setup, r2adj in fp64.

Bar: the project's exact-path bar |d| <= 1e-9 + 1e-12 |expected|.  A pair's error is a few ulps (the engine forms the
dot from nine exact integers and the SNPs' fp64 constants; |R_j . R_k| <= N), and a window here holds tens of
neighbours (at most ~10^3 in the golden sets), so a sum stays orders below 1e-9.  Every compared SNP's own G_jj is
asserted within 1e-12 of 1 on the truth first: the vectors the truth correlates are the standardised ones.

Runs use PLINK's sample order (the truth's)."""
import numpy as np
import pytest

from conftest import golden_sets, load_set
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")
STRICT, ADDITIVE_ONLY, EXACT_I8, FP32, EXACT_RARE = 1, 2, 4, 8, 32  # _lib.FLAG_*
E_ARG = -4
_GENO_OF_CODE = np.array([0, -1, 1, 2], np.int8)  # bit pair -> A2 count (01: missing)


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


def pack(g):
    from nldsc_amd import synth
    return synth.pack_bed_rows(np.asarray(g, np.int8))


def random_geno(M, N, seed, missing=0.02):
    """Independent SNPs with allele frequencies on both sides of 1/2 (tests/test_gpu_covar.py random_set: the same
    draws), as A2 counts with -1 for a missing call, and their positions."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.08, 0.92, M)
    g = ((rng.random((M, N)) < f[:, None]).astype(np.int8) + (rng.random((M, N)) < f[:, None]).astype(np.int8))
    g[rng.random((M, N)) < missing] = -1
    return g, np.cumsum(rng.exponential(0.05, M))


_sets: dict = {}


def dataset(name):
    """(rows, positions, run arguments (ld_wind, maf, std_thr, rsq_thr), n_org), made once."""
    if name in _sets:
        return _sets[name]
    if name == "n67":  # rows shorter than one 128-sample chunk
        g, pos = random_geno(200, 67, 67)
        out = (pack(g), pos, (1.0, 0.01, 1e-5, 1.0 / 200), 67)
    elif name == "n32773":  # N = 2^15 + 5: several K pieces, a ragged tail; 24 SNPs copy their left neighbour
        N = 2 ** 15 + 5
        g, pos = random_geno(96, N, 32773)
        rng = np.random.default_rng(5)
        rows_g, rows_p = [], []
        for j in range(96):
            rows_g.append(g[j])
            rows_p.append(pos[j])
            if j % 4 == 1:  # a copy with a tenth of its calls redrawn from another SNP of the same kind
                c = g[j].copy()
                redraw = rng.random(N) < 0.1
                c[redraw] = rng.permutation(g[j])[redraw]
                rows_g.append(c)
                rows_p.append(pos[j] + 1e-4)
        out = (pack(np.stack(rows_g)), np.asarray(rows_p), (1.0, 0.01, 1e-5, 1.0 / 120), N)
    elif name == "blockmiss":  # blocks 0 and 2 hold missing calls, blocks 1 and 3 none; one window over all
        g, pos = random_geno(128, 200, 128, missing=0.0)
        rng = np.random.default_rng(6)
        for b in (0, 2):
            blk = g[32 * b:32 * b + 32]
            blk[rng.random(blk.shape) < 0.05] = -1
        out = (pack(g), pos * 0.1, (1.0, 0.01, 1e-5, 1.0 / 128), 200)
    elif name in ("m31", "m65"):  # a ragged last block: of 31 SNPs, of one SNP
        M = int(name[1:])
        g, pos = random_geno(M, 150, M)
        out = (pack(g), pos, (1.0, 0.01, 1e-5, 1.0 / M), 150)
    else:
        bed, pos, meta, _, _ = load_set(name)
        rows = np.frombuffer(bed, np.uint8, offset=3).reshape(meta["n_snp"], -1)
        out = (rows, pos, (meta["ld_wind"], meta["maf"], meta["std_thr"], meta["rsq_thr"]), meta["n_org"])
    _sets[name] = out
    return out


def truth_of(rows, pos, args, N):
    """dict: "l2dd" (NaN where L2 is NaN — the SNP is not computed, or its window holds a SNP without an observed call —
    and where its rstd <= std_thr), "r2max" (the largest in-window r2adj),
    "gdiag" (G_jj), "replayed" (SNPs a default plain run replays in the reference's fp32 arithmetic)."""
    ld_wind, maf, std_thr, _ = args
    M = len(rows)
    codes = O.unpack_codes(rows, N, strict=True).astype(np.int64)
    cnt = np.stack([(codes == k).sum(1) for k in range(4)], 1)
    st = O.stats_from_counts(cnt, N)
    rpass = np.nan_to_num(st["rstd"], nan=0.0) > std_thr
    lr = st["lut_r"].copy()
    lr[~rpass] = 0.0
    lr[np.isnan(lr).any(axis=1)] = 0.0
    lr[:, 1] = 0.0  # missing calls
    R = np.take_along_axis(lr, codes, 1)
    G = R @ R.T / N
    s = O.f64_setup(rows, N, ld_wind, maf, std_thr, pos, strict=True)
    assert np.array_equal(s["rpass"], rpass)
    L, Rp, passed = s["L"], s["R"], s["passed"]
    n = float(N)
    adj = lambda r: 1.0 - (1.0 - r * r) * ((n - 1.0) / (n - 2.0))  # noqa: E731
    out, r2max = np.full(M, np.nan), 0.0
    allmiss = cnt[:, [0, 2, 3]].sum(1) == 0  # no observed call: A is NaN, and so is the L2 of every SNP that counts it
    for j in range(M):
        if L[j] < 0 or not rpass[j]:
            continue
        ks = np.arange(L[j], Rp[j] + 1)
        ks = ks[passed[ks] & (np.abs(pos[ks] - pos[j]) <= ld_wind) & (ks != j)]
        if allmiss[j] or allmiss[ks].any():  # L2_j is NaN (a poisoned window): so is L2DD_j
            continue
        ks = ks[rpass[ks]]
        r2 = adj(G[j, ks])
        out[j] = 1.0 + r2.sum()
        r2max = max(r2max, float(r2.max(initial=0.0)))
    obs = cnt[:, [0, 2, 3]]
    replayed = passed & (obs.sum(1) > 0) & (obs.min(1) <= 16)  # ld_kernels.h REF_RESIDUAL_MIN_CLASS
    return dict(l2dd=out, r2max=r2max, gdiag=np.diag(G).copy(), rpass=rpass, computed=L >= 0, replayed=replayed)


_truth: dict = {}


def truth(name):
    if name not in _truth:
        _truth[name] = truth_of(*dataset(name))
    return _truth[name]


def load(engine, name):
    rows, pos, args, N = dataset(name)
    from nldsc_amd import synth
    engine.set_keep(None)
    engine.load_bed_bytes(synth.bed_bytes(rows), len(rows), N)
    return pos, args


def bitwise(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_bitwise(got, exp, label, keys=KEYS):
    for k in keys:
        assert bitwise(got[k], exp[k]), \
            f"{label}: {k} differs at {np.flatnonzero(~((got[k] == exp[k]) | ((got[k] != got[k]) & (exp[k] != exp[k]))))[:10]}"


def assert_l2dd(got, t, label):
    """got["l2dd"] against the truth t: equal NaN patterns (and NaN exactly where L2 is NaN or rstd <= std_thr), every
    value within 1e-9 + 1e-12 |expected|.  Returns the worst error."""
    g, e = got["l2dd"], t["l2dd"]
    m = ~np.isnan(e)
    assert (np.abs(t["gdiag"][m] - 1.0) <= 1e-12).all(), f"{label}: the truth's own G_jj is not 1"
    assert np.array_equal(np.isnan(g), np.isnan(e)), \
        f"{label}: NaN pattern differs at {np.flatnonzero(np.isnan(g) != np.isnan(e))[:10]}"
    assert np.array_equal(np.isnan(g), np.isnan(got["l2"]) | ~t["rpass"]), f"{label}: the NaN rule"
    err = np.abs(g[m] - e[m])
    lim = 1e-9 + 1e-12 * np.abs(e[m])
    worst = float(err.max(initial=0))
    print(f"{label} l2dd: worst |d| {worst:.3g} ({int(m.sum())} values in [{np.nanmin(e):.4g}, {np.nanmax(e):.4g}], "
          f"largest in-window r2 {t['r2max']:.3g})")
    assert (err <= lim).all(), f"{label}: {int((err > lim).sum())} out of tolerance, worst {worst:.3g}"
    return worst


def run_dd(engine, name, **kw):
    pos, args = load(engine, name)
    return engine.run_domdom(*args, pos, flags=STRICT, **kw)


# ---- 1. against the truth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orient", [0, 1])
def test_n67_short_rows(engines, orient):
    t = truth("n67")
    assert int((~t["rpass"]).sum()) == 14 and t["r2max"] > 0.7  # two-class SNPs: the NaN rule and the neighbour mask
    got = run_dd(engines[orient], "n67")
    assert_l2dd(got, t, f"n67 orient={orient}")


def test_n32773_ksplit(engine):
    """Long ragged rows with near-copies (DD correlations of order 0.5); K-split factors 1 and > 1 bitwise equal."""
    t = truth("n32773")
    assert t["r2max"] > 0.2, t["r2max"]
    got = {}
    try:
        for label, opts in (("p1", {"ksplit": 0}), ("pk", {"ksplit": 1, "annot_batch_items": 16})):
            for k, v in opts.items():
                engine.set_option(k, v)
            got[label] = run_dd(engine, "n32773")
            P = engine.timings()["ksplit"]
            assert (P == 1) if label == "p1" else (P > 1), f"{label}: K-split factor {P}"
            assert_l2dd(got[label], t, f"n32773 {label} (K-split {P})")
    finally:
        engine.set_option("ksplit", 1)
        engine.set_option("annot_batch_items", 0)
    assert_bitwise(got["pk"], got["p1"], "n32773 K-split > 1 vs 1", KEYS + ("l2dd",))


def test_block_missing_combinations(engines):
    """Blocks with and without missing calls in one window: all four RM / CM kernels and both kinds of diagonal item
    (a wrong h x h block scale shows here)."""
    rows, pos, args, N = dataset("blockmiss")
    codes = O.unpack_codes(rows, N, strict=True)
    miss = (codes == 1).reshape(4, 32, -1).any(axis=(1, 2))
    assert list(miss) == [True, False, True, False]
    assert pos[-1] - pos[0] <= args[0]  # every block pair is needed
    t = truth("blockmiss")
    for orient, e in engines.items():
        assert_l2dd(run_dd(e, "blockmiss"), t, f"blockmiss orient={orient}")


@pytest.mark.parametrize("name", ["m31", "m65"])
def test_ragged_snp_counts(engine, name):
    assert_l2dd(run_dd(engine, name), truth(name), name)


@pytest.mark.parametrize("name", sorted(golden_sets()))
def test_golden_sets(engine, name):
    """L2DD against the truth; the seven ordinary arrays bitwise a plain EXACT_RARE run's, and a default plain run's
    where no SNP is replayed."""
    t = truth(name)
    pos, args = load(engine, name)
    got = engine.run_domdom(*args, pos, flags=STRICT)
    assert_l2dd(got, t, name)
    assert_bitwise(got, engine.run(*args, pos, flags=STRICT | EXACT_RARE), f"{name} vs plain EXACT_RARE")
    if not t["replayed"].any():
        assert_bitwise(got, engine.run(*args, pos, flags=STRICT), f"{name} vs default plain")
    print(f"{name}: {int(t['replayed'].sum())} replayed SNPs")


def test_no_replayed_snp_equals_default_plain(engine):
    """Common variants only (every genotype class above the replay's 16 calls): the default plain run's arrays."""
    assert not truth("n32773")["replayed"].any()
    pos, args = load(engine, "n32773")
    got = engine.run_domdom(*args, pos, flags=STRICT)
    assert_bitwise(got, engine.run(*args, pos, flags=STRICT), "n32773 vs default plain")


# ---- 2. schedule independence ----------------------------------------------------------------------------------------
def test_owned_ranges(engine):
    pos, args = load(engine, "n1001")
    M = len(pos)
    whole = engine.run_domdom(*args, pos, flags=STRICT)
    lo = engine.run_domdom(*args, pos, flags=STRICT, own=(0, M // 2))
    hi = engine.run_domdom(*args, pos, flags=STRICT, own=(M // 2, M))
    for k in KEYS + ("l2dd",):
        joined = np.concatenate([lo[k][:M // 2], hi[k][M // 2:]])
        assert bitwise(joined, whole[k]), f"owned halves: {k}"
    assert np.isnan(lo["l2dd"][M // 2:]).all() and np.isnan(hi["l2dd"][:M // 2]).all()


def test_keep_list(engine):
    """A run under set_keep equals the run on the compacted file."""
    from nldsc_amd import synth
    rows, pos, args, N = dataset("n1003")
    M = len(rows)
    idx = np.sort(np.random.default_rng(12).choice(N, 601, replace=False)).astype(np.int32)
    engine.set_keep(idx, N)
    engine.load_bed_bytes(synth.bed_bytes(rows), M, N)
    assert engine.n_org == len(idx)
    kept = engine.run_domdom(*args, pos)
    engine.set_keep(None)
    sub = pack(_GENO_OF_CODE[O.unpack_codes(rows, N, strict=True)[:, idx]])
    engine.load_bed_bytes(synth.bed_bytes(sub), M, len(idx))
    plain = engine.run_domdom(*args, pos, flags=STRICT)
    assert_bitwise(kept, plain, "keep list vs compacted file", KEYS + ("l2dd",))
    assert_l2dd(plain, truth_of(sub, pos, args, len(idx)), "n1003 kept 601")


def test_engine_state(engine):
    """A plain run, a dom-dom run, a plain run on one engine: the two plain results are bitwise equal."""
    pos, args = load(engine, "n1000")
    a = engine.run(*args, pos)
    engine.run_domdom(*args, pos)
    b = engine.run(*args, pos)
    assert_bitwise(a, b, "plain runs around a dom-dom run")


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def refused(fn, *needles):
    from nldsc_amd._lib import NLDSCError
    with pytest.raises(NLDSCError) as ei:
        fn()
    assert ei.value.code == E_ARG, ei.value
    for n in needles:
        assert n in str(ei.value), (n, str(ei.value))


def test_refusals(engine):
    from nldsc_amd.engine import Engine
    pos, args = load(engine, "n67")
    M, N = len(pos), 67
    refused(lambda: engine.run_domdom(*args, pos, flags=FP32), "exact fp4 path only", "fp32")
    refused(lambda: engine.run_domdom(*args, pos, flags=EXACT_I8), "exact fp4 path only", "int8")
    refused(lambda: engine.run_domdom(*args, pos, flags=ADDITIVE_ONLY), "NLDSC_FLAG_ADDITIVE_ONLY")
    for kw in (dict(annot=np.ones((M, 1))), dict(covar=np.ones((N, 1))), dict(pairs=True)):
        refused(lambda kw=kw: engine.run_domdom(*args, pos, **kw), "annotations, a pair table or covariates")
    # n_org >= 2^19: refused on the parameters, before they are held against the loaded image
    big = Engine(0)
    try:
        big.n_snp, big.n_org = M, 1 << 19
        refused(lambda: big.run_domdom(*args, pos), "n_org < 2^19", "unsegmented rows")
    finally:
        big.close()
    got = engine.run_domdom(*args, pos, flags=STRICT)  # the engine still runs
    assert_l2dd(got, truth("n67"), "n67 after the refusals")
