"""The pairwise LD table (nldsc_engine_run_pairs, --pairs-out): for every owned computed SNP j one entry (k, r, rd) per
neighbour k the run counts in l2_ws[j], CSR over the owned range, rows sorted by k.

Truth: oracle.pair_r2_f64 (integer contingency tables, binary64 per pair) for the neighbour sets and the r2adj values,
and the signed correlations la[j] . C . la[k] / N, la[j] . C . lr[k] / N restated here from O.f64_setup and
O.code_tables.  The bound is the project's exact-path bar (1e-9, 1e-12) of tests/test_gpu_parity.py, per term:
|got - exp| <= 1e-9 + 1e-12 |exp|.  Everything else (row lengths, counts, the filter, owned ranges, invariance across
schedules) is exact."""
import ctypes

import numpy as np
import pytest

from conftest import record
from oracle import oracle as O
from test_gpu_annot import SETS, bitwise, dataset, load, assert_plain_bitwise

pytestmark = pytest.mark.gpu

ADDITIVE_ONLY, EXACT_I8, FP32, EXACT_RARE = 2, 4, 8, 32  # _lib.FLAG_*
ABS, REL = 1e-9, 1e-12
TABLE = ("row_ptr", "k", "r", "rd")


@pytest.fixture(scope="module")
def engine():
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)
    from nldsc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def r2adj(c, n):
    from nldsc_amd.ldscore.common import r2_adjusted
    return r2_adjusted(c, n)


def rows_of(t, j0=0):
    """entry -> its SNP j (row j - j0 of the table)"""
    return j0 + np.repeat(np.arange(len(t["row_ptr"]) - 1), np.diff(t["row_ptr"]))


def same_table(a, b):
    return all(bitwise(a[k], b[k]) for k in TABLE)


def within(got, exp):
    """worst |got - exp| in units of the bar 1e-9 + 1e-12 |exp| (equal NaN patterns asserted)"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    m = ~np.isnan(exp)
    return float((np.abs(got[m] - exp[m]) / (ABS + REL * np.abs(exp[m]))).max(initial=0))


def signed_truth(rows, N, args, pos, bed=None, targets=None, strict=False):
    """Per target (None: every SNP) None or (ks, r, r2a, kd mask over ks, rd at kd, r2d): oracle._f64_pairs with
    the signed correlations kept, plus O.pair_r2_f64 itself for ks / kds / the r2adj values."""
    s = O.f64_setup(rows, N, args[0], args[1], args[2], pos, strict=strict, bed=bed)
    targets = np.arange(len(rows)) if targets is None else np.asarray(targets)
    la, lr = s["st"]["lut_a"], s["st"]["lut_r"]
    out = []
    for j, p in zip(targets, O.pair_r2_f64(rows, N, args[0], args[1], args[2], pos, targets, strict=strict, setup=s)):
        if p is None:
            out.append(None)
            continue
        ks, r2a, kds, r2d = p
        kd = np.isin(ks, kds)
        C = O.code_tables(s["bed"], s["M"], N, int(j), ks, strict).astype(np.float64)
        r = np.einsum("g,kgh,kh->k", la[j], C, la[ks]) / float(N)
        rd = np.einsum("g,kgh,kh->k", la[j], C[kd], lr[ks[kd]]) / float(N)
        out.append((ks, r, np.asarray(r2a), kd, rd, np.asarray(r2d)))
    return out


@pytest.fixture(scope="module")
def truth_n1001():
    rows, pos, args, N, bed = dataset("n1001")
    return signed_truth(rows, N, args, pos, bed=bed)


def check_rows(t, truth, N, targets, j0=0, dom=True):
    """Rows of the targets against the truth: ks exact and in order, rd non-NaN exactly on kds, values within the
    bar.  Returns the worst errors in units of the bar."""
    worst = dict(r=0.0, rd=0.0, r2=0.0, r2d=0.0)
    rp = t["row_ptr"]
    for j, p in zip(targets, truth):
        a, b = rp[j - j0], rp[j - j0 + 1]
        if p is None:
            assert a == b, f"SNP {j} is not computed but has a row"
            continue
        ks, r, r2a, kd, rd, r2d = p
        assert np.array_equal(t["k"][a:b], ks), f"SNP {j}: neighbours"
        worst["r"] = max(worst["r"], within(t["r"][a:b], r))
        worst["r2"] = max(worst["r2"], within(r2adj(t["r"][a:b], N), r2a))
        if dom:
            assert np.array_equal(~np.isnan(t["rd"][a:b]), kd), f"SNP {j}: rd's NaN pattern"
            worst["rd"] = max(worst["rd"], within(t["rd"][a:b][kd], rd))
            worst["r2d"] = max(worst["r2d"], within(r2adj(t["rd"][a:b][kd], N), r2d))
        else:
            assert np.isnan(t["rd"][a:b]).all()
    return worst


def test_truth(engine, truth_n1001):
    """1. n1001, FLAG_EXACT_RARE, no filter: every row against the fp64 truth; the same additive-only (rd all NaN)."""
    rows, pos0, args, N, _ = dataset("n1001")
    pos, args = load(engine, "n1001")
    M = len(rows)
    t = engine.run_pairs(*args, pos, flags=EXACT_RARE)
    assert sum(p is not None for p in truth_n1001) > 1000
    w = check_rows(t, truth_n1001, N, np.arange(M))
    print("n1001 worst errors in units of the bar:", w)
    add = engine.run_pairs(*args, pos, flags=EXACT_RARE | ADDITIVE_ONLY)
    wa = check_rows(add, truth_n1001, N, np.arange(M), dom=False)
    assert np.isnan(add["rd"]).all() and len(add["rd"]) == len(t["rd"])
    record("pairs_truth_n1001", dict(dominance_run=w, additive_only=wa, pairs=int(t["n_pairs"])))
    assert max(w.values()) <= 1.0 and max(wa.values()) <= 1.0, (w, wa)


@pytest.fixture(scope="module")
def plain_and_pairs(engine):
    out = {}

    def get(name):
        if name not in out:
            pos, args = load(engine, name)
            out[name] = (engine.run(*args, pos), engine.run_pairs(*args, pos))
        return out[name]
    return get


@pytest.mark.parametrize("name", SETS)
def test_decomposition(plain_and_pairs, name):
    """2. + 3. default flags (rare1003 takes the KC path): the table decomposes the run's own sums and counts, and the
    seven ordinary arrays are bitwise a plain run's."""
    plain, t = plain_and_pairs(name)
    rows, pos, args, N, _ = dataset(name)
    assert_plain_bitwise(t, plain, name)
    M = len(rows)
    computed = plain["l2_ws"] >= 0
    lens = np.diff(t["row_ptr"])
    assert len(lens) == M and t["n_pairs"] == t["row_ptr"][-1] == len(t["k"])
    assert np.array_equal(lens[computed], plain["l2_ws"][computed]) and not lens[~computed].any()
    j = rows_of(t)
    has_rd = ~np.isnan(t["rd"])
    n_rd = np.bincount(j[has_rd], minlength=M)
    # An all-missing SNP's own row is the one place where a NaN rd is a value, not an absence: its A is NaN, so is
    # every rd of its row, and the run still counts those pairs in l2d_ws (its l2 and l2d are NaN).  Such a row has
    # no finite r at all; every other computed row is held to the exact count.
    own_nan = computed & (lens > 0) & (np.bincount(j[np.isfinite(t["r"])], minlength=M) == 0)
    assert np.isnan(plain["l2"][own_nan]).all() and np.isnan(plain["l2d"][own_nan]).all() and not n_rd[own_nan].any()
    assert (name == "allmiss") == bool(own_nan.any())
    held = computed & ~own_nan
    assert np.array_equal(n_rd[held], plain["l2d_ws"][held])
    r2, r2d = r2adj(t["r"], N), r2adj(t["rd"], N)
    with np.errstate(invalid="ignore"):
        over = has_rd & (r2d > args[3])
    assert np.array_equal(np.bincount(j[over], minlength=M)[computed], plain["l2d_wse"][computed])
    s2 = 1.0 + np.bincount(j, weights=r2, minlength=M)
    sd = np.bincount(j[has_rd], weights=r2d[has_rd], minlength=M)
    bad = np.bincount(j[~np.isfinite(t["r"])], minlength=M) > 0
    assert np.array_equal(bad[computed], np.isnan(plain["l2"][computed])), "non-finite r exactly where l2 is NaN"
    if name == "allmiss":  # (allmiss_pad's committed results hold no NaN l2)
        assert bad.sum() > 100
    ok = computed & ~bad
    w2 = within(s2[ok], plain["l2"][ok])
    okd = computed & ~np.isnan(plain["l2d"]) & np.isfinite(sd)
    wd = within(sd[okd], plain["l2d"][okd])
    print(f"{name}: sums against the run's l2 / l2d, worst in units of the bar: {w2:.3g} / {wd:.3g}")
    assert w2 <= 1.0 and wd <= 1.0
    for a, b in zip(t["row_ptr"][:-1], t["row_ptr"][1:]):
        assert (np.diff(t["k"][a:b]) > 0).all()


@pytest.mark.parametrize("name", ["n1001", "rare1003"])
def test_symmetry(plain_and_pairs, name):
    """4. wherever both (j, k) and (k, j) are present, their r are bitwise equal."""
    _, t = plain_and_pairs(name)
    M = len(t["row_ptr"]) - 1
    j, k = rows_of(t).astype(np.int64), t["k"].astype(np.int64)
    key, rev = j * M + k, k * M + j  # (key is ascending: rows in order, k ascending within a row)
    at = np.searchsorted(key, rev)
    both = (at < len(key)) & (key[np.minimum(at, len(key) - 1)] == rev)
    assert both.sum() > 1000
    assert np.array_equal(t["r"][both].view(np.int64), t["r"][at[both]].view(np.int64))


OPTION_SETS = [dict(pairs_batch_items=7), dict(pairs_batch_items=1), dict(ksplit=0), dict(gpu_plan=0),
               dict(plan_fused=0), dict(t2=0), dict(t2=2, pairs_batch_items=7)]
DEFAULTS = dict(pairs_batch_items=0, ksplit=1, gpu_plan=1, plan_fused=1, t2=3)


@pytest.mark.parametrize("name", ["n1001", "rare1003"])
def test_invariance(engine, plain_and_pairs, name):
    """5. the table is bitwise the same across batch sizes, schedules and repeated runs."""
    _, base = plain_and_pairs(name)
    pos, args = load(engine, name)
    assert same_table(engine.run_pairs(*args, pos), base), "repeated run"
    try:
        for opts in OPTION_SETS:
            for k, v in {**DEFAULTS, **opts}.items():
                engine.set_option(k, v)
            t = engine.run_pairs(*args, pos)
            assert same_table(t, base), f"options {opts}"
            assert_plain_bitwise(t, base, f"{name} {opts}")
    finally:
        for k, v in DEFAULTS.items():
            engine.set_option(k, v)


def test_owned_ranges(engine, plain_and_pairs):
    """6. owned ranges equal the matching slices of the full table; three ranges tiling [0, M) concatenate to it."""
    _, full = plain_and_pairs("n1002")
    pos, args = load(engine, "n1002")
    M = len(pos)

    def slice_of(lo, hi):
        a, b = full["row_ptr"][lo], full["row_ptr"][hi]
        return dict(row_ptr=full["row_ptr"][lo:hi + 1] - a, k=full["k"][a:b], r=full["r"][a:b], rd=full["rd"][a:b])

    for own in [(0, 1), (M - 1, M), (M // 3 + 5, 2 * M // 3 - 7), (77, 77)]:
        t = engine.run_pairs(*args, pos, own=own)
        assert same_table(t, slice_of(*own)), f"own {own}"
        for key in ("l2", "l2d", "l2_ws"):
            assert bitwise(t[key][own[0]:own[1]], full[key][own[0]:own[1]])
    cuts = [0, 411, 800, M]
    parts = [engine.run_pairs(*args, pos, own=(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    for key in ("k", "r", "rd"):
        assert bitwise(np.concatenate([p[key] for p in parts]), full[key])
    ptr = np.concatenate([[0]] + [p["row_ptr"][1:] + off for p, off in
                                  zip(parts, np.cumsum([0] + [p["n_pairs"] for p in parts[:-1]]))])
    assert np.array_equal(ptr, full["row_ptr"])


def raw_call(engine, args, pos, own, cap, with_arrays=True, flags=0, min_r2=float("nan")):
    """nldsc_engine_run_pairs itself: (return code, message, n_pairs, row_ptr, k, r, rd, result arrays)"""
    from nldsc_amd import _lib
    n = engine.n_snp
    p, _keep = _lib.make_params(n, engine.n_org, args[0], args[1], args[2], args[3], pos, flags=flags)
    arrs, res = _lib.alloc_result(n)
    row_ptr = np.full(own[1] - own[0] + 1, -7, np.int64)
    m = max(cap, 1)
    k, r, rd = np.full(m, -7, np.int32), np.full(m, -7.0), np.full(m, -7.0)
    n_pairs = ctypes.c_int64(-7)
    err = _lib.errbuf()
    rc = engine._L.nldsc_engine_run_pairs(
        engine._h, ctypes.byref(p), own[0], own[1], ctypes.byref(res), min_r2, row_ptr.ctypes.data,
        k.ctypes.data if with_arrays else None, r.ctypes.data if with_arrays else None,
        rd.ctypes.data if with_arrays else None, cap, ctypes.byref(n_pairs), err, len(err))
    return rc, err.value.decode(), int(n_pairs.value), row_ptr, k, r, rd, arrs


def test_sizing(engine, plain_and_pairs):
    """7. cap 0 and cap n_pairs - 1 give NLDSC_E_SPACE with n_pairs and row_ptr filled; cap n_pairs succeeds."""
    from nldsc_amd import _lib
    plain, full = plain_and_pairs("n1003")
    pos, args = load(engine, "n1003")
    M = len(pos)
    own = (M // 3 + 5, 2 * M // 3 - 7)
    ws = plain["l2_ws"][own[0]:own[1]]
    need = int(ws[ws > 0].sum())
    ptr = full["row_ptr"][own[0]:own[1] + 1] - full["row_ptr"][own[0]]
    for cap, arrays in ((0, True), (need - 1, True), (need, False)):
        rc, msg, n_pairs, row_ptr, k, r, rd, arrs = raw_call(engine, args, pos, own, cap, arrays)
        assert rc == _lib.E_SPACE and str(need) in msg, (rc, msg)
        assert n_pairs == need and np.array_equal(row_ptr, ptr)
        assert (k == -7).all() and (r == -7.0).all() and (rd == -7.0).all(), "nothing is emitted"
        assert bitwise(arrs["l2"][own[0]:own[1]], plain["l2"][own[0]:own[1]])  # (documented: `r` is written)
    rc, msg, n_pairs, row_ptr, k, r, rd, _ = raw_call(engine, args, pos, own, need)
    assert rc == 0 and n_pairs == need and np.array_equal(row_ptr, ptr)
    a = full["row_ptr"][own[0]]
    assert bitwise(k, full["k"][a:a + need]) and bitwise(r, full["r"][a:a + need]) and bitwise(rd, full["rd"][a:a + need])
    s = engine.size_pairs(*args, pos, own=own)
    assert s["n_pairs"] == need and np.array_equal(s["row_ptr"], ptr)


def clear_threshold(values, lo=0.04, hi=0.06, gap=1e-6, centre=0.05):
    """The value in [lo, hi] nearest `centre` that is clear by more than `gap` of every one of `values` (None: none):
    a midpoint between two neighbours more than 2 gap apart, or a point gap-and-a-bit inside the interval's ends."""
    v = np.sort(values[(values > lo - 2 * gap) & (values < hi + 2 * gap)])
    v = np.concatenate([[lo - 2 * gap], v, [hi + 2 * gap]])
    wide = np.flatnonzero(np.diff(v) > 2.5 * gap)
    cand = [float(np.clip(centre, v[i] + 1.25 * gap, v[i + 1] - 1.25 * gap)) for i in wide]
    cand = [c for c in cand if lo <= c <= hi]
    return min(cand, key=lambda c: abs(c - centre)) if cand else None


def filtered_truth(truth, thr):
    """signed_truth's rows with the entries whose exact r2adj(r) or r2adj(rd) exceeds thr."""
    kept = []
    for p in truth:
        if p is None:
            kept.append(None)
            continue
        ks, r, r2a, kd, rd, r2d = p
        d_over = np.zeros(len(ks), bool)
        d_over[kd] = r2d > thr
        m = (r2a > thr) | d_over
        kept.append((ks[m], r[m], r2a[m], kd[m], rd[m[kd]], r2d[m[kd]]))
    return kept


def test_filter(engine, truth_n1001):
    """8. min_r2 near 0.05, clear by 1e-6 of every pair's exact values: the filtered table is the truth's filtered
    pair set exactly, values within the bar."""
    rows, _, _, N, _ = dataset("n1001")
    allv = np.concatenate([np.concatenate([p[2], p[5]]) for p in truth_n1001 if p is not None])
    thr = clear_threshold(allv)
    assert thr is not None and 0.04 <= thr <= 0.06
    assert np.abs(allv[np.isfinite(allv)] - thr).min() >= 1e-6
    pos, args = load(engine, "n1001")
    t = engine.run_pairs(*args, pos, flags=EXACT_RARE, min_r2=thr)
    kept = filtered_truth(truth_n1001, thr)
    n_kept = sum(len(p[0]) for p in kept if p is not None)
    assert 0 < n_kept < len(allv) and t["n_pairs"] == n_kept
    w = check_rows(t, kept, N, np.arange(len(rows)))
    print(f"min_r2 {thr!r}: {n_kept} pairs kept, worst errors in units of the bar {w}")
    assert max(w.values()) <= 1.0


# ---- geometry beyond the fixtures: short rows (N = 67), as tests/test_gpu_schedule_scale.py ----
N67, MAF67, STD67, RSQ67 = 67, 0.05, 1e-5, 0.01


def short_rows(M, seed):
    from nldsc_amd import synth
    from test_gpu_schedule_scale import fast_genotypes
    geno = fast_genotypes(M, N67, seed=seed, missing=0.02)
    assert all((geno[b:b + 32] < 0).any() for b in range(0, M, 32)), "missing calls in every block"
    rows = synth.pack_bed_rows(geno)
    return rows, synth.bed_bytes(rows)


def full_window_set():
    """(M, rows, bed bytes, positions, arguments): M = 32 * 9 + 1 short rows and a window as long as the chromosome."""
    M = 32 * 9 + 1
    rows, bed = short_rows(M, 501)
    pos = np.cumsum(np.random.default_rng(5).integers(0, 600, size=M)).astype(np.float64)
    return M, rows, bed, pos, (float(pos[-1]), MAF67, STD67, RSQ67)


def test_full_window(engine):
    """9a. M = 32 * 9 + 1 and a window as long as the chromosome: every block pair is an item, the last block holds
    one SNP, and row j is exactly the passed SNPs other than j."""
    M, rows, bed, pos, args = full_window_set()
    engine.set_keep(None)
    engine.load_bed_bytes(bed, M, N67)
    t = engine.run_pairs(*args, pos, flags=EXACT_RARE)
    passed = O.f64_setup(rows, N67, *args[:3], pos, bed=bed)["passed"]
    assert 200 < passed.sum() < M and passed[M - 1]
    for j in range(M):
        exp = np.flatnonzero(passed & (np.arange(M) != j)) if passed[j] else np.zeros(0, np.int64)
        assert np.array_equal(t["k"][t["row_ptr"][j]:t["row_ptr"][j + 1]], exp), f"row {j}"
    assert_plain_bitwise(t, engine.run(*args, pos, flags=EXACT_RARE), "full window")


def ragged_set():
    """(M, rows, bed bytes, positions, arguments, the run of SNPs at one position, the exact window ties): ~3 000
    ragged positions, 230 SNPs at one position, a gap beyond the window, exact window ties."""
    M, w = 3001, 3000.0
    rng = np.random.default_rng(77)
    gaps = np.round(rng.exponential(30.0, size=M))
    gaps[32 * 40] = 3 * w
    pos = np.cumsum(gaps)
    run = (1000 - 40, 1000 + 190)
    pos[run[0]:run[1]] = pos[run[0]]
    ties = []
    for a in (100, 2000, 2700):
        b = int(np.searchsorted(pos, pos[a] + w, side="left"))
        assert b < M and pos[b] - pos[a] < 2 * w
        pos[b] = pos[a] + w
        ties.append((a, b))
    assert (np.diff(pos) >= 0).all()
    rows, bed = short_rows(M, 502)
    args = (w, MAF67, STD67, RSQ67)
    return M, rows, bed, pos, args, run, ties


def ragged_targets(M, run, ties):
    """~60 targets: block edges, the tie run, the exact window ties, the ends, 30 random SNPs."""
    tg = {0, 1, 31, 32, 33, M - 1, M - 2, 32 * 40 - 1, 32 * 40, 32 * 40 + 1, run[0] - 1, run[0], (run[0] + run[1]) // 2,
          run[1] - 1, run[1], 32 * 93, 32 * 93 + 31, 959, 991, 992, 1023, 1024}
    tg |= {x for ab in ties for x in ab} | {x + d for ab in ties for x in ab for d in (-1, 1)}
    tg |= set(np.random.default_rng(M).choice(M, 30, replace=False).tolist())
    tg = np.array(sorted(x for x in tg if 0 <= x < M))
    return tg


def test_ragged(engine):
    """9b. ~3 000 ragged positions: 230 SNPs at one position, a gap beyond the window, exact window ties.  Row lengths
    equal the run's l2_ws; the rows of ~60 targets (block edges, the tie run, the ends) equal the truth's."""
    M, rows, bed, pos, args, run, ties = ragged_set()
    engine.set_keep(None)
    engine.load_bed_bytes(bed, M, N67)
    # (FLAG_EXACT_RARE: at N = 67 nearly every SNP is a rare variant, and the truth is the exact restatement)
    t = engine.run_pairs(*args, pos, flags=EXACT_RARE)
    plain = engine.run(*args, pos, flags=EXACT_RARE)
    assert_plain_bitwise(t, plain, "ragged")
    computed = plain["l2_ws"] >= 0
    lens = np.diff(t["row_ptr"])
    assert np.array_equal(lens[computed], plain["l2_ws"][computed]) and not lens[~computed].any()
    tg = ragged_targets(M, run, ties)
    assert len(tg) >= 55
    truth = signed_truth(rows, N67, args, pos, bed=bed, targets=tg)
    assert sum(p is not None for p in truth) >= 40
    wst = check_rows(t, truth, N67, tg)
    print("ragged: worst errors in units of the bar", wst)
    assert max(wst.values()) <= 1.0


def test_rejections(engine):
    """10. NLDSC_E_ARG with its reason: the fp32 flag, the int8 flag, a count matrix beyond the cap, annotations are
    a different entry point; n_org >= 2^19 on a tiny M."""
    from nldsc_amd import _lib
    pos, args = load(engine, "n1000")
    M = len(pos)
    for flags, word in ((FP32, "fp32"), (EXACT_I8, "int8")):
        rc, msg, *_ = raw_call(engine, args, pos, (0, M), 0, flags=flags)
        assert rc == _lib.E_ARG and "exact fp4 path only" in msg and word in msg, (rc, msg)
    engine.set_option("pairs_max_cells", 64)
    try:
        rc, msg, *_ = raw_call(engine, args, pos, (0, M), 0)
        assert rc == _lib.E_ARG and "narrow the owned range" in msg, (rc, msg)
        t = engine.run_pairs(*args, pos, own=(5, 6))  # (one SNP's row always fits 64 cells here)
        assert t["n_pairs"] == np.diff(t["row_ptr"])[0]
    finally:
        engine.set_option("pairs_max_cells", 0)
    with pytest.raises(_lib.NLDSCError) as ei:
        engine.run_pairs(*args, pos, flags=FP32)
    assert ei.value.code == _lib.E_ARG
    # 2^19 individuals, 33 SNPs (4.3 MB of rows): rejected before any kernel of the band runs
    Mb, Nb = 33, 1 << 19
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 256, size=(Mb, Nb // 4), dtype=np.uint8)
    engine.load_bed_bytes(b"\x6c\x1b\x01" + rows.tobytes(), Mb, Nb)
    rc, msg, *_ = raw_call(engine, (1.0, 0.0, 1e-5, 0.01), np.arange(Mb, dtype=np.float64) / Mb, (0, Mb), 0)
    assert rc == _lib.E_ARG and "n_org < 2^19" in msg, (rc, msg)


@pytest.mark.parametrize("keep", [False, True])
def test_estimate_lds_pairs_out(engine, plain_and_pairs, tmp_path, monkeypatch, keep):
    """--pairs-out end to end on n1003: the .L2 bytes are those of a run without it; the table (gzip, a budget that
    cuts the chromosome into several owned ranges, sizing calls of 500 SNPs) holds the engine's pairs, row for row;
    with --keep both go through the kept individuals."""
    import gzip
    import os
    import pandas as pd
    from conftest import GOLDEN
    from nldsc_amd.ldscore import routine
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rows, pos, args, N, _ = dataset("n1003")
    kw = dict(ld_wind=args[0] / 1000.0, wind_metric="kbp", maf_thr=args[1], std_thr=args[2], rsq_thr=args[3], extra=True,
              summary=False, progress=False)
    if keep:
        fam = pd.read_csv(os.path.join(GOLDEN, "n1003.fam"), sep=r"\s+", header=None, dtype=str)
        (tmp_path / "keep.txt").write_text("".join(f"{a} {b}\n" for a, b in zip(fam[0][::2], fam[1][::2])))
        kw["keep"] = str(tmp_path / "keep.txt")
    bfile = os.path.join(GOLDEN, "n1003")
    routine.estimate_lds(bfile, out=str(tmp_path / "a.L2"), **kw)
    real = routine.run_pairs_to_file
    monkeypatch.setattr("nldsc_amd.ldscore.genome.run_pairs_to_file",
                        lambda *a, **k: real(*a, **{**k, "size_snps": 500}))
    routine.estimate_lds(bfile, out=str(tmp_path / "b.L2"), pairs_out=str(tmp_path / "p.tsv.gz"), pairs_budget=20_000,
                         **kw)
    assert (tmp_path / "a.L2").read_bytes() == (tmp_path / "b.L2").read_bytes()
    df = pd.read_csv(gzip.open(tmp_path / "p.tsv.gz", "rt"), sep="\t")
    l2 = pd.read_csv(tmp_path / "b.L2", sep="\t")
    wsa = l2["WSA"].to_numpy()
    assert len(df) == wsa[wsa > 0].sum() > 20_000
    snp = l2["SNP"].to_numpy()
    index = {s: i for i, s in enumerate(snp)}
    ja, kb = df["SNP_A"].map(index).to_numpy(), df["SNP_B"].map(index).to_numpy()
    assert (np.diff(ja) >= 0).all() and np.array_equal(np.bincount(ja, minlength=len(snp))[wsa > 0], wsa[wsa > 0])
    assert ((np.diff(kb) > 0) | (np.diff(ja) > 0)).all()
    if not keep:
        _, t = plain_and_pairs("n1003")
        assert np.array_equal(kb, t["k"]) and np.allclose(df["R"], t["r"], atol=5.1e-7, rtol=0)
        assert np.array_equal(df["RD"].isna(), np.isnan(t["rd"]))
        assert np.allclose(df["R2"], r2adj(t["r"], N), atol=5.1e-7, rtol=0)
