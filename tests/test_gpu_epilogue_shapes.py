"""The pairs and the annotated K-split epilogues (band_f4_epi_pairs_kernel, band_f4_epi_annot_kernel) where
tests/test_gpu_pairs.py and tests/test_gpu_annot.py never take them: rows the band splits into K pieces (P > 1), rows
up to the admitted 2^19 - 1 samples, missing-free blocks beside blocks with missing calls, rows of both stored
orientations in one window, an engine that stores the file's orientation (orient 0: pa.flip == nullptr), replayed
rare variants under the default flags (the KC instantiations and their sign rule), and windows of hundreds of items
behind one SNP's annotation accumulators.

Truth and bars are the neighbouring modules': test_gpu_pairs.signed_truth / check_rows (1e-9 + 1e-12 |expected| per
value, neighbour sets and NaN patterns exact) and test_gpu_annot.truth / assert_truth (1e-9 max(1, |a_c|max) +
1e-12 |expected| per annotation column).  Every run here uses the reference's sample order (flags without
STRICT_PLINK_ORDER, as the CLI), so at N % 4 != 0 the truth and the engine both read the padding pair of the last
byte.  Every truth case asserts that the seven ordinary arrays are bitwise a plain run's.

Replayed rare variants (test_replayed_signs): the engine's values for an entry with a replayed SNP are the
reference's fp32 vectors', not the closed form's, so they are held (a) in sign to the exact truth wherever the exact
|r| (|rd|) is at least 1e-3 - three orders above any fp32 rounding of a standardised vector at these N - and (b) in
magnitude to the C oracle run on the two-row file of the pair (l2[0] - 1 and l2d[0] are the pair's r2adj in the
reference's arithmetic) within conftest.TOL["l2d"], 3e-6 + 1e-4 |x|, the bar the project applies to sums of such
terms; the oracle's own distance from the exact truth on the same sample is measured first and, should it exceed
that bar, twice that distance is the bar instead.
"""
import time

import numpy as np
import pytest

from conftest import TOL, record
from oracle import oracle as O
from test_gpu_annot import assert_truth, six_columns
from test_gpu_annot import truth as annot_truth
from test_gpu_covar import assert_bitwise, bitwise, dataset, engines, forget_set, load, register_set  # noqa: F401
from test_gpu_covar_shapes import CAP_N, cap_rows, registered
from test_gpu_pairs import (ABS, ADDITIVE_ONLY, EXACT_RARE, N67, REL, check_rows, clear_threshold, filtered_truth,
                            full_window_set, r2adj, ragged_set, ragged_targets, rows_of, same_table, signed_truth)
from test_gpu_parity import missing_free_blocks

pytestmark = pytest.mark.gpu

E_ARG = -4
ANNOT_KEYS = ("l2_annot", "l2d_annot")
REPLAY_MAX_CLASS = 16  # ld_kernels.h REF_RESIDUAL_MIN_CLASS
SIGN_MARGIN = 1e-3


# ---- data sets ------------------------------------------------------------------------------------------------------
def ld_set():
    """N = 32 773, M = 96 of the project's LD model (rho = 0.9, 1 % missing), every pair inside the window: exact
    r2adj up to 0.5."""
    from nldsc_amd import synth
    M, N = 96, 32773
    rows = synth.pack_bed_rows(synth.genotypes(synth.SynthSpec(n_org=N, n_snp=M, rho=0.9, missing=0.01)))
    return rows, 0.01 * np.arange(M), (1.0, 0.01, 1e-5, 1.0 / M), N


def mixed_rare(N, M=128, seed=5):
    """conftest.rare_variant_set with orientation crossed against rarity: even j rare (MAF log-uniform in 3/N ..
    60/N), odd j common (MAF uniform in 0.05 .. 0.5); A1 the minor allele for j % 4 < 2; 1 % missing calls; positions
    cumulative Exp(0.05)."""
    from nldsc_amd import synth
    rng = np.random.default_rng(seed)
    maf = np.where(np.arange(M) % 2 == 0, 10 ** rng.uniform(np.log10(3.0 / N), np.log10(60.0 / N), M),
                   rng.uniform(0.05, 0.5, M))
    g = np.empty((M, N), np.int8)
    for j in range(M):
        a = (rng.random(N) < maf[j]).astype(np.int8) + (rng.random(N) < maf[j]).astype(np.int8)
        if j % 4 < 2:
            a = 2 - a  # minor allele = A1
        a[rng.random(N) < 0.01] = -1
        g[j] = a
    return synth.pack_bed_rows(g), np.cumsum(rng.exponential(0.05, M))


def named(name):
    """test_gpu_covar.dataset for this module's sets too: (rows, positions, arguments, n_org, bed bytes)."""
    if name == "ld32773":
        register_set(name, *ld_set())
    elif name.startswith("mixed_rare"):
        N = int(name[len("mixed_rare"):])
        rows, pos = mixed_rare(N)
        register_set(name, rows, pos, (1.0, 0.0, 1e-5, 1.0 / len(rows)), N)
    return registered(name)


def columns17(M, seed=17):
    """test_gpu_annot.six_columns and eleven sparse normal columns: one column into the second ANNOT_CHUNK of 16."""
    rng = np.random.default_rng(seed)
    return np.concatenate([six_columns(M), rng.standard_normal((M, 11)) * (rng.random((M, 11)) < 0.3)], axis=1)


def wide_columns(M, seed=23):
    """17 columns, one into the second ANNOT_CHUNK: all-ones, the three classes j % 3, a normal column, that times
    1000, a 2 % binary column, ten sparse normal columns"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(M)
    return np.stack([np.ones(M)] + [(np.arange(M) % 3 == r).astype(float) for r in range(3)] +
                    [z, 1000.0 * z, (rng.random(M) < 0.02).astype(float)] +
                    list((rng.standard_normal((M, 10)) * (rng.random((M, 10)) < 0.3)).T), axis=1)


_truth: dict = {}


def pair_truth(name):
    """(signed_truth of every SNP, seconds it took), once per data set."""
    if name not in _truth:
        t0 = time.perf_counter()
        rows, pos, args, N, bed = named(name)
        _truth[name] = (signed_truth(rows, N, args, pos, bed=bed), time.perf_counter() - t0)
    return _truth[name]


def both_orientations_in_a_window(name):
    """Entries (j, k) of the truth whose rows an orienting engine stores differently (A2 frequency on both sides of
    1/2): where the pairs epilogue's sgi * sgj is -1."""
    rows, pos, args, N, bed = named(name)
    cnt = O.code_counts(bed, len(rows), N)
    hi = cnt[:, 3] > cnt[:, 0]
    return int(sum((hi[p[0]] != hi[j]).sum() for j, p in enumerate(pair_truth(name)[0]) if p is not None))


def split_asserted(e, label):
    t = e.timings()
    assert t["band_kernel"] == "f4_ksplit" and t["ksplit"] > 1, (label, t["band_kernel"], t["ksplit"])
    return int(t["ksplit"])


def pairs_against_truth(e, name, label, dom=True, split=False):
    """The pairs table of `name` (FLAG_EXACT_RARE) against the truth, the seven arrays bitwise the plain run's.
    Returns (worst errors in units of the bar, P, the table)."""
    rows, pos, args, N, bed = named(name)
    flags = EXACT_RARE | (0 if dom else ADDITIVE_ONLY)
    plain = e.run(*args, pos, flags=flags)
    t = e.run_pairs(*args, pos, flags=flags)
    P = split_asserted(e, label) if split else int(e.timings()["ksplit"])
    w = check_rows(t, pair_truth(name)[0], N, np.arange(len(rows)), dom=dom)
    print(f"{label}: worst errors in units of the bar {w}, P = {P}, {t['n_pairs']} pairs")
    assert max(w.values()) <= 1.0, (label, w)
    assert_bitwise(t, plain, label)
    return w, P, t


def annot_against_truth(e, name, annot, label, split=False):
    """The annotated run of `name` (FLAG_EXACT_RARE) against the truth, the seven arrays bitwise the plain run's."""
    rows, pos, args, N, bed = named(name)
    exp2, expd = annot_truth(rows, N, args, pos, annot)
    assert np.isfinite(exp2[:, 0]).sum() >= 30
    got = e.run(*args, pos, flags=EXACT_RARE, annot=annot)
    P = split_asserted(e, label) if split else int(e.timings()["ksplit"])
    rec = dict(l2=assert_truth(got["l2_annot"], exp2, annot, f"{label} l2_annot")["worst_bound_units"],
               l2d=assert_truth(got["l2d_annot"], expd, annot, f"{label} l2d_annot")["worst_bound_units"], P=P)
    assert_bitwise(got, e.run(*args, pos, flags=EXACT_RARE), label)
    return rec


# ---- 1. row lengths -------------------------------------------------------------------------------------------------
def test_rows_of_32773_samples(engines):
    """n32773 (frequencies on both sides of 1/2): the pairs table with dominance and additive-only, 17 annotation
    columns; every run in P > 1 pieces."""
    t0 = time.perf_counter()
    name = "n32773"
    rows, pos, args, N, bed = named(name)
    M = len(rows)
    truth, t_truth = pair_truth(name)
    mixed = both_orientations_in_a_window(name)
    assert sum(p is not None for p in truth) >= 90 and mixed >= 500, mixed
    annot = columns17(M)
    rec = dict(N=N, M=M, truth_s=t_truth, entries_of_mixed_orientation=mixed)
    for orient, e in engines.items():
        load(e, name)
        w, P, t = pairs_against_truth(e, name, f"{name} orient {orient}", split=True)
        wa, Pa, _ = pairs_against_truth(e, name, f"{name} orient {orient} additive-only", dom=False, split=True)
        rec[f"orient {orient}"] = dict(pairs=w, pairs_additive_only=wa, P=P, P_additive_only=Pa, n_pairs=int(t["n_pairs"]),
                                       annot=annot_against_truth(e, name, annot, f"{name} orient {orient} annot",
                                                                 split=True))
    rec["seconds"] = time.perf_counter() - t0
    record("epilogue_shapes_rows_n32773", rec)


def test_row_length_limit(engines):
    """N = 2^19 - 1 (code 11 dominant in the file's coding: Gram entries near 2^23): the pairs table and three
    annotation columns against the truth; the same rows with one more individual are rejected."""
    from nldsc_amd._lib import NLDSCError
    t0 = time.perf_counter()
    name = "cap_epilogue"
    rows, rows_over, pos, args = cap_rows()
    M = len(rows)
    register_set(name, rows, pos, args, CAP_N)
    try:
        codes11 = O.code_counts(dataset(name)[4], M, CAP_N)[:, 3]
        assert (codes11 > 0.45 * CAP_N).all()
        annot = six_columns(M)[:, [0, 1, 3]]
        rec = dict(N=CAP_N, M=M, truth_s=pair_truth(name)[1], largest_gram=float(16 * codes11.max()) / 2 ** 23)
        for orient, e in engines.items():
            load(e, name)
            w, P, t = pairs_against_truth(e, name, f"cap orient {orient}", split=True)
            rec[f"orient {orient}"] = dict(pairs=w, P=P, n_pairs=int(t["n_pairs"]),
                                           annot=annot_against_truth(e, name, annot, f"cap orient {orient} annot",
                                                                     split=True))
        e = engines[0]
        e.load_bed_bytes(b"\x6c\x1b\x01" + rows_over.tobytes(), M, CAP_N + 1)
        for call in (lambda: e.run_pairs(*args, pos, flags=EXACT_RARE),
                     lambda: e.run(*args, pos, flags=EXACT_RARE, annot=annot)):
            with pytest.raises(NLDSCError, match="2\\^19") as ex:
                call()
            assert ex.value.code == E_ARG
    finally:
        forget_set(name)
        _truth.pop(name, None)
    rec["seconds"] = time.perf_counter() - t0
    record("epilogue_shapes_cap", rec)


def test_ld_set_and_filter(engines):
    """Correlated SNPs at N = 32 773 (exact r2adj up to 0.5): the table against the truth, and min_r2 near 0.05, clear
    by 1e-6 of every exact value: the filtered table is the truth's filtered pair set exactly."""
    t0 = time.perf_counter()
    name = "ld32773"
    rows, pos, args, N, bed = named(name)
    M = len(rows)
    truth, t_truth = pair_truth(name)
    allv = np.concatenate([np.concatenate([p[2], p[5]]) for p in truth if p is not None])
    assert len(allv) == 2 * M * (M - 1) and allv.max() > 0.4
    near = int(((allv >= 0.04) & (allv <= 0.06)).sum())
    assert near >= 100, near
    thr = clear_threshold(allv)
    assert thr is not None and 0.04 <= thr <= 0.06
    assert np.abs(allv[np.isfinite(allv)] - thr).min() >= 1e-6
    kept = filtered_truth(truth, thr)
    n_kept = sum(len(p[0]) for p in kept if p is not None)
    assert 0 < n_kept < M * (M - 1)
    rec = dict(N=N, M=M, truth_s=t_truth, min_r2=thr, values_near_threshold=near, kept=n_kept,
               largest_r2adj=float(allv.max()))
    for orient, e in engines.items():
        load(e, name)
        w, P, _ = pairs_against_truth(e, name, f"{name} orient {orient}", split=True)
        t = e.run_pairs(*args, pos, flags=EXACT_RARE, min_r2=thr)
        split_asserted(e, f"{name} filtered")
        assert t["n_pairs"] == n_kept, (t["n_pairs"], n_kept)
        wf = check_rows(t, kept, N, np.arange(M))
        print(f"{name} orient {orient} min_r2 {thr!r}: {n_kept} pairs kept, worst errors in units of the bar {wf}")
        assert max(wf.values()) <= 1.0, wf
        rec[f"orient {orient}"] = dict(pairs=w, filtered=wf, P=P)
    rec["seconds"] = time.perf_counter() - t0
    record("epilogue_shapes_ld_filter", rec)


# ---- 2. schedule independence at P > 1, bitwise ---------------------------------------------------------------------
# batch sizes: 1 (a batch per item: the emit pass computes every batch's Gram tiles again), 4 (two batches at these 5
# or 6 items, the last one smaller), 7 (one batch here), 0 (the default: what the Gram scratch holds, one batch)
BATCHES = (1, 4, 7, 0)


@pytest.mark.parametrize("name", ["n32773", "ld32773"])
def test_schedule_independence(name):
    from nldsc_amd.engine import Engine
    t0 = time.perf_counter()
    rows, pos, args, N, bed = named(name)
    M = len(rows)
    truth = pair_truth(name)[0]
    annot = columns17(M, seed=29)

    def run(kind, options, own=None):
        with Engine(0, options=options) as e:
            e.load_bed_bytes(bed, M, N)
            got = e.run_pairs(*args, pos, flags=EXACT_RARE, own=own) if kind == "pairs" else \
                e.run(*args, pos, flags=EXACT_RARE, annot=annot, own=own)
            return got, e.timings()

    rec = dict(N=N, M=M)
    for kind, option in (("pairs", "pairs_batch_items"), ("annot", "annot_batch_items")):
        base, tb = run(kind, {})
        if kind == "pairs":
            w = check_rows(base, truth, N, np.arange(M))
            assert max(w.values()) <= 1.0, w
        else:
            assert np.isfinite(base["l2_annot"]).sum() >= 90 * annot.shape[1]
        P = {}
        for batch in BATCHES:
            for ksplit in (1, 0):
                got, t = run(kind, {option: batch, "ksplit": ksplit})
                label = f"{name} {kind} {option}={batch} ksplit={ksplit}"
                assert_bitwise(got, base, label)
                if kind == "pairs":
                    assert same_table(got, base), label
                else:
                    assert all(bitwise(got[k], base[k]) for k in ANNOT_KEYS), label
                assert t["band_kernel"] == "f4_ksplit" and t["band_items"] == tb["band_items"]
                if ksplit:
                    P[batch] = int(t["ksplit"])
                else:
                    assert t["ksplit"] == 1, label
        assert tb["band_items"] > 4, tb["band_items"]  # (so batches of 1 and of 4 items are several batches)
        assert P[0] > 1 and (P[1] > 1 or P[4] > 1), P
        rec[kind] = dict(P_by_batch_items=P, band_items=int(tb["band_items"]))
        # owned ranges at P > 1: cuts inside 32-SNP blocks
        cuts = [0, 37, 70, M]
        parts = [run(kind, {}, own=(a, b))[0] for a, b in zip(cuts[:-1], cuts[1:])]
        if kind == "pairs":
            for key in ("k", "r", "rd"):
                assert bitwise(np.concatenate([p[key] for p in parts]), base[key]), key
            ptr = np.concatenate([[0]] + [p["row_ptr"][1:] + off for p, off in
                                          zip(parts, np.cumsum([0] + [p["n_pairs"] for p in parts[:-1]]))])
            assert np.array_equal(ptr, base["row_ptr"])
        else:
            for (a, b), p in zip(zip(cuts[:-1], cuts[1:]), parts):
                for k in ANNOT_KEYS + ("l2", "l2d", "l2_ws"):
                    assert bitwise(p[k][a:b], base[k][a:b]), (k, a, b)
                assert np.isnan(p["l2_annot"][:a]).all() and np.isnan(p["l2_annot"][b:]).all()
    rec["seconds"] = time.perf_counter() - t0
    record(f"epilogue_shapes_schedule_{name}", rec)


# ---- 3. missing-free blocks beside blocks with missing calls --------------------------------------------------------
@pytest.mark.parametrize("name", ["blocks_mixed", "blocks_free"])
def test_missing_free_and_mixed_blocks(engines, name):
    """Blocks whose m-products the partial kernel skips beside blocks with missing calls, and a set without any."""
    t0 = time.perf_counter()
    rows, pos, args, N, bed = named(name)
    M = len(rows)
    nblk = (M + 31) // 32
    free = missing_free_blocks(rows, N)
    assert free == (4 if name == "blocks_mixed" else nblk) and nblk == 11, free
    annot = six_columns(M)
    rec = dict(N=N, M=M, truth_s=pair_truth(name)[1], missing_free_blocks=free, blocks=nblk,
               entries_of_mixed_orientation=both_orientations_in_a_window(name))
    assert rec["entries_of_mixed_orientation"] >= 1000
    for orient, e in engines.items():
        load(e, name)
        w, P, t = pairs_against_truth(e, name, f"{name} orient {orient}")
        rec[f"orient {orient}"] = dict(pairs=w, P=P, n_pairs=int(t["n_pairs"]),
                                       annot=annot_against_truth(e, name, annot, f"{name} orient {orient} annot"))
    rec["seconds"] = time.perf_counter() - t0
    record(f"epilogue_shapes_{name}", rec)


# ---- 4. replayed rare variants under the default flags: the signs ---------------------------------------------------
def flat(truth):
    """signed_truth of every SNP as a table: row_ptr, k, r, rd (NaN where the pair is not in the row's kd)."""
    lens = [0 if p is None else len(p[0]) for p in truth]
    ks, r, rd = [], [], []
    for p in truth:
        if p is None:
            continue
        ks.append(p[0])
        r.append(p[1])
        d = np.full(len(p[0]), np.nan)
        d[p[3]] = p[4]
        rd.append(d)
    return dict(row_ptr=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), k=np.concatenate(ks).astype(np.int64),
                r=np.concatenate(r), rd=np.concatenate(rd))


def bar_units(got, exp):
    return np.abs(got - exp) / (ABS + REL * np.abs(exp))


def tol_units(got, exp):
    atol, rtol = TOL["l2d"]
    return np.abs(got - exp) / (atol + rtol * np.abs(exp))


def oracle_pair(rows, N, args, j, k):
    """The C oracle on the two-row file (j, k), both rows inside one window: r2adj(r(j, k)) and r2adj(rd(j, k)) in the
    reference's own arithmetic (the latter None where the reference does not count k in WSD[j])."""
    from nldsc_amd import synth
    o = O.run_c(synth.bed_bytes(rows[[j, k]]), 2, N, 1.0, args[1], args[2], args[3], np.array([0.0, 0.5]), threads=1)
    assert o["l2_ws"][0] == 1
    return float(o["l2"][0] - 1.0), (float(o["l2d"][0]) if o["l2d_ws"][0] == 1 else None)


@pytest.mark.parametrize("N", [4099, 32773])
def test_replayed_signs(engines, N):
    """mixed_rare under the default flags (the replay on, KC items), with dominance, on both orientations."""
    t0 = time.perf_counter()
    name = f"mixed_rare{N}"
    rows, pos, args, _, bed = named(name)
    M = len(rows)
    truth, t_truth = pair_truth(name)
    s = O.f64_setup(rows, N, args[0], args[1], args[2], pos, bed=bed)
    cnt = O.code_counts(bed, M, N)[:, [0, 2, 3]]
    replayed = s["passed"] & (cnt.sum(1) > 0) & (cnt.min(1) <= REPLAY_MAX_CLASS)
    a1_minor = np.arange(M) % 4 < 2
    assert 60 <= replayed.sum() <= 70 and replayed[::2].sum() >= 60, int(replayed.sum())
    ex = flat(truth)
    j, k = rows_of(ex), ex["k"]
    cls = 8 * replayed[j] + 4 * a1_minor[j] + 2 * replayed[k] + a1_minor[k]
    clear = np.abs(ex["r"]) >= SIGN_MARGIN
    per_class = np.bincount(cls[clear], minlength=16)
    assert (per_class >= 100).all(), per_class
    # both signs in every class but two: two replayed SNPs of the same minor allele (classes 10 and 15) are two rare
    # variants, whose alleles correlate at about minus their frequency unless a carrier is shared - and with A1 minor
    # the padding pair the reference reads at N % 4 != 0 is a shared hom-minor call, which makes every such r positive
    positive = np.bincount(cls[clear & (ex["r"] > 0)], minlength=16)
    for c in range(16):
        assert c in (10, 15) or min(positive[c], per_class[c] - positive[c]) >= 10, (c, positive, per_class)
    rep = replayed[j] | replayed[k]
    clear_d = np.abs(ex["rd"]) >= SIGN_MARGIN  # (NaN compares false)
    assert (rep & clear_d).sum() >= 500

    # the sample for the magnitudes: 18 entries of every class with a replayed SNP, spread over the class's clear ones
    sample = np.concatenate([(lambda i: i[np.linspace(0, len(i) - 1, 18).astype(int)])(np.flatnonzero(clear & (cls == c)))
                             for c in range(16) if c & 10])
    assert len(sample) >= 200 and rep[sample].all()
    orc = [oracle_pair(rows, N, args, int(j[i]), int(k[i])) for i in sample]
    orc_r = np.array([o[0] for o in orc])
    has_d = np.array([o[1] is not None for o in orc])
    orc_d = np.array([np.nan if o[1] is None else o[1] for o in orc])
    ex_d = ~np.isnan(ex["rd"][sample])
    both = has_d & ex_d
    assert np.array_equal(has_d, ex_d) and has_d.sum() >= 100  # (no residual flag of the sample differs: see below)
    # the oracle's own distance from the exact truth, per quantity, in units of the bar; above it, twice that distance
    # is what the engine is held to
    oracle_vs_exact = dict(r=float(tol_units(orc_r, r2adj(ex["r"][sample], N)).max()),
                           rd=float(tol_units(orc_d[both], r2adj(ex["rd"][sample][both], N)).max()))
    limit = {q: 1.0 if d <= 1.0 else 2.0 * d for q, d in oracle_vs_exact.items()}
    print(f"{name}: the oracle against the exact truth on {len(sample)} pairs, in units of the bar: {oracle_vs_exact}; "
          f"the engine is held to {limit} against the oracle")
    rec = dict(N=N, M=M, truth_s=t_truth, replayed=int(replayed.sum()), entries=int(len(k)),
               clear_entries_per_class=per_class.tolist(), positive_of_them=positive.tolist(), sample=int(len(sample)),
               sample_with_rd=int(has_d.sum()),
               oracle_vs_exact_bar_units=oracle_vs_exact, engine_vs_oracle_limit_bar_units=limit)

    annot = np.stack([np.ones(M)] + [(np.arange(M) % 3 == c).astype(float) for c in range(3)], axis=1)
    tables = {}
    for orient, e in engines.items():
        label = f"{name} orient {orient}"
        load(e, name)
        plain = e.run(*args, pos)
        t = tables[orient] = e.run_pairs(*args, pos)
        assert_bitwise(t, plain, label)
        # neighbour sets: exact
        assert np.array_equal(t["row_ptr"], ex["row_ptr"]) and np.array_equal(t["k"], k), label
        # rd's NaN pattern: exact, but in the rows with a replayed neighbour whose residual-std flag the replay changes
        flag_changed = replayed & ((plain["residuals_std"] > args[2]) != s["rpass"])
        excluded_rows = np.bincount(j[flag_changed[k]], minlength=M) > 0
        n_rows = int((np.diff(ex["row_ptr"]) > 0).sum())
        assert excluded_rows.sum() <= 0.02 * n_rows, (label, int(excluded_rows.sum()), n_rows)
        held = ~excluded_rows[j]
        assert np.array_equal(np.isnan(t["rd"][held]), np.isnan(ex["rd"][held])), label
        # neither SNP replayed: the exact-path bar
        m = ~rep
        md = m & held & ~np.isnan(ex["rd"])
        w_r = float(bar_units(t["r"][m], ex["r"][m]).max())
        w_rd = float(bar_units(t["rd"][md], ex["rd"][md]).max())
        print(f"{label}: entries without a replayed SNP, worst in units of the bar: r {w_r:.3g}, rd {w_rd:.3g}")
        assert m.sum() >= 1000 and md.sum() >= 500 and w_r <= 1.0 and w_rd <= 1.0, (label, w_r, w_rd)
        # a replayed SNP: the signs
        ms, msd = rep & clear, rep & held & clear_d & ~np.isnan(t["rd"])
        bad = np.flatnonzero(ms & (np.sign(t["r"]) != np.sign(ex["r"])))
        assert bad.size == 0, (label, "sign of r", bad[:10], j[bad[:10]], k[bad[:10]], cls[bad[:10]])
        bad = np.flatnonzero(msd & (np.sign(t["rd"]) != np.sign(ex["rd"])))
        assert bad.size == 0, (label, "sign of rd", bad[:10], j[bad[:10]], k[bad[:10]], cls[bad[:10]])
        # ... and the magnitudes, against the reference
        assert np.array_equal(~np.isnan(t["rd"][sample]), has_d), label
        u_r = float(tol_units(r2adj(t["r"][sample], N), orc_r).max())
        u_d = float(tol_units(r2adj(t["rd"][sample][has_d], N), orc_d[has_d]).max(initial=0))
        print(f"{label}: r2adj against the oracle on the sample, worst in units of the bar: r {u_r:.3g}, rd {u_d:.3g}")
        assert u_r <= limit["r"] and u_d <= limit["rd"], (label, u_r, u_d, limit)
        # the annotated run under the same flags
        got = e.run(*args, pos, annot=annot)
        assert_bitwise(got, plain, f"{label} annot")
        worst = {}
        for key, ref in (("l2_annot", plain["l2"]), ("l2d_annot", plain["l2d"])):
            for c in range(annot.shape[1]):
                assert np.array_equal(np.isnan(got[key][:, c]), np.isnan(ref)), (label, key, c)
            ok = ~np.isnan(ref)
            worst[key] = (float(np.abs(got[key][ok, 0] - ref[ok]).max()),
                          float(np.abs(got[key][ok, 1:4].sum(axis=1) - ref[ok]).max()))
            assert ok.sum() >= 100 and max(worst[key]) <= 1e-9, (label, key, worst[key])
        rec[f"orient {orient}"] = dict(signs_checked=(int(ms.sum()), int(msd.sum())), rows_excluded=int(excluded_rows.sum()),
                                       unreplayed_r=w_r, unreplayed_rd=w_rd, sample_r_vs_oracle=u_r,
                                       sample_rd_vs_oracle=u_d, annot_ones_and_partition=worst,
                                       kernel=e.timings()["band_kernel"], P=int(e.timings()["ksplit"]))
    # the two orientations
    a, b = tables[0], tables[1]
    assert np.array_equal(a["row_ptr"], b["row_ptr"]) and np.array_equal(a["k"], b["k"])
    for key in ("r", "rd"):
        assert np.array_equal(np.isnan(a[key]), np.isnan(b[key])), key
        ok = ~np.isnan(a[key])
        assert np.array_equal(np.sign(a[key][ok]), np.sign(b[key][ok])), key
        m = ok & ~rep
        assert (bar_units(a[key][m], b[key][m]) <= 2.0).all(), key
        m = ok & rep
        assert (tol_units(r2adj(a[key][m], N), r2adj(b[key][m], N)) <= 2.0 * limit[key]).all(), key
    rec["seconds"] = time.perf_counter() - t0
    record(f"epilogue_shapes_replayed_signs_{N}", rec)


# ---- 5. the annotated epilogue on wide windows ----------------------------------------------------------------------
_wide: dict = {}


def wide_case(engines, which):
    """Short rows (N = 67, FLAG_EXACT_RARE as test_gpu_pairs.test_ragged) on engines[1], 17 columns: "full_window"
    (M = 289 in one window) or "ragged" (M = 3 001, a 230-SNP tie); the set is loaded when this returns.  The runs are
    made once."""
    e = engines[1]
    if which not in _wide:
        if which == "full_window":
            M, rows, bed, pos, args = full_window_set()
            tg = np.unique(np.concatenate([[0, 1, M - 2, M - 1], np.arange(31, M, 32), np.arange(32, M, 32),
                                           np.random.default_rng(M).choice(M, 24, replace=False)]))
        else:
            M, rows, bed, pos, args, run, ties = ragged_set()
            tg = ragged_targets(M, run, ties)
        _wide[which] = dict(M=M, rows=rows, bed=bed, pos=pos, args=args, tg=tg, annot=wide_columns(M))
    d = _wide[which]
    e.set_keep(None)
    e.load_bed_bytes(d["bed"], d["M"], N67)
    if "got" not in d:
        d["plain"] = e.run(*d["args"], d["pos"], flags=EXACT_RARE)
        d["got"] = e.run(*d["args"], d["pos"], flags=EXACT_RARE, annot=d["annot"])
        d["items"] = int(e.timings()["band_items"])
    return e, d


@pytest.mark.parametrize("which", ["full_window", "ragged"])
def test_annot_wide_windows(engines, which):
    """Hundreds of items behind one SNP's accumulators: the all-ones column and a partition against l2 / l2d, >= 40
    targets (first, last, block edges, the 230-SNP tie) against the truth, bitwise the same in batches of 7 items."""
    t0 = time.perf_counter()
    e, d = wide_case(engines, which)
    M, pos, args, tg, annot, plain, got = (d[k] for k in ("M", "pos", "args", "tg", "annot", "plain", "got"))
    assert annot.shape[1] == 17 and len(tg) >= 40
    assert_bitwise(got, plain, which)
    widest = int(plain["l2_ws"].max())
    assert widest >= 200 and d["items"] > 7, (widest, d["items"])
    rec = dict(N=N67, M=M, targets=int(len(tg)), widest_window=widest, band_items=d["items"])
    for key, ref in (("l2_annot", plain["l2"]), ("l2d_annot", plain["l2d"])):
        ok = ~np.isnan(ref)
        for c in range(annot.shape[1]):
            assert np.array_equal(np.isnan(got[key][:, c]), ~ok), (key, c)
        ones = float(np.abs(got[key][ok, 0] - ref[ok]).max())
        part = float(np.abs(got[key][ok, 1:4].sum(axis=1) - ref[ok]).max())
        print(f"{which} {key}: all-ones {ones:.3g}, partition {part:.3g}")
        assert ok.sum() >= 200 and ones <= 1e-9 and part <= 1e-9, (key, ones, part)
        rec[key] = dict(all_ones=ones, partition=part)
    t1 = time.perf_counter()
    exp2, expd = annot_truth(d["rows"], N67, args, pos, annot, targets=tg)
    rec["truth_s"] = time.perf_counter() - t1
    assert np.isfinite(exp2[tg, 0]).sum() >= 30
    rec["l2_truth"] = assert_truth(got["l2_annot"][tg], exp2[tg], annot, f"{which} l2_annot")["worst_bound_units"]
    rec["l2d_truth"] = assert_truth(got["l2d_annot"][tg], expd[tg], annot, f"{which} l2d_annot")["worst_bound_units"]
    e.set_option("annot_batch_items", 7)
    try:
        again = e.run(*args, pos, flags=EXACT_RARE, annot=annot)
    finally:
        e.set_option("annot_batch_items", 0)
    assert_bitwise(again, got, f"{which} annot_batch_items=7")
    assert all(bitwise(again[k], got[k]) for k in ANNOT_KEYS)
    rec["seconds"] = time.perf_counter() - t0
    record(f"epilogue_shapes_annot_{which}", rec)


@pytest.mark.parametrize("which", ["full_window", "ragged"])
def test_annot_wide_windows_times_1000(engines, which):
    """The x1000 column within relative 1e-12 of 1000 x its base, per value: test_gpu_annot.test_times_1000_column's
    bar on the wide windows.

    With a standard normal column over windows of 150 to 400 neighbours some sums cancel: L2D of SNP 2219 of "ragged"
    is 4.34e-5, a sum of 151 terms z_k r2adj_k whose magnitudes add up to 1.69 (condition number 3.9e4; 4 of the 2 775
    L2D values have one above 1e-12 / 2.2e-16).  While the epilogue rounded every product and every 32-term partial in
    fp64 the two columns differed there by 1.59e-12 (0.2 ulp of the terms' magnitude) and this case failed; since it
    splits every term exactly into its two fixed-point parts before any sum (annot_term) the worst gap on the MI355X
    is 9.8e-14, the one of exact arithmetic on these inputs (1000 z is itself rounded).  Should a value miss the bar,
    the values themselves are held to the truth before the comparison fails."""
    e, d = wide_case(engines, which)
    annot, plain, got = d["annot"], d["plain"], d["got"]
    rec, over_all = {}, []
    for key, ref in (("l2_annot", plain["l2"]), ("l2d_annot", plain["l2d"])):
        js = np.flatnonzero(~np.isnan(ref))
        base, big = got[key][js, 4], got[key][js, 5]
        rel = np.abs(big - 1000.0 * base) / np.maximum(np.abs(1000.0 * base), 1e-300)
        order = np.argsort(rel)[::-1]
        over = js[rel > 1e-12]
        print(f"{which} {key}: x1000 worst relative {rel[order[0]]:.4g} at SNP {js[order[0]]} (base {base[order[0]]:.6g}), "
              f"then {rel[order[1]]:.4g}; {len(over)} of {len(js)} values above 1e-12")
        rec[key] = dict(worst=float(rel[order[0]]), worst_snp=int(js[order[0]]), second=float(rel[order[1]]),
                        above=int(len(over)), of=int(len(js)))
        over_all += [(key, int(j)) for j in over]
    record(f"epilogue_shapes_annot_x1000_{which}", rec)
    if over_all:  # the values themselves against the truth, before the comparison of the two columns
        tg = np.unique([j for _, j in over_all])
        exp2, expd = annot_truth(d["rows"], N67, d["args"], d["pos"], annot, targets=tg)
        assert_truth(got["l2_annot"][tg], exp2[tg], annot, f"{which} l2_annot of SNPs {tg}")
        assert_truth(got["l2d_annot"][tg], expd[tg], annot, f"{which} l2d_annot of SNPs {tg}")
    assert not over_all, (over_all, rec)
