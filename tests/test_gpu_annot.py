"""Partitioned LD scores (nldsc_engine_run_annot, --annot): L2[j, c] = a[j, c] + sum_k a[k, c] r2adj(j, k) and the
dominance counterpart, per annotation column c.

Truth: oracle.pair_r2_f64 (integer contingency tables, binary64 per pair), weighted here in numpy.  Throughout,
A_c = max(1, max |a_c|).  The bound against the truth is the project's exact-path bar (1e-9, 1e-12) of
tests/test_gpu_parity.py carried through the linear weighting: 1e-9 A_c + 1e-12 |expected|."""
import gzip
import os
import shutil
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO, load_set, rare_variant_set, record
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")
ADDITIVE_ONLY, EXACT_I8, FP32, EXACT_RARE = 2, 4, 8, 32  # _lib.FLAG_*
SETS = ["n1000", "n1001", "n1002", "n1003", "allmiss", "allmiss_pad", "rare1003"]


@pytest.fixture(scope="module")
def engine():
    import torch
    torch.cuda.init()  # one HIP runtime per process (tests/test_gpu_parity.py)
    from nldsc_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


_sets: dict = {}


def dataset(name):
    """(rows, positions, run arguments (ld_wind, maf, std_thr, rsq_thr), n_org, bed bytes), made once."""
    if name not in _sets:
        from nldsc_amd import synth
        if name == "rare1003":
            rows, pos = rare_variant_set(1003)
            args, N, bed = (1.0, 1e-5, 1e-5, 1.0 / len(rows)), 1003, synth.bed_bytes(rows)
        else:
            bed, pos, meta, _, _ = load_set(name)
            rows = np.frombuffer(bed, np.uint8, offset=3).reshape(meta["n_snp"], -1)
            args, N = (meta["ld_wind"], meta["maf"], meta["std_thr"], meta["rsq_thr"]), meta["n_org"]
        _sets[name] = (rows, pos, args, N, bed)
    return _sets[name]


def load(engine, name):
    rows, pos, args, N, bed = dataset(name)
    engine.set_keep(None)
    engine.load_bed_bytes(bed, len(rows), N)
    return pos, args


def bitwise(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_plain_bitwise(got, exp, label):
    for k in KEYS:
        assert bitwise(got[k], exp[k]), f"{label}: {k} differs from the plain run"


def six_columns(M, seed=21):
    """all-ones; binary 30 %; binary 2 % (whole 32-SNP blocks zero); standard normal; that times 1000; all-zero"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(M)
    return np.stack([np.ones(M), (rng.random(M) < 0.3).astype(float), (rng.random(M) < 0.02).astype(float), z,
                     1000.0 * z, np.zeros(M)], axis=1)


def truth(rows, N, args, pos, annot, strict=False, targets=None):
    """(L2[j, c], L2D[j, c]) from the exact per-pair r2adj; NaN rows for SNPs that are not computed (and, with
    `targets`, for every SNP that is none of them)."""
    M, C = annot.shape
    l2, l2d = np.full((M, C), np.nan), np.full((M, C), np.nan)
    targets = np.arange(M) if targets is None else np.asarray(targets)
    for j, p in zip(targets, O.pair_r2_f64(rows, N, args[0], args[1], args[2], pos, targets, strict=strict)):
        if p is None:
            continue
        ks, r2a, kds, r2d = p
        l2[j] = annot[j] + (annot[ks] * np.asarray(r2a)[:, None]).sum(0)
        l2d[j] = (annot[kds] * np.asarray(r2d)[:, None]).sum(0)
    return l2, l2d


def assert_truth(got, exp, annot, label):
    """|got - exp| <= 1e-9 A_c + 1e-12 |exp| per column, equal NaN patterns; returns the worst error in bound units
    and the worst absolute error per column."""
    A = np.maximum(1.0, np.abs(annot).max(axis=0))
    assert np.array_equal(np.isnan(got), np.isnan(exp)), f"{label}: NaN pattern"
    m = ~np.isnan(exp)
    err = np.where(m, np.abs(got - np.where(m, exp, 0.0)), 0.0)
    lim = 1e-9 * A[None, :] + 1e-12 * np.abs(np.where(m, exp, 0.0))
    worst = float((err / lim).max(initial=0))
    print(f"{label}: worst |d| per column {err.max(axis=0)}, worst in units of the bound {worst:.3g}")
    assert worst <= 1.0, f"{label}: {int((err > lim).sum())} values out of tolerance, worst {worst:.3g} x the bound"
    return dict(worst_bound_units=worst, max_abs_per_column=err.max(axis=0).tolist())


@pytest.fixture(scope="module")
def truth_n1001():
    rows, pos, args, N, _ = dataset("n1001")
    annot = six_columns(len(rows))
    return annot, truth(rows, N, args, pos, annot)


def test_exact_truth(engine, truth_n1001):
    """1. n1001, FLAG_EXACT_RARE, six columns against the fp64 truth; the same additive-only (l2d_annot all NaN)."""
    annot, (exp2, expd) = truth_n1001
    pos, args = load(engine, "n1001")
    got = engine.run(*args, pos, flags=EXACT_RARE, annot=annot)
    assert np.isfinite(exp2[:, 0]).sum() > 1000
    rec = dict(l2=assert_truth(got["l2_annot"], exp2, annot, "n1001 l2_annot"),
               l2d=assert_truth(got["l2d_annot"], expd, annot, "n1001 l2d_annot"))
    add = engine.run(*args, pos, flags=EXACT_RARE | ADDITIVE_ONLY, annot=annot)
    rec["l2_additive_only"] = assert_truth(add["l2_annot"], exp2, annot, "n1001 additive-only l2_annot")
    assert np.isnan(add["l2d_annot"]).all() and np.isnan(add["l2d"]).all()
    record("annot_truth_n1001", rec)


@pytest.fixture(scope="module")
def plain_and_annot(engine):
    """per set: (plain run, annotated run, annotation matrix) with default flags; columns: all-ones, the three classes
    j % 3, a standard normal column and that times 1000"""
    out = {}

    def get(name):
        if name not in out:
            pos, args = load(engine, name)
            M = len(pos)
            z = np.random.default_rng(33).standard_normal(M)
            annot = np.stack([np.ones(M)] + [(np.arange(M) % 3 == r).astype(float) for r in range(3)] +
                             [z, 1000.0 * z], axis=1)
            out[name] = (engine.run(*args, pos), engine.run(*args, pos, annot=annot), annot)
        return out[name]
    return get


@pytest.mark.parametrize("name", SETS)
def test_ordinary_arrays_unchanged(plain_and_annot, name):
    """2. the seven ordinary arrays are bitwise a plain run's; NaN patterns of the per-annotation scores are those of
    l2 / l2d."""
    plain, got, annot = plain_and_annot(name)
    assert_plain_bitwise(got, plain, name)
    assert np.isfinite(plain["l2"]).sum() > len(plain["l2"]) // 4
    for c in range(annot.shape[1]):
        assert np.array_equal(np.isnan(got["l2_annot"][:, c]), np.isnan(plain["l2"])), (name, c)
        assert np.array_equal(np.isnan(got["l2d_annot"][:, c]), np.isnan(plain["l2d"])), (name, c)


@pytest.mark.parametrize("name", SETS)
def test_consistent_with_the_plain_score(plain_and_annot, name):
    """3. the all-ones column is l2 / l2d, and a partition of the SNPs sums to them, within 1e-9: each item's partial
    is rounded to 2^-45, a SNP is touched by a few hundred items at most and a 32-term fp64 sum of values <= 1 errs
    below 1e-13, so the true gap is below 1e-11; 1e-9 is the project's exact-path bar."""
    plain, got, annot = plain_and_annot(name)
    worst = {}
    for key, ref in (("l2_annot", plain["l2"]), ("l2d_annot", plain["l2d"])):
        m = ~np.isnan(ref)
        ones = np.abs(got[key][m, 0] - ref[m]).max(initial=0)
        part = np.abs(got[key][m, 1:4].sum(axis=1) - ref[m]).max(initial=0)
        worst[key] = (float(ones), float(part))
        print(f"{name} {key}: all-ones {ones:.3g}, partition {part:.3g}")
        assert ones <= 1e-9 and part <= 1e-9, (name, key, ones, part)
    record(f"annot_consistency_{name}", worst)


def test_times_1000_column(plain_and_annot):
    """3 (last item). the x1000 column equals 1000 x its base column within relative 1e-12, taken per value:
    |V - 1000 b| <= 1e-12 |1000 b|.  The two columns accumulate at different fixed-point scales (2^-42 and 2^-32 for a
    standard normal column); every term a r2 is split exactly into a part at that scale and a residual part before
    any sum (annot_term), so the totals are the sums of their terms.  In exact arithmetic on these inputs (1000 z is
    itself rounded) the worst relative gap is 9.4e-14; measured on the MI355X: 9.2e-14 (3.0e-13 while the products and
    an item's partial sums were rounded in fp64)."""
    bad, rec = [], {}
    for name in SETS:
        plain, got, annot = plain_and_annot(name)
        for key in ("l2_annot", "l2d_annot"):
            base, big = got[key][:, 4], got[key][:, 5]
            m = ~np.isnan(base)
            err = np.abs(big[m] - 1000.0 * base[m])
            rel = err / np.maximum(np.abs(1000.0 * base[m]), 1e-300)
            over = int((err > 1e-12 * np.abs(1000.0 * base[m])).sum())
            rec[f"{name} {key}"] = dict(max_abs=float(err.max(initial=0)), max_rel=float(rel.max(initial=0)),
                                        above=over, of=int(m.sum()))
            print(f"{name} {key}: x1000 worst |d| {err.max(initial=0):.3g}, worst relative {rel.max(initial=0):.3g}, "
                  f"{over} of {int(m.sum())} values above 1e-12")
            if over:
                bad.append((name, key, over))
    record("annot_x1000", rec)
    assert not bad, bad


@pytest.mark.parametrize("name", ["n1003", "rare1003"])
def test_schedule_independence(name):
    """4. bitwise equal per-annotation scores across batch sizes, K-split, both planners, the fused plan, t2."""
    from nldsc_amd.engine import Engine
    rows, pos, args, N, bed = dataset(name)
    M = len(rows)
    annot = six_columns(M, seed=8)
    settings = [{}] + [{"annot_batch_items": b} for b in (7, 1)] + [{"ksplit": 0}, {"gpu_plan": 0},
                                                                     {"plan_fused": 0}, {"t2": 0},
                                                                     {"annot_batch_items": 7, "ksplit": 0, "t2": 0},
                                                                     {"annot_batch_items": 7, "gpu_plan": 0}]
    ref = None
    for opts in settings:
        with Engine(0, options=opts) as e:
            e.load_bed_bytes(bed, M, N)
            got = e.run(*args, pos, annot=annot)
        if ref is None:
            ref = got
            assert np.isfinite(ref["l2_annot"]).sum() > M
            continue
        for k in ("l2_annot", "l2d_annot") + KEYS:
            assert bitwise(got[k], ref[k]), (name, opts, k)


def test_owned_range_and_slice(engine, tmp_path):
    """5. own = (300, 900): sentinels outside survive, values inside are the full run's; a load_bed_file_range slice
    [200, 700) with its annotation rows equals those rows loaded plainly."""
    from nldsc_amd import synth
    rows, pos, args, N, bed = dataset("n1003")
    M = len(rows)
    annot = six_columns(M, seed=9)
    C = annot.shape[1]
    pos_, _ = load(engine, "n1003")
    full = engine.run(*args, pos, annot=annot)
    out = dict(l2=np.full(M, -7.0), l2d=np.full(M, -7.0), maf=np.full(M, -7.0), residuals_std=np.full(M, -7.0),
               l2_ws=np.full(M, -7, np.int32), l2d_ws=np.full(M, -7, np.int32), l2d_wse=np.full(M, -7, np.int32),
               l2_annot=np.full((C, M), -7.0).T, l2d_annot=np.full((C, M), -7.0).T)
    got = engine.run(*args, pos, own=(300, 900), out=out, annot=annot)
    for k in ("l2_annot", "l2d_annot"):
        assert (got[k][:300] == -7.0).all() and (got[k][900:] == -7.0).all(), k
        assert bitwise(got[k][300:900], full[k][300:900]), k
    for k in KEYS:
        assert (got[k][:300] == -7).all() and (got[k][900:] == -7).all() and bitwise(got[k][300:900], full[k][300:900])
    path = tmp_path / "n1003.bed"
    path.write_bytes(bed)
    engine.load_bed_file_range(str(path), M, N, 200, 700)
    sl = engine.run(*args, pos[200:700], annot=annot[200:700])
    engine.load_bed_bytes(synth.bed_bytes(rows[200:700]), 500, N)
    exp = engine.run(*args, pos[200:700], annot=annot[200:700])
    for k in ("l2_annot", "l2d_annot") + KEYS:
        assert bitwise(sl[k], exp[k]), k
    assert np.isfinite(sl["l2_annot"]).sum() > 500


@pytest.mark.parametrize("M,N", [(20, 50), (33, 67)])
@pytest.mark.parametrize("C", [1, 70])
def test_small_shapes(engine, M, N, C):
    """6. one diagonal item; two blocks, the second holding one SNP; C = 70: more than one LDS chunk, more than 64
    columns."""
    from nldsc_amd import synth
    rng = np.random.default_rng(100 * M + C)
    g = rng.binomial(2, rng.uniform(0.2, 0.5, M)[:, None], (M, N)).astype(np.int8)
    g[rng.random((M, N)) < 0.02] = -1
    rows = synth.pack_bed_rows(g)
    pos = np.cumsum(rng.exponential(0.05, M))
    args = (1.0, 1e-5, 1e-5, 1.0 / M)
    annot = rng.standard_normal((M, C)) * (rng.random((M, C)) < 0.7)
    annot[:, 0] = 1.0
    engine.set_keep(None)
    engine.load_bed_bytes(synth.bed_bytes(rows), M, N)
    got = engine.run(*args, pos, flags=EXACT_RARE, annot=annot)
    exp2, expd = truth(rows, N, args, pos, annot)
    assert np.isfinite(exp2).sum() > M * C // 2
    assert_truth(got["l2_annot"], exp2, annot, f"M={M} C={C} l2_annot")
    assert_truth(got["l2d_annot"], expd, annot, f"M={M} C={C} l2d_annot")
    assert_plain_bitwise(got, engine.run(*args, pos, flags=EXACT_RARE), f"M={M} C={C}")


def _subset_rows(rows, n_org, idx):
    from nldsc_amd import synth
    geno_of_code = np.array([0, -1, 1, 2], np.int8)
    return synth.pack_bed_rows(geno_of_code[O.unpack_codes(rows, n_org, strict=True)[:, idx]])


def test_keep_list(engine):
    """7. an annotated run after a keep-load is bitwise the annotated strict-order run on the subset file."""
    from nldsc_amd import synth
    rows, pos, args, N, bed = dataset("n1001")
    M = len(rows)
    annot = six_columns(M, seed=10)
    idx = np.sort(np.random.default_rng(12).choice(N, 601, replace=False)).astype(np.int32)
    engine.set_keep(None)
    engine.load_bed_bytes(synth.bed_bytes(_subset_rows(rows, N, idx)), M, len(idx))
    exp = engine.run(*args, pos, flags=1, annot=annot)  # FLAG_STRICT_PLINK_ORDER
    try:
        engine.set_keep(idx, N)
        engine.load_bed_bytes(bed, M, N)
        got = engine.run(*args, pos, annot=annot)
    finally:
        engine.set_keep(None)
    for k in ("l2_annot", "l2d_annot") + KEYS:
        assert bitwise(got[k], exp[k]), k
    assert np.isfinite(got["l2_annot"]).sum() > M


def test_rejections(engine):
    """8. each returns E_ARG with a message; a plain run still works afterwards."""
    from nldsc_amd import _lib, synth
    from nldsc_amd.engine import Engine
    pos, args = load(engine, "n1001")
    M = len(pos)
    ones = np.ones((M, 2))

    def rejected(annot, match, flags=0, eng=engine, pos=pos):
        with pytest.raises(_lib.NLDSCError, match=match) as ex:
            eng.run(*args, pos, flags=flags, annot=annot)
        assert ex.value.code == _lib.E_ARG

    rejected(np.ones((M, 0)), "n_annot")
    rejected(np.ones((M, _lib.MAX_ANNOT + 1)), "n_annot")
    for bad in (np.nan, np.inf, -np.inf):
        a = ones.copy()
        a[17, 1] = bad
        rejected(a, "not finite")
    rejected(ones, "fp4", flags=FP32)
    rejected(ones, "fp4", flags=EXACT_I8)
    for mode in (0, 1):
        with Engine(0, options={"band_mode": mode}) as e:
            e.load_bed_bytes(dataset("n1001")[4], M, dataset("n1001")[3])
            rejected(ones, "fp4", eng=e)
    plain = engine.run(*args, pos)
    assert np.isfinite(plain["l2"]).sum() > 1000
    # n_org = 2^19 (the part kernel's unsegmented rows end there): 40 synthetic rows
    N2, M2 = 1 << 19, 40
    rng = np.random.default_rng(3)
    rows2 = rng.integers(0, 256, (M2, N2 // 4), dtype=np.uint8)
    rows2 &= ~((rows2 & 0x55) & ~((rows2 >> 1) & 0x55))  # no missing calls: pairs 01 -> 00
    pos2 = np.arange(M2, dtype=np.float64) * 0.01
    with Engine(0) as e:
        e.load_bed_bytes(synth.bed_bytes(rows2), M2, N2)
        with pytest.raises(_lib.NLDSCError, match="2\\^19") as ex:
            e.run(1.0, 1e-5, 1e-5, 1.0 / M2, pos2, annot=np.ones((M2, 1)))
        assert ex.value.code == _lib.E_ARG
        assert np.isfinite(e.run(1.0, 1e-5, 1e-5, 1.0 / M2, pos2)["l2"]).sum() > 0


@pytest.fixture(scope="module")
def annot_case(engine, tmp_path_factory):
    """n1001 with a full-form .annot file, its .gz, and the engine's annotated result (default flags)."""
    d = tmp_path_factory.mktemp("annot")
    rows, pos, args, N, bed = dataset("n1001")
    M = len(rows)
    rng = np.random.default_rng(44)
    names = ["base", "coding", "cons_score"]
    annot = np.stack([np.ones(M), (rng.random(M) < 0.1).astype(float), np.round(rng.standard_normal(M), 4)], axis=1)
    bim = [ln.split("\t") for ln in open(os.path.join(GOLDEN, "n1001.bim")).read().splitlines()]
    text = "CHR\tBP\tSNP\tCM\t" + "\t".join(names) + "\n" + "".join(
        f"{b[0]}\t{b[3]}\t{b[1]}\t{b[2]}\t" + "\t".join(repr(float(v)) for v in annot[j]) + "\n"
        for j, b in enumerate(bim))
    (d / "n1001.annot").write_text(text)
    with gzip.open(d / "n1001.annot.gz", "wt") as fh:
        fh.write(text)
    load(engine, "n1001")
    return d, names, annot, engine.run(*args, pos, annot=annot)


def test_one_shot_and_pybind(annot_case):
    """9. engine.calculate(annot=) and the pybind module equal Engine.run bitwise."""
    from nldsc_amd import engine as E
    from nldsc_amd.ldscore import _ldscore as lds
    d, names, annot, exp = annot_case
    rows, pos, args, N, _ = dataset("n1001")
    M = len(rows)
    path = os.path.join(GOLDEN, "n1001.bed")
    got = E.calculate(path, M, N, *args, pos, annot=annot)
    for k in ("l2_annot", "l2d_annot") + KEYS:
        assert bitwise(got[k], exp[k]), k
    p = lds.LDScoreParams(path, n_snp=M, n_org=N, ld_wind=args[0], maf=args[1], std_thr=args[2], rsq_thr=args[3],
                          positions=pos.tolist())
    p.annot = annot.ravel().tolist()
    r = lds.calculate(p)
    for k in KEYS:
        assert bitwise(np.asarray(getattr(r, k), dtype=exp[k].dtype), exp[k]), k
    for k in ("l2_annot", "l2d_annot"):
        assert bitwise(np.asarray(getattr(r, k)).reshape(M, len(names)), np.ascontiguousarray(exp[k])), k
    p.annot = []
    assert lds.calculate(p).l2_annot == []


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _ld(args, *, ranks=1, timeout=300, ok=True):
    """The CLI, as tests/test_gpu_torchrun.py starts it (gloo: both ranks on GPU 0)."""
    env = dict(os.environ, NLDSC_DIST_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    if ranks > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "-m", "nldsc_amd", "ld"] + args
    else:
        cmd = [sys.executable, "-m", "nldsc_amd", "ld"] + args
    p = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert p.returncode == 0 and "crashed" not in p.stderr, p.stderr[-3000:]
    return p


COMMON = ["--ld-wind-cm", "1", "-maf", "0.01", "--extra", "--write-m", "--quiet"]


def test_cli(annot_case):
    """10. --annot with a full-form file and its .gz: identical tables whose existing columns are those of a run
    without --annot and whose appended columns are %.5f of the engine's values; .M unchanged, .M_annot written."""
    d, names, annot, _ = annot_case
    rows, pos, args, N, _ = dataset("n1001")
    M = len(rows)
    bfile = os.path.join(GOLDEN, "n1001")
    _ld(["--bfile", bfile, "--annot", str(d / "n1001.annot"), "--out", str(d / "a.L2")] + COMMON)
    _ld(["--bfile", bfile, "--annot", str(d / "n1001.annot.gz"), "--out", str(d / "gz.L2")] + COMMON)
    _ld(["--bfile", bfile, "--out", str(d / "plain.L2")] + COMMON)
    assert (d / "a.L2").read_bytes() == (d / "gz.L2").read_bytes()
    assert (d / "a.M").read_bytes() == (d / "plain.M").read_bytes()
    assert (d / "a.M_annot").read_bytes() == (d / "gz.M_annot").read_bytes()
    assert not (d / "plain.M_annot").exists()
    got = [ln.split("\t") for ln in (d / "a.L2").read_text().split("\n")]
    plain = [ln.split("\t") for ln in (d / "plain.L2").read_text().split("\n")]
    assert len(got) == len(plain) == M + 2 and got[-1] == [""]
    n0, C = len(plain[0]), len(names)
    assert got[0] == plain[0] + [f"L2_{n}" for n in names] + [f"L2D_{n}" for n in names]
    assert [r[:n0] for r in got[:-1]] == plain[:-1]
    # the CLI's run: rsq_thr = 1 / M, std_thr its default
    from nldsc_amd.engine import Engine
    with Engine(0) as e:
        e.load_bed_file(bfile + ".bed", M, N)
        exp = e.run(1.0, 0.01, 1e-4, 1.0 / M, pos, annot=annot)
    fmt = lambda v: "" if np.isnan(v) else "%.5f" % v  # noqa: E731
    for j in range(M):
        want = [fmt(v) for v in exp["l2_annot"][j]] + [fmt(v) for v in exp["l2d_annot"][j]]
        assert got[1 + j][n0:] == want, (j, got[1 + j][n0:], want)
    m_plain = (d / "a.M").read_text().splitlines()[1].split("\t")
    m_annot = [ln.split("\t") for ln in (d / "a.M_annot").read_text().splitlines()]
    assert m_annot[0] == ["ANNOT", "M", "MD"] and [r[0] for r in m_annot[1:]] == names
    # the all-ones row: M and MD of .M before their integer cast (printed to 5 decimals)
    assert float(m_annot[1][1]) == int(m_plain[0]) and 0 <= float(m_annot[1][2]) - int(m_plain[1]) < 1 + 1e-5


def test_cli_genome_substitutes_the_chromosome(annot_case, tmp_path):
    """a two-chromosome chr@ run substitutes '@' in --bfile and in --annot"""
    d, names, annot, _ = annot_case
    for c in ("1", "2"):
        for ext in (".bed", ".bim", ".fam"):
            shutil.copy(os.path.join(GOLDEN, "n1001" + ext), tmp_path / f"chr{c}{ext}")
    shutil.copy(d / "n1001.annot", tmp_path / "ann1.annot")
    shutil.copy(d / "n1001.annot", tmp_path / "ann2.annot")
    _ld(["--bfile", str(tmp_path / "chr@"), "--annot", str(tmp_path / "ann@.annot"), "--out",
         str(tmp_path / "out@.L2")] + COMMON)
    _ld(["--bfile", os.path.join(GOLDEN, "n1001"), "--annot", str(d / "n1001.annot"), "--out",
         str(tmp_path / "one.L2")] + COMMON)
    for c in ("1", "2"):
        assert (tmp_path / f"out{c}.L2").read_bytes() == (tmp_path / "one.L2").read_bytes()
        assert (tmp_path / f"out{c}.M_annot").read_bytes() == (tmp_path / "one.M_annot").read_bytes()


def test_cli_two_ranks_rejects_annot(annot_case, tmp_path):
    d = annot_case[0]
    p = _ld(["--bfile", os.path.join(GOLDEN, "n1001"), "--annot", str(d / "n1001.annot"), "--out",
             str(tmp_path / "two.L2")] + COMMON, ranks=2, ok=False)
    assert "NLDSCParameterError" in p.stderr and "--annot" in p.stderr and "one GPU" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "two.L2").exists()
