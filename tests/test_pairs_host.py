"""Host side of the pairwise LD table (--pairs-out): the owned ranges of a pair budget, the cell geometry of the dense
count matrix, the table writer, the CLI's rejections, and the .L2 output left alone.  No GPU."""
import gzip
import io

import numpy as np
import pandas as pd
import pytest

from oracle import oracle as O


def test_split_ranges():
    from nldsc_amd._lib import pairs_split_ranges
    assert pairs_split_ranges([0], 10) == []
    assert pairs_split_ranges([0, 3, 3, 10, 11, 30], 10) == [(0, 3), (3, 4), (4, 5)]
    assert pairs_split_ranges([0, 0, 0], 0) == [(0, 2)]
    assert pairs_split_ranges([0, 5], 0) == [(0, 1)]
    rng = np.random.default_rng(1)
    for budget in (0, 1, 7, 50, 10_000):
        lens = rng.integers(0, 40, size=500) * (rng.random(500) < 0.7)
        row_ptr = np.concatenate([[0], np.cumsum(lens)])
        ranges = pairs_split_ranges(row_ptr, budget)
        assert ranges[0][0] == 0 and ranges[-1][1] == 500
        assert all(a[1] == b[0] for a, b in zip(ranges[:-1], ranges[1:])) and all(lo < hi for lo, hi in ranges)
        for lo, hi in ranges:
            n = row_ptr[hi] - row_ptr[lo]
            assert n <= budget or hi == lo + 1, "only a single row may exceed the budget"
            if hi < 500:  # greedy: the next row would not have fitted
                assert row_ptr[hi + 1] - row_ptr[lo] > budget
    with pytest.raises(ValueError):
        pairs_split_ranges([0, 5, 3], 10)


def test_cell_geometry():
    """pairs_cell / pairs_window_blocks against a quadratic restatement: on a replayed window set every (SNP, block
    holding a neighbour) has a cell, the cells of a row ascend with the block, no two pairs of (SNP, block) share one,
    and everything outside is -1."""
    from nldsc_amd._lib import pairs_cell, pairs_window_blocks
    rng = np.random.default_rng(2)
    M = 700
    pos = np.cumsum(rng.exponential(1.0, M))
    pos[300:420] = pos[300]
    passed = rng.random(M) < 0.8
    L, R = O.replay_windows(pos, passed, 40.0)
    nblk = (M + 31) // 32
    for own in ((0, M), (100, 333), (5, 6), (650, M)):
        wb = pairs_window_blocks(L, R, own)
        exp_wb = max([R[g] // 32 - L[g] // 32 + 1 for g in range(*own) if L[g] >= 0], default=1)
        assert wb == max(1, exp_wb)
        seen = {}
        for g in range(M):
            for nb in range(nblk):
                c = pairs_cell(g, nb, own, L[g], wb)
                inside = own[0] <= g < own[1] and L[g] >= 0 and 0 <= nb - L[g] // 32 < wb
                assert (c >= 0) == inside
                if inside:
                    assert c == (g - own[0]) * wb + nb - L[g] // 32 and 0 <= c < (own[1] - own[0]) * wb
                    assert seen.setdefault(c, (g, nb)) == (g, nb)
            if own[0] <= g < own[1] and L[g] >= 0:  # every neighbour's block has a cell
                for k in range(L[g], R[g] + 1):
                    assert pairs_cell(g, k // 32, own, L[g], wb) >= 0


class _Bim:
    def __init__(self, n, chrom=7):
        self.chr = pd.Series([chrom] * n)
        self.snp = pd.Series([f"rs{100 + i}" for i in range(n)])
        self.bp = pd.Series([1000 + 10 * i for i in range(n)])


TABLE = dict(row_ptr=np.array([0, 2, 2, 3]), k=np.array([3, 4, 2], np.int32),
             r=np.array([0.5, -0.25, 1.0 / 3.0]), rd=np.array([np.nan, 0.125, -0.0000004]))


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_writer(tmp_path, suffix):
    from nldsc_amd.ldscore.common import r2_adjusted
    from nldsc_amd.ldscore.routine import PAIRS_HEADER, open_pairs, write_pairs
    path = str(tmp_path / ("t.pairs" + suffix))
    N = 1001
    with open_pairs(path) as fh:
        assert write_pairs(fh, _Bim(6), TABLE, 1, N) == 3
        assert write_pairs(fh, _Bim(6), dict(row_ptr=np.array([0, 0]), k=np.zeros(0, np.int32), r=np.zeros(0),
                                            rd=np.zeros(0)), 4, N) == 0
    raw = open(path, "rb").read()
    text = (gzip.decompress(raw) if suffix else raw).decode()
    assert (raw[:2] == b"\x1f\x8b") == bool(suffix)
    lines = text.split("\n")
    assert lines[0].split("\t") == list(PAIRS_HEADER) == ["CHR", "SNP_A", "BP_A", "SNP_B", "BP_B", "R", "R2", "RD", "R2D"]
    q = (N - 1.0) / (N - 2.0)
    r2 = [1.0 - (1.0 - r * r) * q for r in TABLE["r"]]
    assert lines[1] == f"7\trs101\t1010\trs103\t1030\t0.500000\t{r2[0]:.6f}\t\t"
    assert lines[2] == f"7\trs101\t1010\trs104\t1040\t-0.250000\t{r2[1]:.6f}\t0.125000\t{1.0 - (1.0 - 0.125 ** 2) * q:.6f}"
    assert lines[3].startswith("7\trs103\t1030\trs102\t1020\t0.333333\t") and lines[3].split("\t")[7] == "-0.000000"
    assert lines[4:] == [""]
    back = pd.read_csv(io.StringIO(text), sep="\t")
    assert np.allclose(back["R2"], r2_adjusted(TABLE["r"], N), atol=5e-7)
    assert np.isnan(back["RD"][0]) and np.isnan(back["R2D"][0])
    assert r2_adjusted(0.5, 1001) == 1.0 - (1.0 - 0.25) * (1000.0 / 999.0)


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    from nldsc_amd import synth
    d = tmp_path_factory.mktemp("pairs_genome")
    for i, (c, m) in enumerate({"1": 120, "2": 60}.items()):
        synth.write_plink(str(d / f"chr{c}"), synth.SynthSpec(n_org=257, n_snp=m, length_cm=m / 60, seed=70 + i),
                          chrom=int(c))
    (d / "chr1.annot").write_text("A\n" + "1\n" * 120)
    (d / "chr2.annot").write_text("A\n" + "1\n" * 60)
    return d


def test_rejections(genome, monkeypatch):
    from nldsc_amd.core.common import NLDSCParameterError
    from nldsc_amd.ldscore.genome import estimate_lds_genome
    from nldsc_amd.ldscore.routine import estimate_lds
    d = genome
    kw = dict(maf_thr="0.01", std_thr=1e-5)
    with pytest.raises(NLDSCParameterError, match="--pairs-out and --annot"):
        estimate_lds(str(d / "chr1"), "1", "cm", annot=str(d / "chr1.annot"), pairs_out=str(d / "p.tsv"), **kw)
    with pytest.raises(NLDSCParameterError, match="--pairs-out and --annot"):
        estimate_lds_genome(str(d / "chr@"), "1", "cm", annot=str(d / "chr@.annot"), pairs_out=str(d / "p@.tsv"), **kw)
    with pytest.raises(NLDSCParameterError, match="'@' in --pairs-out"):
        estimate_lds_genome(str(d / "chr@"), "1", "cm", pairs_out=str(d / "p.tsv"), runner=lambda *a, **k: None, **kw)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NLDSCParameterError, match="one GPU"):
        estimate_lds(str(d / "chr1"), "1", "cm", pairs_out=str(d / "p.tsv"), **kw)
    with pytest.raises(NLDSCParameterError, match="one GPU"):
        estimate_lds_genome(str(d / "chr@"), "1", "cm", pairs_out=str(d / "p@.tsv"), rank=0, world=2, **kw)


def test_cli_options():
    from click.testing import CliRunner
    from nldsc_amd.__main__ import main
    out = CliRunner().invoke(main, ["ld", "--help"]).output
    assert "--pairs-out" in out and "--pairs-min-r2" in out


def test_l2_bytes_unchanged(genome, tmp_path):
    """Through a fake runner: the .L2 files are the same bytes with and without --pairs-out, and the runner is
    handed each chromosome's pair-table path, .bim, filter and budget."""
    from nldsc_amd.ldscore.genome import estimate_lds_genome
    from nldsc_amd.ldscore.routine import PAIRS_BUDGET, open_pairs, write_pairs
    d = genome
    asked = []

    def runner(bed, n_snp, n_org, w, maf, std_thr, rsq, pos, flags, pairs=None):
        res = O.run_c(bed.tobytes(), n_snp, n_org, w, maf, std_thr, rsq, pos, threads=1)
        if pairs is not None:
            asked.append(pairs)
            with open_pairs(pairs["path"]) as fh:
                write_pairs(fh, pairs["bim"], dict(row_ptr=np.array([0, 1] + [1] * (n_snp - 1)),
                                                   k=np.array([1], np.int32), r=np.array([0.1]),
                                                   rd=np.array([np.nan])), 0, n_org)
        return res, {}

    kw = dict(maf_thr="0.01", std_thr=1e-5, extra=True, runner=runner, rank=0, world=1)
    estimate_lds_genome(str(d / "chr@"), "1", "cm", out=str(tmp_path / "a@.L2"), **kw)
    estimate_lds_genome(str(d / "chr@"), "1", "cm", out=str(tmp_path / "b@.L2"), pairs_out=str(tmp_path / "p@.tsv.gz"),
                        pairs_min_r2=0.2, **kw)
    for c in ("1", "2"):
        assert (tmp_path / f"a{c}.L2").read_bytes() == (tmp_path / f"b{c}.L2").read_bytes()
        assert gzip.open(tmp_path / f"p{c}.tsv.gz", "rt").readline().startswith("CHR\tSNP_A")
    assert [p["path"] for p in asked] == [str(tmp_path / f"p{c}.tsv.gz") for c in ("1", "2")]
    assert all(p["min_r2"] == 0.2 and p["budget"] == PAIRS_BUDGET and p["bim"].n_snp in (120, 60) for p in asked)


class _FakeEngine:
    """Engine.size_pairs / Engine._pairs over a hand-made full table (row j: up to 3 neighbours after j)."""

    def __init__(self, n, n_org=1001):
        self.n_snp, self.n_org, self.calls = n, n_org, []
        lens = np.array([min(3, n - 1 - j) * (j % 5 != 4) for j in range(n)])
        self.row_ptr = np.concatenate([[0], np.cumsum(lens)])
        self.k = np.concatenate([np.arange(j + 1, j + 1 + m) for j, m in enumerate(lens)]).astype(np.int32)
        self.r = np.cos(np.arange(len(self.k)))
        self.rd = np.where(np.arange(len(self.k)) % 3 == 0, np.nan, np.sin(np.arange(len(self.k))))

    def _res(self, own):
        res = dict(l2=np.full(self.n_snp, np.nan), l2d=np.full(self.n_snp, np.nan), maf=np.full(self.n_snp, np.nan),
                   residuals_std=np.full(self.n_snp, np.nan), l2_ws=np.full(self.n_snp, -1, np.int32),
                   l2d_ws=np.full(self.n_snp, -1, np.int32), l2d_wse=np.full(self.n_snp, -1, np.int32))
        for key in res:
            res[key][own[0]:own[1]] = np.arange(own[0], own[1])
        return res

    def size_pairs(self, *args, own, flags, min_r2):
        self.calls.append(("size", own))
        a = self.row_ptr[own[0]]
        return dict(self._res(own), row_ptr=self.row_ptr[own[0]:own[1] + 1] - a,
                    n_pairs=int(self.row_ptr[own[1]] - a))

    def _pairs(self, ld_wind, maf, std_thr, rsq_thr, positions, own, flags, min_r2, emit, cap=None):
        self.calls.append(("emit", own, cap))
        a, b = self.row_ptr[own[0]], self.row_ptr[own[1]]
        assert emit and cap == b - a
        return dict(self._res(own), row_ptr=self.row_ptr[own[0]:own[1] + 1] - a, k=self.k[a:b], r=self.r[a:b],
                    rd=self.rd[a:b], n_pairs=int(b - a))


def test_run_pairs_to_file_chunks(tmp_path):
    """The chunked run on a fake engine: sizing calls of size_snps SNPs tile the chromosome, the emitting calls are
    the owned ranges of the budget, the file holds the whole table in order and the result arrays are assembled."""
    from nldsc_amd.ldscore.routine import run_pairs_to_file
    n = 103
    eng = _FakeEngine(n)
    path = str(tmp_path / "p.tsv")
    res = run_pairs_to_file(eng, 1.0, 0.01, 1e-5, 0.01, np.arange(n, dtype=np.float64), 0, path=path, bim=_Bim(n),
                            min_r2=None, budget=25, size_snps=40)
    assert [c[1] for c in eng.calls if c[0] == "size"] == [(0, 40), (40, 80), (80, 103)]
    emits = [c for c in eng.calls if c[0] == "emit"]
    assert emits[0][1][0] == 0 and emits[-1][1][1] == n and len(emits) > 5
    assert all(a[1][1] == b[1][0] for a, b in zip(emits[:-1], emits[1:])) and all(c[2] <= 25 for c in emits)
    for key in ("l2", "l2_ws"):
        assert np.array_equal(res[key], np.arange(n))
    df = pd.read_csv(path, sep="\t")
    assert len(df) == len(eng.k)
    assert np.array_equal(df["SNP_B"].str[2:].astype(int) - 100, eng.k)
    assert np.allclose(df["R"], eng.r, atol=5.1e-7) and np.array_equal(df["RD"].isna(), np.isnan(eng.rd))
