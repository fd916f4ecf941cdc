"""Host side of the dominance-by-dominance LD scores (--dom-dom): the CLI flag and its combination errors, the L2DD
column of the table, the pybind fields, the C ABI's declarations, and the batch planner with the nine-tile unit size.
No GPU."""
import os
import re
import types

import numpy as np
import pytest

from conftest import REPO

M = 6
NAN = float("nan")
# the table of hand_result() as it was written before the L2DD column existed (extra False / True)
PLAIN = (b"CHR\tSNP\tBP\tL2\tL2D\n1\trs0\t1000\t1.50000\t0.50000\n1\trs1\t1010\t\t\n1\trs2\t1020\t2.25000\t0.25000\n"
         b"1\trs3\t1030\t1.00000\t\n1\trs4\t1040\t3.00000\t0.75000\n1\trs5\t1050\t1.12500\t0.12500\n")
PLAIN_EXTRA = (b"CHR\tSNP\tBP\tL2\tL2D\tMAF\tWSA\tWSD\tWSDE\tRSTD\n"
               b"1\trs0\t1000\t1.50000\t0.50000\t0.10000\t4\t4\t2\t0.50000\n"
               b"1\trs1\t1010\t\t\t0.00100\t-1\t-1\t-1\t\n"
               b"1\trs2\t1020\t2.25000\t0.25000\t0.20000\t5\t5\t5\t0.50000\n"
               b"1\trs3\t1030\t1.00000\t\t0.30000\t2\t2\t1\t0.50000\n"
               b"1\trs4\t1040\t3.00000\t0.75000\t0.40000\t4\t4\t1\t0.50000\n"
               b"1\trs5\t1050\t1.12500\t0.12500\t0.25000\t8\t8\t2\t0.50000\n")


@pytest.fixture()
def bim(tmp_path):
    from nldsc_amd.ldscore.common import BIMFile
    p = tmp_path / "x.bim"
    p.write_text("".join(f"1\trs{j}\t{0.1 * j:.2f}\t{1000 + 10 * j}\tA\tG\n" for j in range(M)))
    return BIMFile(str(p))


def hand_result():
    """a result of M SNPs: SNP 1 not computed (NaN / -1), SNP 3 with a constant dominance residual"""
    return types.SimpleNamespace(
        l2=[1.5, NAN, 2.25, 1.0, 3.0, 1.125], l2d=[0.5, NAN, 0.25, NAN, 0.75, 0.125],
        maf=[0.1, 0.001, 0.2, 0.3, 0.4, 0.25], residuals_std=[0.5, NAN, 0.5, 0.5, 0.5, 0.5],
        l2_ws=[4, -1, 5, 2, 4, 8], l2d_ws=[4, -1, 5, 2, 4, 8], l2d_wse=[2, -1, 5, 1, 1, 2],
        l2dd=[1.0123456, NAN, 0.999996, NAN, 12.5, 1.0])


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def test_cli_has_the_dom_dom_flag():
    from click.testing import CliRunner

    from nldsc_amd.__main__ import main
    out = CliRunner().invoke(main, ["ld", "--help"]).output
    assert "--dom-dom" in out and "L2DD" in out


def test_dom_dom_rejects_its_combinations_before_any_file_is_read():
    from nldsc_amd.core.common import NLDSCParameterError
    from nldsc_amd.ldscore import _ldscore
    from nldsc_amd.ldscore.genome import estimate_lds_genome
    from nldsc_amd.ldscore.routine import estimate_lds, reject_domdom_options
    reject_domdom_options(None, None, None, 0)
    reject_domdom_options(None, None, None, _ldscore.FLAG_STRICT_PLINK_ORDER)
    msg = "dom-dom scores with annotations, a pair table or covariates in one run are not supported"
    for kw in (dict(annot="a.annot"), dict(pairs_out="p.tsv"), dict(covar="c.covar")):
        args = dict(annot=None, pairs_out=None, covar=None)
        args.update(kw)
        with pytest.raises(NLDSCParameterError, match=msg):
            reject_domdom_options(args["annot"], args["pairs_out"], args["covar"], 0)
        # (the files do not exist: the error comes before anything is opened)
        with pytest.raises(NLDSCParameterError, match=msg):
            estimate_lds("nowhere/x", 1.0, "cm", dom_dom=True, **kw)
        with pytest.raises(NLDSCParameterError, match=msg):
            estimate_lds_genome("nowhere/chr@", 1.0, "cm", dom_dom=True, **kw)
    with pytest.raises(NLDSCParameterError, match="--additive-only: the dominance-by-dominance scores need the "
                                                  "dominance residuals"):
        reject_domdom_options(None, None, None, _ldscore.FLAG_ADDITIVE_ONLY)
    with pytest.raises(NLDSCParameterError, match="--additive-only"):
        estimate_lds("nowhere/x", 1.0, "cm", dom_dom=True, flags=_ldscore.FLAG_ADDITIVE_ONLY)


def test_dom_dom_is_refused_under_several_ranks_on_one_chromosome(monkeypatch):
    from nldsc_amd.core.common import NLDSCParameterError
    from nldsc_amd.ldscore.routine import reject_domdom_options
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(NLDSCParameterError, match="runs a chromosome on one GPU"):
        reject_domdom_options(None, None, None, 0)
    reject_domdom_options(None, None, None, 0, sharded_ok=True)  # whole chromosomes per rank


def test_cli_reports_the_combination_error(tmp_path, monkeypatch):
    """The command carries the flag to estimate_lds, whose parameter error ends it in the house style."""
    from click.testing import CliRunner

    from nldsc_amd import __main__ as cli
    said = []
    monkeypatch.setattr(cli.log, "critical", lambda msg, **kw: said.append(msg))
    for more, needle in ((["--additive-only"], "--dom-dom cannot be combined with --additive-only"),
                         (["--covar", "c.covar"], "--dom-dom cannot be combined with --annot, --pairs-out or --covar")):
        said.clear()
        CliRunner().invoke(cli.main, ["ld", "--bfile", str(tmp_path / "x"), "-cm", "1", "--dom-dom", "--quiet"] + more)
        assert len(said) == 1 and "NLDSCParameterError" in said[0] and needle in said[0], said


# ---- the table -------------------------------------------------------------------------------------------------------
def test_l2dd_column_position_and_format(bim, tmp_path):
    from nldsc_amd.ldscore import routine as R
    ld = hand_result()
    for extra, plain in ((False, PLAIN), (True, PLAIN_EXTRA)):
        out = tmp_path / f"t{int(extra)}.L2"
        R.write_scores(str(out), bim, ld, extra=extra, dom_dom=True)
        got = out.read_bytes().decode().split("\n")
        exp = plain.decode().split("\n")
        assert len(got) == len(exp) == M + 2 and got[-1] == ""
        assert got[0] == exp[0] + "\tL2DD"  # after every existing column
        cells = []
        for g, p in zip(got[1:-1], exp[1:-1]):
            assert g.rsplit("\t", 1)[0] == p  # every existing column in place, to the byte
            cells.append(g.rsplit("\t", 1)[1])
        assert cells == ["1.01235", "", "1.00000", "", "12.50000", "1.00000"]  # %.5f, NaN as an empty field
    df = R.domdom_output(bim, ld, extra=True)
    assert list(df.columns)[-1] == "L2DD" and list(df.columns)[:-1] == list(R.make_output(bim, ld, extra=True).columns)


def test_table_without_the_flag_is_byte_identical(bim, tmp_path):
    from nldsc_amd.ldscore import routine as R
    ld = hand_result()  # (l2dd present or not: the table does not show it without the flag)
    for extra, plain in ((False, PLAIN), (True, PLAIN_EXTRA)):
        out = tmp_path / f"p{int(extra)}.L2"
        R.write_scores(str(out), bim, ld, extra=extra, dom_dom=False)
        assert out.read_bytes() == plain
        del_ld = types.SimpleNamespace(**{k: v for k, v in vars(ld).items() if k != "l2dd"})
        R.write_scores(str(out), bim, del_ld, extra=extra)
        assert out.read_bytes() == plain
    # the h2 reader's M / MD come from the columns that were there before
    assert R.m_values(bim, ld) == R.m_values(bim, types.SimpleNamespace(**{k: v for k, v in vars(ld).items()
                                                                          if k != "l2dd"}))


def test_summary_has_one_line_for_l2dd(capsys):
    from nldsc_amd.ldscore import routine as R
    ld = hand_result()
    R.show_summary(ld)
    out = capsys.readouterr().out
    assert out.count("dominance-by-dominance non-null LD: 4") == 1
    R.show_summary(types.SimpleNamespace(**{k: v for k, v in vars(ld).items() if k != "l2dd"}))
    assert "dominance-by-dominance" not in capsys.readouterr().out


# ---- the pybind module and the C ABI ---------------------------------------------------------------------------------
def test_pybind_fields_and_stub():
    from nldsc_amd.ldscore import _ldscore
    p = _ldscore.LDScoreParams()
    assert p.dom_dom is False
    p.dom_dom = True
    assert p.dom_dom is True
    assert _ldscore.LDScoreResult().l2dd == []
    stub = open(os.path.join(REPO, "nldsc_amd", "ldscore", "_ldscore.pyi")).read()
    assert re.search(r"^\s+dom_dom: bool", stub, flags=re.M) and re.search(r"^\s+l2dd: List\[float\]", stub, flags=re.M)
    # a dom-dom request with annotations is refused before anything is read
    p.annot = [1.0]
    p.n_snp, p.positions = 1, [0.0]
    with pytest.raises(ValueError, match="dom-dom scores with annotations"):
        _ldscore.calculate(p)


def test_c_abi_declares_and_exports_the_dom_dom_entry_points():
    from nldsc_amd import _lib
    text = open(os.path.join(REPO, "include", "nldsc_ld.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nldsc_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in ("nldsc_engine_run_domdom", "nldsc_ld_calculate_domdom", "nldsc_plan_batches_unit"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name), name
    from nldsc_amd.engine import Engine
    assert callable(Engine.run_domdom)


# ---- the batch planner with the nine-tile unit -----------------------------------------------------------------------
@pytest.mark.parametrize("n_items,n_it,n_cu,want,cap", [
    (26034, 40, 256, 0, 0),           # the C3 band under the engine's 1 GiB
    (26034, 40, 256, 0, 64 << 20),    # a small cap: many batches
    (1000, 258, 256, 0, 9 << 20),     # long rows (K-split pieces), a cap of a few units
    (37, 8, 256, 5, 0),               # the batch option
    (1, 2, 256, 0, 1),                # a cap below one unit: one item per batch all the same
    (0, 8, 256, 0, 0),
])
def test_planner_with_the_nine_tile_unit(n_items, n_it, n_cu, want, cap):
    from nldsc_amd import _lib
    unit = _lib.DD_UNIT_FLOATS
    assert unit == 9 * 32 * 32
    b = _lib.plan_batches_unit(n_items, n_it, n_cu, unit, batch_items=want, cap_bytes=cap)
    cap_bytes = cap if cap > 0 else 1 << 30
    # every item exactly once, in order
    assert int(b[:, 1].sum()) == n_items and (b[:, 1] > 0).all()
    assert np.array_equal(b[:, 0], np.concatenate([[0], np.cumsum(b[:, 1])[:-1]])[:len(b)])
    for first, n, P in b:
        assert 1 <= P <= 8 and 2 * P <= max(n_it, 2)
        assert n * P * unit * 4 <= cap_bytes or n == 1  # the cap on the nine-tile size
        if want:
            assert n <= want
    # the eight-tile planner is unchanged and holds more items under the same cap
    b8 = _lib.plan_batches_unit(n_items, n_it, n_cu, 8192, batch_items=want, cap_bytes=cap)
    if cap == 0:
        assert np.array_equal(b8, _lib.annot_plan_batches(n_items, n_it, n_cu, True, want))
    if n_items > 1 and not want:
        assert b8[0, 1] >= b[0, 1]
