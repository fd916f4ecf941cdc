"""Host side of partitioned LD scores (--annot): the AnnotFile reader, the output tables, and the pure batch and
fixed-point-scale arithmetic of annotated runs (band_plan.cpp), the latter also under ASan + UBSan through the
stand-alone program tests/native/annot_plan_check.cpp.  No GPU."""
import gzip
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "nldsc_amd", "csrc")
M = 6


@pytest.fixture()
def bim(tmp_path):
    from nldsc_amd.ldscore.common import BIMFile
    p = tmp_path / "x.bim"
    p.write_text("".join(f"1\trs{j}\t{0.1 * j:.2f}\t{1000 + 10 * j}\tA\tG\n" for j in range(M)))
    return BIMFile(str(p))


def full_text(values, names=("base", "coding"), snps=None):
    snps = [f"rs{j}" for j in range(M)] if snps is None else snps
    head = "CHR\tBP\tSNP\tCM\t" + "\t".join(names) + "\n"
    return head + "".join(f"1\t{1000 + 10 * j}\t{snps[j]}\t{0.1 * j:.2f}\t" + "\t".join(map(str, values[j])) + "\n"
                          for j in range(len(values)))


VALUES = [[1, 0], [1, 1], [1, 0.5], [1, -2.25], [1, 1e3], [1, 0]]


def test_annot_file_full_thin_and_gz(bim, tmp_path):
    from nldsc_amd.ldscore.common import AnnotFile
    (tmp_path / "a.annot").write_text(full_text(VALUES))
    a = AnnotFile(str(tmp_path / "a.annot"), bim)
    assert a.names == ["base", "coding"] and a.data.dtype == np.float64 and a.data.shape == (M, 2)
    assert np.array_equal(a.data, np.asarray(VALUES, dtype=np.float64))
    assert "n_annot=2" in repr(a)
    with gzip.open(tmp_path / "a.annot.gz", "wt") as fh:
        fh.write(full_text(VALUES))
    g = AnnotFile(str(tmp_path / "a.annot.gz"), bim)
    assert g.names == a.names and np.array_equal(g.data, a.data)
    # thin form: annotation columns only, any whitespace between them
    (tmp_path / "thin.annot").write_text("base  coding\n" + "".join(f"{v[0]} \t{v[1]}\n" for v in VALUES))
    t = AnnotFile(str(tmp_path / "thin.annot"), bim)
    assert t.names == a.names and np.array_equal(t.data, a.data)
    with pytest.raises(FileNotFoundError):
        AnnotFile(str(tmp_path / "nope.annot"), bim)


def test_annot_file_rejections(bim, tmp_path):
    from nldsc_amd.ldscore.common import AnnotFile, NLDSCParameterError
    path = tmp_path / "bad.annot"

    def rejected(text, match):
        path.write_text(text)
        with pytest.raises(NLDSCParameterError, match=match):
            AnnotFile(str(path), bim)

    snps = [f"rs{j}" for j in range(M)]
    snps[3], snps[4] = snps[4], snps[3]
    rejected(full_text(VALUES, snps=snps), r"row 4: SNP rs4 where the \.bim has rs3")  # the first differing row
    rejected(full_text(VALUES[:-1]), "5 rows, but the .bim has 6")
    rejected("base\n" + "1\n" * (M + 1), "7 rows, but the .bim has 6")  # thin form: the row count must be M
    bad = [list(v) for v in VALUES]
    bad[2][1] = "yes"
    rejected(full_text(bad), "row 3: non-numeric value 'yes'")
    for word in ("nan", "inf", "-inf"):
        bad[2][1] = word
        rejected(full_text(bad), "row 3, column coding: the value is not finite")
    rejected(full_text(VALUES, names=("base", "base")), "duplicate annotation column name base")
    rejected("base coding base\n" + "1 0 1\n" * M, "duplicate annotation column name base")
    rejected("CHR\tBP\tSNP\tCM\n" + "".join(f"1\t{1000 + 10 * j}\trs{j}\t0\n" for j in range(M)), "no annotation column")
    rejected(full_text(VALUES).replace("\t0.5\n", "\n"), "row 3: 5 fields, expected 6")


def hand_result():
    """a result of M SNPs: SNP 1 not computed (NaN / -1), the others with window sizes"""
    nan = float("nan")
    ld = types.SimpleNamespace(
        l2=[1.5, nan, 2.25, 1.0, 3.0, 1.125], l2d=[0.5, nan, 0.25, nan, 0.75, 0.125],
        maf=[0.1, 0.001, 0.2, 0.3, 0.4, 0.25], residuals_std=[0.5, nan, 0.5, 0.5, 0.5, 0.5],
        l2_ws=[4, -1, 5, 2, 4, 8], l2d_ws=[4, -1, 5, 2, 4, 8], l2d_wse=[2, -1, 5, 1, 1, 2])
    annot = np.array([[1, 0], [1, 1], [1, 0.5], [1, -2.25], [1, 1e3], [1, 0]], dtype=np.float64)
    ld.l2_annot = np.array([[1.5, 0.1234567], [nan, nan], [2.25, -0.000004], [1.0, 2.0], [3.0, 1234.5], [1.125, 0]])
    ld.l2d_annot = np.array([[0.5, 0.0], [nan, nan], [0.25, 1e-7], [nan, nan], [0.75, -3.0], [0.125, 0.5]])
    return ld, annot


def test_output_table_columns_and_format(bim, tmp_path):
    from nldsc_amd.ldscore import routine as R
    ld, annot = hand_result()
    names = ["base", "coding"]
    for extra in (False, True):
        out = tmp_path / f"t{int(extra)}.L2"
        R.write_scores(str(out), bim, ld, extra=extra, annot_names=names)
        got = out.read_text().split("\n")
        plain = R.make_output(bim, ld, extra=extra).to_csv(sep="\t", index=False, float_format="%.5f").split("\n")
        n0 = len(plain[0].split("\t"))
        assert got[0].split("\t") == plain[0].split("\t") + ["L2_base", "L2_coding", "L2D_base", "L2D_coding"]
        assert len(got) == len(plain) == M + 2
        for g, p in zip(got[1:-1], plain[1:-1]):
            assert g.split("\t")[:n0] == p.split("\t")  # every existing column in place
        rows = [g.split("\t")[n0:] for g in got[1:-1]]
        assert rows[0] == ["1.50000", "0.12346", "0.50000", "0.00000"]
        assert rows[1] == ["", "", "", ""]  # NaN: empty fields
        assert rows[2] == ["2.25000", "-0.00000", "0.25000", "0.00000"]
        assert rows[3] == ["1.00000", "2.00000", "", ""]
        assert rows[4] == ["3.00000", "1234.50000", "0.75000", "-3.00000"]
    # the pybind result holds row-major lists
    flat = types.SimpleNamespace(**vars(ld))
    flat.l2_annot, flat.l2d_annot = ld.l2_annot.ravel().tolist(), ld.l2d_annot.ravel().tolist()
    assert R.annot_output(bim, flat, names).equals(R.annot_output(bim, ld, names))
    # without annotations the table is the native writer's, as before
    R.write_scores(str(tmp_path / "plain.L2"), bim, ld, extra=True)
    assert (tmp_path / "plain.L2").read_bytes() == R.format_scores(bim, ld, extra=True)


def test_m_annot_values(bim, tmp_path):
    from nldsc_amd.ldscore import routine as R
    ld, annot = hand_result()
    t = R.m_annot_values(bim, ld, annot, ["base", "coding"])
    # rows m_values keeps: no NaN in any column of the extra table -> SNPs 0, 2, 4, 5
    keep = [0, 2, 4, 5]
    ratio = np.array([2 / 4, 5 / 5, 1 / 4, 2 / 8])
    assert list(t.columns) == ["ANNOT", "M", "MD"] and list(t["ANNOT"]) == ["base", "coding"]
    assert np.allclose(t["M"], annot[keep].sum(0), rtol=0, atol=1e-12)
    assert np.allclose(t["MD"], (annot[keep] * ratio[:, None]).sum(0), rtol=0, atol=1e-12)
    m, md = R.m_values(bim, ld)
    assert int(t["M"][0]) == m == 4 and int(t["MD"][0]) == md == 2
    R.write_m_annot_file(str(tmp_path / "x.M_annot"), t)
    assert (tmp_path / "x.M_annot").read_text() == "ANNOT\tM\tMD\nbase\t4.00000\t2.00000\ncoding\t1000.50000\t250.50000\n"


def test_sharded_annot_is_rejected(monkeypatch):
    from nldsc_amd.ldscore import routine as R
    from nldsc_amd.ldscore.common import NLDSCParameterError
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NLDSCParameterError, match="--annot"):
        R.reject_sharded_annot()
    monkeypatch.setenv("WORLD_SIZE", "1")
    R.reject_sharded_annot()


def test_scale_exponent():
    from nldsc_amd import _lib
    for max_abs, e in ((0, 0), (1, 0), (1.5, 1), (2, 1), (1000, 10), (1e-3, 0)):
        assert _lib.annot_scale_exp(max_abs) == e, max_abs
    assert _lib.annot_scale_exp(np.nextafter(4.0, 5.0)) == 3 and _lib.annot_scale_exp(4.0) == 2


def test_batches():
    from nldsc_amd import _lib
    cap_items = (1 << 30) // (8 * 32768)  # what 1 GiB of Gram scratch holds at the largest K-split
    assert len(_lib.annot_plan_batches(0, 64, 256)) == 0
    b = _lib.annot_plan_batches(100, 64, 256, batch_items=7)
    assert b[:, 1].tolist() == [7] * 14 + [2] and b[:, 0].tolist() == list(range(0, 100, 7))  # a ragged last batch
    assert _lib.annot_plan_batches(5, 64, 256, batch_items=1)[:, :2].tolist() == [[k, 1] for k in range(5)]
    b = _lib.annot_plan_batches(3 * cap_items + 5, 2466, 256)
    assert b[:, 1].tolist() == [cap_items] * 3 + [5]
    for first, n, p in b.tolist():
        assert 1 <= p <= 8 and n * p * 32768 <= 1 << 30
    assert (_lib.annot_plan_batches(3300, 2466, 256, ksplit_ok=False)[:, 2] == 1).all()
    assert _lib.annot_plan_batches(3300, 2466, 256)[0, 2] > 1  # a rank's shard: the K-split fills the wave slots
    assert (_lib.annot_plan_batches(40, 2, 256)[:, 2] == 1).all()  # 2 P <= n_it
    with pytest.raises(ValueError):
        _lib.annot_plan_batches(10, 1, 256)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_annot_plan_under_asan_ubsan():
    subprocess.run(["make", "-s", "-C", CSRC, "sanitize-annot"], check=True, capture_output=True, timeout=600)
    exe = os.path.join(CSRC, "build", "annot_plan_check_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-4000:]
    assert "annot_plan_check OK" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
