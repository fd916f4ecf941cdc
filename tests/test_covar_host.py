"""Host layer of --covar (no GPU): the PLINK covariate file reader, the orthonormal basis the engine takes, and the C
ABI's declarations."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

# (the package is imported inside the tests, as the other host tests do: importing it at collection time would load the
# engine library's HIP runtime before a GPU test's torch.cuda.init())


def write(tmp_path, text, name="x.covar"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


IDS = [("F1", "A"), ("F1", "B"), ("F2", "A"), ("F3", "C")]


# ---- CovarFile ------------------------------------------------------------------------------------------------------
def test_header_is_recognised_by_a_non_numeric_third_field(tmp_path):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    with_header = CovarFile(write(tmp_path, "FID IID PC1 AGE\nF1 A 0.5 30\nF1 B -1e-3 41\n"))
    assert with_header.names == ["PC1", "AGE"] and with_header.ids == [("F1", "A"), ("F1", "B")]
    without = CovarFile(write(tmp_path, "F1\tA\t0.5\t30\n\nF1  B -1e-3 41\n"))  # tabs, blank lines, runs of spaces
    assert without.names == ["COV1", "COV2"] and without.ids == [("F1", "A"), ("F1", "B")]
    m = np.array([[0.5, 30.0], [-1e-3, 41.0]])
    assert np.array_equal(with_header.matrix(IDS[:2]), m) and np.array_equal(without.matrix(IDS[:2]), m)
    # a missing value in the first row is no header
    na_first = CovarFile(write(tmp_path, "F1 A NA 30\nF1 B 2 41\n"))
    assert na_first.names == ["COV1", "COV2"] and len(na_first.ids) == 2


def test_rows_are_matched_by_fid_iid_in_fam_order(tmp_path):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    text = "F3 C 4 40\nEXTRA X NA oops\nF2 A 3 30\nF1 B 2 20\nF1 A 1 10\n"
    cf = CovarFile(write(tmp_path, text))
    assert np.array_equal(cf.matrix(IDS), np.array([[1, 10], [2, 20], [3, 30], [4, 40.0]]))
    # a subset (after --keep): the other rows, unusable values included, are ignored
    assert np.array_equal(cf.matrix([IDS[2], IDS[0]]), np.array([[3, 30], [1, 10.0]]))


def test_missing_individual(tmp_path):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    cf = CovarFile(write(tmp_path, "F1 A 1\nF2 A 3\n"))
    with pytest.raises(NLDSCParameterError, match=r"no row for individual F1 B \(\.fam line 2 .*--keep"):
        cf.matrix(IDS)


def test_duplicate_row(tmp_path):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    with pytest.raises(NLDSCParameterError, match=r"line 3: a second row for individual F1 A \(the first is line 1\)"):
        CovarFile(write(tmp_path, "F1 A 1\nF1 B 2\nF1 A 3\n"))
    with pytest.raises(NLDSCParameterError, match="duplicate covariate column name PC1"):
        CovarFile(write(tmp_path, "FID IID PC1 PC1\nF1 A 1 2\n"))


@pytest.mark.parametrize("field, what", [("NA", "is missing"), ("nan", "is missing"), ("abc", "non-numeric value 'abc'"),
                                         ("inf", "is not finite")])
def test_unusable_values_name_the_first_offender(tmp_path, field, what):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    cf = CovarFile(write(tmp_path, f"FID IID PC1 AGE\nF1 A 1 2\nF1 B 3 {field}\nF2 A {field} 5\n"))
    with pytest.raises(NLDSCParameterError) as ex:
        cf.matrix(IDS[:3])
    msg = str(ex.value)
    assert what in msg and "line 3" in msg and "AGE" in msg and "F1 B" in msg and "--keep" in msg
    assert np.array_equal(cf.matrix(IDS[:1]), [[1.0, 2.0]])  # without that individual the file is fine


def test_malformed_files(tmp_path):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    with pytest.raises(NLDSCParameterError, match="line 2: 3 fields, expected 4"):
        CovarFile(write(tmp_path, "F1 A 1 2\nF1 B 3\n"))
    with pytest.raises(NLDSCParameterError, match="fewer than three fields"):
        CovarFile(write(tmp_path, "F1 A\n"))
    with pytest.raises(NLDSCParameterError, match="empty"):
        CovarFile(write(tmp_path, "\n\n"))
    with pytest.raises(FileNotFoundError):
        CovarFile(str(tmp_path / "absent.covar"))


# ---- covar_basis ----------------------------------------------------------------------------------------------------
def check_basis(Q, N):
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    assert Q.shape[0] == N and Q.dtype == np.float64 and Q.flags.c_contiguous
    assert np.abs(Q.T @ Q - np.eye(Q.shape[1])).max(initial=0) <= 1e-12
    assert np.abs(Q.sum(axis=0)).max(initial=0) <= 1e-12


def test_basis_rank_orthonormality_and_centring():
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    rng = np.random.default_rng(1)
    N = 501
    C = rng.standard_normal((N, 5))
    Q, dropped = covar_basis(C)
    check_basis(Q, N)
    assert Q.shape[1] == 5 and dropped == []
    # the basis spans the centred columns
    Cc = C - C.mean(axis=0)
    assert np.abs(Q @ (Q.T @ Cc) - Cc).max() <= 1e-12
    # duplicated, constant, scaled and dependent columns drop out, and are named
    wide = np.concatenate([C, C[:, 1:2], np.full((N, 1), -7.0), 1e6 * C[:, 3:4], (C[:, 0] - 2 * C[:, 4])[:, None],
                           rng.standard_normal((N, 1))], axis=1)
    Qw, dropped = covar_basis(wide)
    check_basis(Qw, N)
    assert Qw.shape[1] == 6 and dropped == [5, 6, 7, 8]
    # one column, as a vector; a constant column alone leaves nothing
    q1, d1 = covar_basis(C[:, 0])
    check_basis(q1, N)
    assert q1.shape == (N, 1) and d1 == []
    q0, d0 = covar_basis(np.full((N, 2), 3.0))
    assert q0.shape == (N, 0) and d0 == [0, 1]
    with pytest.raises(NLDSCParameterError, match="not finite"):
        covar_basis(np.array([[1.0, np.nan], [0.0, 1.0], [2.0, 2.0]]))


def test_basis_is_invariant_under_column_mixing():
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    rng = np.random.default_rng(2)
    N = 400
    C = np.concatenate([rng.standard_normal((N, 3)), rng.integers(0, 2, (N, 1)).astype(float),
                        rng.uniform(18, 80, (N, 1))], axis=1)
    P = covar_basis(C)[0]
    P = P @ P.T
    for label, Cv in (("mixed", C @ rng.standard_normal((5, 5))),
                      ("scaled and shifted", 1000.0 * C + rng.uniform(-1e4, 1e4, 5)[None, :]),
                      ("permuted, with a duplicate and a constant",
                       np.concatenate([C[:, ::-1], C[:, :1], np.ones((N, 1))], axis=1))):
        Q, _ = covar_basis(Cv)
        check_basis(Q, N)
        assert Q.shape[1] == 5, label
        assert np.abs(Q @ Q.T - P).max() <= 1e-10, (label, np.abs(Q @ Q.T - P).max())


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_exported_list():
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    from nldsc_amd import _lib
    text = open(os.path.join(REPO, "include", "nldsc_ld.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nldsc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_lib.EXPORTED), (sorted(declared - set(_lib.EXPORTED)), sorted(set(_lib.EXPORTED) - declared))
    for name in ("nldsc_engine_run_covar", "nldsc_ld_calculate_covar", "nldsc_engine_covar_projections"):
        assert name in declared
    assert re.search(r"#define\s+NLDSC_MAX_COVAR\s+64\b", text) and _lib.MAX_COVAR == 64


def test_cli_has_the_covar_option():
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    from click.testing import CliRunner

    from nldsc_amd.__main__ import main
    out = CliRunner().invoke(main, ["ld", "--help"]).output
    assert "--covar FILE" in out


def test_covar_rejects_annot_and_pairs_before_any_file_is_read():
    from nldsc_amd.core.common import NLDSCParameterError  # noqa: F401
    from nldsc_amd.ldscore.common import CovarFile, covar_basis  # noqa: F401
    from nldsc_amd.ldscore.routine import reject_covar_options
    reject_covar_options(None, None)
    for annot, pairs in (("a.annot", None), (None, "p.tsv")):
        with pytest.raises(NLDSCParameterError, match="covariates with annotations or a pair table in one run are not "
                                                      "supported"):
            reject_covar_options(annot, pairs)
