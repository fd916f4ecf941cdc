"""Input / parameter model of `nldsc ld` (the validation contract of nldsc/ldscore/common.py:10-182).

The reference's public names, validation rules and messages, written table-driven:
  LDWindow               kb -> bp x 1000; > 0; <= 5 Mbp or <= 100 cM
  PLINKFile.parse        prefix or one of the three paths -> (BEDFile, BIMFile, FAMFile)
  BIMFile / FAMFile      tab-separated tables, one chromosome per .bim; n_snp / n_org = number of lines
  read_id_file, kept_individuals   --keep / --remove lists (FID IID per line) -> .fam line numbers (no reference
                         counterpart: PLINK's / LDSC's flags of the same names)
  AnnotFile              LDSC's .annot / .annot.gz (partitioned LD scores, --annot): names + an [M, C] float64 matrix
  r2_adjusted            the adjusted r-squared of a correlation, in the engine's fp64 expression (--pairs-out)
  CovarFile, covar_basis PLINK's covariate file (--covar) and the orthonormal basis of its columns the engine takes
  MAF, ResidualsSTDThreshold, RSQThreshold: [0, 1), [0, 1), [0, 0.1)
(RSQThreshold's repr says `std_thr=`, as the reference's does.)
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import pandas as pd

from ..core.common import Data, NLDSCParameterError
from ..core.logger import log

__all__ = ["LDWindow", "PLINKFile", "BEDFile", "BIMFile", "FAMFile", "MAF", "ResidualsSTDThreshold",
           "RSQThreshold", "NLDSCParameterError", "read_id_file", "kept_individuals", "AnnotFile", "r2_adjusted",
           "CovarFile", "covar_basis"]

# window metric -> (largest window, how the message names it)
_WINDOW_LIMITS = {"bp": (5 * 10 ** 6, "5 Mbp"), "cm": (100, "100 cm")}


class LDWindow(Data):
    def __init__(self, ld_wind: float, metric: str = "bp"):
        scale = 1000 if metric == "kbp" else 1  # kilobases are carried as base pairs
        self._data = float(ld_wind) * scale
        self._metric = "bp" if metric == "kbp" else metric
        self._validate()

    @property
    def metric(self) -> str:
        return self._metric

    def __repr__(self) -> str:
        return f"LDWindow(ld_wind={self._data}, metric='{self._metric}')"

    def _validate(self):
        limit = _WINDOW_LIMITS.get(self._metric)
        if limit is None:
            raise NLDSCParameterError("Invalid metric")
        if self._data <= 0:
            raise NLDSCParameterError("The ld-window must be greater than 0")
        if self._data > limit[0]:
            raise NLDSCParameterError(f"The ld-window cannot be larger than {limit[1]}")


class PLINKFile(Data):
    """One file of a PLINK 1 binary set; a table file keeps its columns in `_data`."""
    EXT = ""
    COLUMNS: tuple = ()

    def __init__(self, path: str):
        self._path = str(path)
        if not os.path.exists(self._path):
            raise FileNotFoundError(f'No such file: "{self._path}"')
        if self.COLUMNS:
            self._data = pd.read_csv(self._path, sep="\t", names=self.COLUMNS)
        self._validate()

    def _validate(self):
        pass

    def __repr__(self):
        return f"{type(self).__name__}(path='{self._path}')"

    @staticmethod
    def parse(bfile: str):
        """`bfile` is a prefix or the path of one of the three files -> (BEDFile, BIMFile, FAMFile)."""
        path = Path(bfile).resolve()
        if path.suffix in (".bed", ".bim", ".fam"):
            path = path.with_suffix("")
        elif path.is_dir():
            raise NotImplementedError("")
        return tuple(kind(path.as_posix() + kind.EXT) for kind in (BEDFile, BIMFile, FAMFile))


def _column(name: str):
    return property(lambda self: self._data[name])


class BEDFile(PLINKFile):
    EXT = ".bed"

    def __init__(self, path: str):
        super().__init__(path)
        self._data = path  # the engine reads the file itself


class BIMFile(PLINKFile):
    EXT = ".bim"
    COLUMNS = ("CHR", "SNP", "CM", "BP", "A1", "A2")
    chr, snp, cm, bp = (_column(c) for c in ("CHR", "SNP", "CM", "BP"))

    def __init__(self, path: str, **kwargs):
        super().__init__(path)

    @property
    def n_snp(self) -> int:
        return len(self._data)

    def __repr__(self):
        return f"BIMFile(n_snp={self.n_snp})"

    def _validate(self):
        if self._data["CHR"].nunique(dropna=False) != 1:
            raise NLDSCParameterError("The current version of the program "
                                      "can only work with one chromosome in one file.")


class FAMFile(PLINKFile):
    """The number of individuals is counted from the lines (the rows pandas would parse: non-blank
    lines; a whole-genome run reads 22 copies of a 315 599-line file, ~0.15 s each through pandas); the table is
    parsed when `data` is first asked for, and the (FID, IID) pairs of the lines (--keep / --remove) when `ids` is."""
    EXT = ".fam"
    COLUMNS = ("FID", "IID", "FATHER", "MOTHER", "SEX", "TRAIT")

    def __init__(self, path: str):
        self._path = str(path)
        if not os.path.exists(self._path):
            raise FileNotFoundError(f'No such file: "{self._path}"')
        with open(self._path, "rb") as fh:
            # \n, \r\n and lone \r all end a row for pandas' C parser, which skips lines that are empty or hold
            # only spaces (an empty file is 0 rows, as the reference's read_csv with `names` gives)
            self._n_org = sum(1 for line in fh.read().splitlines() if line.strip(b" "))
        self._table = None
        self._ids = None

    @property
    def ids(self) -> list:
        """(FID, IID) of every line, in file order: line s is individual s of every .bed row (PLINK: fields
        separated by tabs or spaces)."""
        if self._ids is None:
            ids = []
            with open(self._path, "rb") as fh:
                for line in fh.read().splitlines():
                    if not line.strip(b" "):
                        continue
                    f = line.split()
                    if len(f) < 2:
                        raise NLDSCParameterError(f'"{self._path}": a line with fewer than two fields (FID IID)')
                    ids.append((f[0].decode(errors="replace"), f[1].decode(errors="replace")))
            self._ids = ids
        return self._ids

    @property
    def data(self) -> pd.DataFrame:
        if self._table is None:
            self._table = pd.read_csv(self._path, sep="\t", names=self.COLUMNS)
        return self._table

    @property
    def n_org(self) -> int:
        return self._n_org

    def __repr__(self):
        return f"FAMFile(n_org={self.n_org})"


class AnnotFile(Data):
    """LDSC's annotation file (`.annot`, or `.annot.gz`): whitespace-delimited with a header line.  The full form
    leads with the columns CHR BP SNP CM and its SNP column must equal the .bim's, row for row; the thin form holds
    annotation columns only and must have one row per .bim SNP.  `names`: the annotation columns' names (no
    duplicates); `data`: their values, an [M, C] float64 matrix, every one numeric and finite."""
    LEAD = ("CHR", "BP", "SNP", "CM")

    def __init__(self, path: str, bim: BIMFile):
        import gzip
        self._path = str(path)
        if not os.path.exists(self._path):
            raise FileNotFoundError(f'No such file: "{self._path}"')
        opener = gzip.open if self._path.endswith(".gz") else open
        with opener(self._path, "rt") as fh:
            header = fh.readline().split()
            rows = [f for f in (line.split() for line in fh) if f]
        self._full = tuple(header[:4]) == self.LEAD
        self._names = header[4:] if self._full else header
        self._rows, self._bim = rows, bim
        self._validate()
        del self._rows, self._bim

    @property
    def names(self) -> list:
        return list(self._names)

    def __repr__(self):
        return f"AnnotFile(path='{self._path}', n_annot={len(self._names)})"

    def _validate(self):
        where = f'"{self._path}"'
        if not self._names:
            raise NLDSCParameterError(f"{where}: no annotation column")
        dup = sorted({n for n in self._names if self._names.count(n) > 1})
        if dup:
            raise NLDSCParameterError(f"{where}: duplicate annotation column name {dup[0]}")
        lead = 4 if self._full else 0
        width = lead + len(self._names)
        m = self._bim.n_snp
        if len(self._rows) != m:
            raise NLDSCParameterError(f"{where}: {len(self._rows)} rows, but the .bim has {m} SNPs")
        for k, f in enumerate(self._rows):
            if len(f) != width:
                raise NLDSCParameterError(f"{where}, row {k + 1}: {len(f)} fields, expected {width}")
        if self._full:
            snp = [str(s) for s in self._bim.snp.tolist()]
            for k, f in enumerate(self._rows):
                if f[2] != snp[k]:
                    raise NLDSCParameterError(f"{where}, row {k + 1}: SNP {f[2]} where the .bim has {snp[k]}: the "
                                              f"annotation rows must be the .bim's, in its order")
        data = np.empty((m, len(self._names)), dtype=np.float64)
        for k, f in enumerate(self._rows):
            try:
                data[k] = [float(v) for v in f[lead:]]
            except ValueError:
                bad = next(v for v in f[lead:] if not _is_number(v))
                raise NLDSCParameterError(f"{where}, row {k + 1}: non-numeric value {bad!r}") from None
        bad = np.argwhere(~np.isfinite(data))
        if len(bad):
            k, c = bad[0]
            raise NLDSCParameterError(f"{where}, row {k + 1}, column {self._names[c]}: the value is not finite")
        self._data = data


class CovarFile(Data):
    """PLINK's covariate file (--covar): whitespace-separated `FID IID c1 c2 ...`, one individual per line.  A first
    line whose third field is not a number (nor NA) is a header naming the columns; without one they are COV1, COV2,
    ...  `names`: the covariate columns' names; `ids`: the (FID, IID) of every row; `matrix(ids)`: the rows of the
    given individuals, in their order, as an [n, c] float64 matrix.  A duplicate (FID, IID) is an error when the file
    is read; the values are checked for the rows a run uses (rows of other individuals are ignored, so individuals
    with missing covariates can be left out with --keep / --remove)."""
    MISSING = ("NA", "NAN", "N/A", ".")

    def __init__(self, path: str):
        self._path = str(path)
        if not os.path.exists(self._path):
            raise FileNotFoundError(f'No such file: "{self._path}"')
        with open(self._path, "rt") as fh:
            self._lines = [(n, f) for n, f in ((n, line.split()) for n, line in enumerate(fh, 1)) if f]
        self._validate()
        del self._lines
        self._data = self._path

    def _validate(self):
        rows, where = self._lines, f'"{self._path}"'
        if not rows:
            raise NLDSCParameterError(f"{where}: the covariate file is empty")
        for n, f in rows:
            if len(f) < 3:
                raise NLDSCParameterError(f'{where}, line {n}: expected "FID IID c1 ...", got fewer than three fields')
        first = rows[0][1]
        header = not (_is_number(first[2]) or first[2].upper() in self.MISSING)
        width = len(first)
        self._names = first[2:] if header else [f"COV{k + 1}" for k in range(width - 2)]
        if header:
            rows = rows[1:]
            dup = sorted({n for n in self._names if self._names.count(n) > 1})
            if dup:
                raise NLDSCParameterError(f"{where}: duplicate covariate column name {dup[0]}")
        self._rows = {}
        for n, f in rows:
            if len(f) != width:
                raise NLDSCParameterError(f"{where}, line {n}: {len(f)} fields, expected {width}")
            key = (f[0], f[1])
            if key in self._rows:
                raise NLDSCParameterError(f"{where}, line {n}: a second row for individual {f[0]} {f[1]} (the first "
                                          f"is line {self._rows[key][0]})")
            self._rows[key] = (n, f[2:])

    @property
    def names(self) -> list:
        return list(self._names)

    @property
    def ids(self) -> list:
        return list(self._rows)

    def __repr__(self):
        return f"CovarFile(path='{self._path}', n_covar={len(self._names)}, rows={len(self._rows)})"

    def matrix(self, ids) -> np.ndarray:
        """The covariates of the individuals `ids` ((FID, IID) pairs: the .fam lines a run uses), row k = ids[k].
        Every one of them needs a row whose values are all numeric and finite; the error names the first that does
        not and advises --keep."""
        where = f'"{self._path}"'
        advice = "give every individual of the run a complete row, or leave such individuals out with --keep / --remove"
        out = np.empty((len(ids), len(self._names)), dtype=np.float64)
        for k, key in enumerate(ids):
            row = self._rows.get(tuple(key))
            if row is None:
                raise NLDSCParameterError(f"{where}: no row for individual {key[0]} {key[1]} (.fam line {k + 1} of "
                                          f"the run's individuals): {advice}")
            n, fields = row
            for c, text in enumerate(fields):
                if text.upper() in self.MISSING:
                    raise NLDSCParameterError(f"{where}, line {n}: covariate {self._names[c]} of individual {key[0]} "
                                              f"{key[1]} is missing ({text}): {advice}")
                if not _is_number(text):
                    raise NLDSCParameterError(f"{where}, line {n}: non-numeric value {text!r} for covariate "
                                              f"{self._names[c]} of individual {key[0]} {key[1]}: {advice}")
                value = float(text)
                if not np.isfinite(value):
                    raise NLDSCParameterError(f"{where}, line {n}: covariate {self._names[c]} of individual {key[0]} "
                                              f"{key[1]} is not finite ({text}): {advice}")
                out[k, c] = value
        return out


def covar_basis(covar, tol: float = 1e-10):
    """The orthonormal basis the engine takes for a covariate matrix `covar` ([N, c]; a 1-D array is one column):
    every column centred and scaled to unit norm (a constant column becomes 0), then the left singular vectors whose
    singular value exceeds `tol` times the largest.  Returns (Q [N, q] float64, dropped): q is the numerical rank of
    the centred matrix, Q's columns sum to 0, and `dropped` lists the indices of the columns that add nothing to the
    columns before them (constant, or linearly dependent on them) — len(dropped) == c - q whenever the two rank
    decisions agree (they are taken at the same tolerance).  Q depends on the covariates' column space only: scaling
    columns, adding constants or mixing them by an invertible matrix gives a basis of the same space."""
    c = np.asarray(covar, dtype=np.float64)
    if c.ndim == 1:
        c = c[:, None]
    if c.ndim != 2:
        raise ValueError(f"covar must be an [N, c] matrix, got shape {c.shape}")
    if not np.isfinite(c).all():
        raise NLDSCParameterError("a covariate value is not finite")
    n, k = c.shape
    scale = np.abs(c).max(axis=0) if n else np.zeros(k)
    c = c - c.mean(axis=0)
    c = c - c.mean(axis=0)  # (the first mean's rounding, large against a column with a big constant added)
    norm = np.sqrt((c * c).sum(axis=0))
    # a constant column is 0 after centring up to the rounding of its mean: at most ~N eps |x|
    live = norm > 64 * n * np.finfo(np.float64).eps * np.maximum(scale, np.finfo(np.float64).tiny)
    c = np.where(live, c / np.where(live, norm, 1.0), 0.0)
    if k == 0 or not live.any():
        return np.zeros((n, 0)), list(range(k))
    u, s, _ = np.linalg.svd(c, full_matrices=False)
    q = u[:, : int((s > tol * s[0]).sum())]
    q = q - q.mean(axis=0)  # (sums of ~1e-16 sqrt(N): exactly centred to the last rounding)
    # which columns drop out: those the columns before them already span (Gram-Schmidt, twice for orthogonality)
    dropped, basis = [], np.zeros((n, 0))
    for j in range(k):
        r = c[:, j]
        if live[j]:
            for _ in range(2):
                r = r - basis @ (basis.T @ r)
        rn = float(np.sqrt(r @ r))
        if not live[j] or rn <= tol:
            dropped.append(j)
        else:
            basis = np.concatenate([basis, (r / rn)[:, None]], axis=1)
    return np.ascontiguousarray(q), dropped


def _is_number(text: str) -> bool:
    try:
        float(text)
        return True
    except ValueError:
        return False


def _threshold(name: str, field: str, hi: float, message: str):
    """A validated threshold in [0, hi) whose repr is `name(field=value)`."""
    def __init__(self, value: float):
        self._data = float(value)
        self._validate()

    def _validate(self):
        if not (0 <= self._data < hi):
            raise NLDSCParameterError(message)

    return type(name, (Data,), {"__init__": __init__, "_validate": _validate,
                                "__repr__": lambda self: f"{name}({field}={self._data})",
                                "__module__": __name__})


MAF = _threshold("MAF", "maf", 1.0, "Minor allele frequency must be between 0 and 1!")
ResidualsSTDThreshold = _threshold("ResidualsSTDThreshold", "std_thr", 1.0,
                                   "standard deviation threshold must be between 0 and 1!")
RSQThreshold = _threshold("RSQThreshold", "std_thr", 0.1, "r-squared threshold must be between 0 and 0.1!")


def r2_adjusted(corr, n_org):
    """1 - (1 - corr^2) (N - 1) / (N - 2) as the engine's pair epilogue forms it in fp64 (ld_kernels.hip R2Adj: the
    factor (N - 1) / (N - 2) hoisted), for a correlation or an array of them; NaN stays NaN."""
    c = np.asarray(corr, dtype=np.float64)
    n = float(n_org)
    return 1.0 - (1.0 - c * c) * ((n - 1.0) / (n - 2.0))


def read_id_file(path: str) -> list:
    """The (FID, IID) pairs of a --keep / --remove file: whitespace-separated `FID IID` per line, further columns
    ignored, blank lines skipped; a line with fewer than two fields is an error."""
    if not os.path.exists(str(path)):
        raise FileNotFoundError(f'No such file: "{path}"')
    ids = []
    with open(str(path), "rb") as fh:
        for n, line in enumerate(fh.read().splitlines(), 1):
            f = line.split()
            if not f:
                continue
            if len(f) < 2:
                raise NLDSCParameterError(f'"{path}", line {n}: expected "FID IID", got fewer than two fields')
            ids.append((f[0].decode(errors="replace"), f[1].decode(errors="replace")))
    return ids


def kept_individuals(fam: FAMFile, keep: str | None = None, remove: str | None = None):
    """The individuals a run uses, as ascending 0-based .fam line numbers (int32 array), or None for everyone (no
    file given): the .fam lines named in the `keep` file (everyone without one) minus those named in the `remove`
    file.  The order is the .fam's; duplicates collapse (in the lists, and every .fam line with a listed ID counts);
    IDs that are not in the .fam are counted in one warning per file.  An empty result is an error."""
    if keep is None and remove is None:
        return None
    fam_ids = fam.ids
    known = set(fam_ids)
    lists = {}
    for what, path in (("--keep", keep), ("--remove", remove)):
        if path is None:
            continue
        ids = set(read_id_file(path))
        unknown = len(ids - known)
        if unknown:
            log.warning(f"{what} {path}: {unknown} of {len(ids)} IDs are not in {fam._path}")
        lists[what] = ids
    keep_ids, remove_ids = lists.get("--keep"), lists.get("--remove", set())
    idx = np.fromiter((s for s, i in enumerate(fam_ids)
                       if (keep_ids is None or i in keep_ids) and i not in remove_ids), dtype=np.int32)
    if idx.size == 0:
        raise NLDSCParameterError("--keep / --remove leave no individual")
    return idx
