"""`estimate_lds` — the caller of the hot path (behaviour of nldsc/ldscore/routine.py:15-102).

Parses .bed/.bim/.fam, validates parameters, builds `_ldscore.LDScoreParams`, runs
`_ldscore.calculate` on the GPU, optionally prints the summary, and writes the TSV
`CHR SNP BP L2 L2D [MAF WSA WSD WSDE RSTD] [L2DD]` (tab-separated, `%.5f`, NaN as empty field)
to `out`.  Additions: `write_m` writes the `M`/`MD` file the h2 reader looks for
(nldsc/h2/common.py:115-132,142-144) with exactly the values its fallback would compute.
"""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import pandas as pd

from ..core.common import elapsed_time
from ..core.logger import log
from . import _ldscore as lds
from ..core.common import NLDSCParameterError
from .common import (AnnotFile, BIMFile, CovarFile, LDWindow, MAF, PLINKFile, ResidualsSTDThreshold, RSQThreshold,
                     covar_basis, kept_individuals, r2_adjusted)

__all__ = ["estimate_lds", "make_output", "format_scores", "write_scores", "show_summary", "m_values", "write_m_file",
           "annot_output", "m_annot_values", "write_m_annot_file", "reject_sharded_annot", "reject_pairs_options",
           "PAIRS_HEADER", "PAIRS_BUDGET", "open_pairs", "write_pairs", "run_pairs_to_file", "reject_covar_options",
           "covar_basis_of_run", "reject_domdom_options", "domdom_output"]


def show_summary(ld) -> None:
    import click
    pd.set_option("display.precision", 3)
    data = pd.DataFrame({"L2": list(ld.l2), "L2D": list(ld.l2d), "MAF": list(ld.maf)})
    click.echo("=" * 62)
    click.echo("L2/L2D/MAF Correlation matrix\n" + str(data.corr()))
    description = data.describe().drop("count")
    click.echo(f"\nShort summary:\n"
               f"- Number of additive non-null LD: {data['L2'].count()}\n"
               f"- Number of non-additive non-null LD: {data['L2D'].count()}\n"
               + (f"- Number of dominance-by-dominance non-null LD: {int(np.isfinite(np.asarray(ld.l2dd)).sum())}\n"
                  if len(getattr(ld, "l2dd", ())) else "")
               + str(description))
    click.echo("=" * 62)


def make_output(bim: BIMFile, ld, *, extra: bool = False) -> pd.DataFrame:
    cols = {"CHR": bim.chr.reset_index(drop=True), "SNP": bim.snp.reset_index(drop=True),
            "BP": bim.bp.reset_index(drop=True), "L2": pd.Series(list(ld.l2)), "L2D": pd.Series(list(ld.l2d))}
    if extra:
        cols.update(MAF=pd.Series(list(ld.maf)), WSA=pd.Series(list(ld.l2_ws)), WSD=pd.Series(list(ld.l2d_ws)),
                    WSDE=pd.Series(list(ld.l2d_wse)), RSTD=pd.Series(list(ld.residuals_std)))
    return pd.DataFrame(cols)


HEADER = ("CHR", "SNP", "BP", "L2", "L2D")
HEADER_EXTRA = ("MAF", "WSA", "WSD", "WSDE", "RSTD")


def format_scores(bim: BIMFile, ld, *, extra: bool = False) -> bytes:
    """The bytes `make_output(bim, ld, extra=extra).to_csv(path, sep="\t", index=False, float_format="%.5f")`
    writes (routine.py:94-101 of the reference), formatted by the native writer (nldsc_format_scores):
    ~20x faster than pandas on the float columns.  CHR / SNP / BP are printed as pandas prints the parsed
    .bim columns (int64 -> decimal, object -> the text); any other column type goes through pandas."""
    import ctypes

    from .. import _lib
    cols = (bim.chr.reset_index(drop=True), bim.snp.reset_index(drop=True), bim.bp.reset_index(drop=True))
    n = len(cols[0])
    # pandas prints a null object cell (e.g. a SNP id read as NaN: 'NA', 'NULL') as an empty field, str() as 'nan'
    if any(c.dtype.kind not in "iuO" or c.isna().any() for c in cols) or len(ld.l2) != n:
        buf = make_output(bim, ld, extra=extra).to_csv(sep="\t", index=False, float_format="%.5f")
        return buf.encode()
    text = [list(map(str, c.tolist())) for c in cols]  # what pandas prints for int64 / object cells
    f64 = lambda v: np.ascontiguousarray(v, dtype=np.float64)  # noqa: E731
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)  # noqa: E731
    arrs = [f64(ld.l2), f64(ld.l2d)]
    if extra:
        arrs += [f64(ld.maf), i32(ld.l2_ws), i32(ld.l2d_ws), i32(ld.l2d_wse), f64(ld.residuals_std)]
    lib, parts, chunk = _lib.lib(), [], 16384
    out = np.empty(0, np.uint8)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        prefix = "\n".join(map("\t".join, zip(text[0][a:b], text[1][a:b], text[2][a:b]))).encode()
        need = len(prefix) + (b - a) * (16 + 7 * 400) + 1  # worst case of the numeric fields
        if out.size < need:
            out = np.empty(need, np.uint8)
        ptrs = [v[a:].ctypes.data for v in arrs] + [None] * (7 - len(arrs))
        got = lib.nldsc_format_scores(prefix, len(prefix), b - a, *ptrs, int(bool(extra)), out.ctypes.data,
                                      out.size)
        if got < 0:
            raise RuntimeError(f"nldsc_format_scores failed ({got})")
        parts.append(out[:got].tobytes())
    head = "\t".join(HEADER + (HEADER_EXTRA if extra else ())) + "\n"
    return head.encode() + b"".join(parts)


def domdom_output(bim: BIMFile, ld, *, extra: bool = False) -> pd.DataFrame:
    """make_output's table, every column in place, then L2DD (ld.l2dd): the dominance-by-dominance LD scores after
    all existing columns, so the h2 reader's view of the table is the same."""
    df = make_output(bim, ld, extra=extra)
    df["L2DD"] = np.asarray(ld.l2dd, dtype=np.float64)
    return df


def write_scores(path: str, bim: BIMFile, ld, *, extra: bool = False, annot_names=None, dom_dom: bool = False) -> None:
    if dom_dom:  # (never with annot_names: reject_domdom_options)
        domdom_output(bim, ld, extra=extra).to_csv(path, sep="\t", index=False, float_format="%.5f")
        return
    if annot_names is not None:  # partitioned scores: the same table with the per-annotation columns appended
        annot_output(bim, ld, annot_names, extra=extra).to_csv(path, sep="\t", index=False, float_format="%.5f")
        return
    with open(path, "wb") as fh:
        fh.write(format_scores(bim, ld, extra=extra))


def _annot_matrix(values, n_snp: int, n_annot: int) -> np.ndarray:
    """ld.l2_annot / ld.l2d_annot (an [M, C] array, or the pybind result's row-major list) as an [M, C] array."""
    return np.asarray(values, dtype=np.float64).reshape(n_snp, n_annot)


def annot_output(bim: BIMFile, ld, names, *, extra: bool = False) -> pd.DataFrame:
    """make_output's table, every column in place, then L2_<name> for every annotation and L2D_<name> for every
    annotation (ld.l2_annot, ld.l2d_annot)."""
    df = make_output(bim, ld, extra=extra)
    n, c = len(df), len(names)
    for prefix, values in (("L2_", ld.l2_annot), ("L2D_", ld.l2d_annot)):
        mat = _annot_matrix(values, n, c)
        for k, name in enumerate(names):
            df[prefix + name] = mat[:, k]
    return df


def m_annot_values(bim: BIMFile, ld, annot, names) -> pd.DataFrame:
    """Per annotation, over the rows m_values keeps: M_c = sum_j a[j, c] and MD_c = sum_j a[j, c] WSDE_j / WSA_j (for
    an all-ones column the M and MD of m_values before its integer cast).  Columns ANNOT, M, MD."""
    df = make_output(bim, ld, extra=True).sort_values(by=["CHR", "BP"]).dropna().drop_duplicates(subset="SNP")
    a = np.asarray(annot, dtype=np.float64).reshape(len(ld.l2), len(names))[df.index.to_numpy()]
    ratio = (df["WSDE"] / df["WSA"]).to_numpy(dtype=np.float64)
    return pd.DataFrame({"ANNOT": list(names), "M": a.sum(axis=0), "MD": (a * ratio[:, None]).sum(axis=0)})


def write_m_annot_file(path: str, table: pd.DataFrame) -> None:
    table.to_csv(path, sep="\t", index=False, float_format="%.5f")


def reject_sharded_annot() -> None:
    """--annot under torchrun with more than one rank: the sharded gather of the per-annotation columns is not
    built."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NLDSCParameterError("--annot (partitioned LD scores) runs on one GPU: launch it without torchrun, or "
                                  "with one rank (the ranks' tables are gathered without the per-annotation columns)")


def reject_pairs_options(annot: str | None) -> None:
    """--pairs-out with --annot (one band, one sink), or under torchrun with more than one rank (a rank's table would
    cover its shard only)."""
    if annot is not None:
        raise NLDSCParameterError("--pairs-out and --annot cannot be combined: run them separately (an annotated "
                                  "band and a pair table are different runs of the engine)")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NLDSCParameterError("--pairs-out (the pairwise LD table) runs on one GPU: launch it without torchrun, "
                                  "or with one rank")


def reject_covar_options(annot: str | None, pairs_out: str | None, *, sharded_ok: bool = False) -> None:
    """--covar with --annot or --pairs-out (the engine's message: partitioned and pairwise covariate-adjusted output
    is not built), or under torchrun with more than one rank on one chromosome (the ranks' shards would each need
    the basis; a whole-genome run gives every rank whole chromosomes and is fine)."""
    if annot is not None or pairs_out is not None:
        raise NLDSCParameterError("--covar cannot be combined with --annot or --pairs-out: covariates with "
                                  "annotations or a pair table in one run are not supported")
    if not sharded_ok and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NLDSCParameterError("--covar (covariate-adjusted LD scores) runs a chromosome on one GPU: launch it "
                                  "without torchrun, or with one rank")


def reject_domdom_options(annot: str | None, pairs_out: str | None, covar: str | None, flags: int, *,
                          sharded_ok: bool = False) -> None:
    """--dom-dom with --annot, --pairs-out or --covar (the engine's message: they are different runs of the engine),
    with --additive-only (no dominance residuals), or under torchrun with more than one rank on one chromosome (the
    ranks' tables are gathered without the L2DD column; a whole-genome run gives every rank whole chromosomes and is
    fine)."""
    if annot is not None or pairs_out is not None or covar is not None:
        raise NLDSCParameterError("--dom-dom cannot be combined with --annot, --pairs-out or --covar: dom-dom scores "
                                  "with annotations, a pair table or covariates in one run are not supported")
    if int(flags) & lds.FLAG_ADDITIVE_ONLY:
        raise NLDSCParameterError("--dom-dom cannot be combined with --additive-only: the dominance-by-dominance "
                                  "scores need the dominance residuals")
    if not sharded_ok and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NLDSCParameterError("--dom-dom (dominance-by-dominance LD scores) runs a chromosome on one GPU: launch "
                                  "it without torchrun, or with one rank")


def covar_basis_of_run(covar: str, fam, kept) -> np.ndarray:
    """The orthonormal basis Q ([n, q]) of the covariate file `covar` for a run on the .fam lines `kept` (None:
    everyone) of `fam`: its rows matched to those individuals by (FID, IID), in .fam order (CovarFile.matrix), then
    common.covar_basis.  Logs the covariates read, the rank kept and the columns dropped."""
    cf = CovarFile(covar)
    fam_ids = fam.ids
    ids = fam_ids if kept is None else [fam_ids[int(s)] for s in kept]
    q, dropped = covar_basis(cf.matrix(ids))
    names = cf.names
    log.info(f"Covariates: c = {len(names)} columns of {covar} for {len(ids)} individuals, q = {q.shape[1]} kept"
             + (f"; dropped (constant or dependent): {', '.join(names[j] for j in dropped)}" if dropped else ""))
    if q.shape[1] == 0:
        raise NLDSCParameterError(f'"{covar}": every covariate column is constant: nothing to adjust for')
    return q


# ---- the pairwise LD table (--pairs-out): one row per ordered pair (SNP_A, SNP_B) the run counts in WSA[SNP_A] ----
PAIRS_HEADER = ("CHR", "SNP_A", "BP_A", "SNP_B", "BP_B", "R", "R2", "RD", "R2D")
PAIRS_BUDGET = 32 * 1024 * 1024  # pairs per engine call (20 bytes each on the device, 36 in the host arrays)


def open_pairs(path: str):
    """A new pair table at `path` (gzip-compressed for a .gz suffix) with its header line; a text file object."""
    import gzip
    fh = gzip.open(path, "wt", newline="") if str(path).endswith(".gz") else open(path, "w", newline="")
    fh.write("\t".join(PAIRS_HEADER) + "\n")
    return fh


def write_pairs(fh, bim: BIMFile, table: dict, own_begin: int, n_org: int) -> int:
    """Append the rows of one owned range (a CSR table of Engine.run_pairs: row_ptr, k, r, rd; row 0 is SNP own_begin)
    to the pair table `fh`: CHR SNP_A BP_A SNP_B BP_B R R2 RD R2D, tab-separated, floats "%.6f", NaN as an empty
    field; R2 / R2D are r2_adjusted of R / RD for n_org individuals.  Returns the number of rows."""
    row_ptr = np.asarray(table["row_ptr"], dtype=np.int64)
    k = np.asarray(table["k"], dtype=np.int64)
    if len(k) == 0:
        return 0
    j = own_begin + np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    snp, bp, chrom = bim.snp.to_numpy(), bim.bp.to_numpy(), bim.chr.to_numpy()
    r, rd = np.asarray(table["r"], dtype=np.float64), np.asarray(table["rd"], dtype=np.float64)
    df = pd.DataFrame({"CHR": chrom[j], "SNP_A": snp[j], "BP_A": bp[j], "SNP_B": snp[k], "BP_B": bp[k], "R": r,
                       "R2": r2_adjusted(r, n_org), "RD": rd, "R2D": r2_adjusted(rd, n_org)})
    df.to_csv(fh, sep="\t", index=False, header=False, float_format="%.6f", na_rep="")
    return len(df)


def run_pairs_to_file(engine, ld_wind, maf, std_thr, rsq_thr, positions, flags, *, path: str, bim: BIMFile,
                      min_r2: float | None = None, budget: int = PAIRS_BUDGET, size_snps: int = 65536) -> dict:
    """A run of the resident image that also writes its pair table to `path`: sizing calls over at most size_snps SNPs
    each give the result arrays (bitwise a plain run's) and the table's row_ptr; the chromosome then goes in owned
    ranges of at most `budget` pairs (_lib.pairs_split_ranges on that row_ptr), each appended to the file.  Returns
    the result dict of Engine.run."""
    from .. import _lib
    n = engine.n_snp
    args = (ld_wind, maf, std_thr, rsq_thr, positions)
    res, row_ptr = None, [np.zeros(1, np.int64)]
    for lo in range(0, n, size_snps):
        hi = min(n, lo + size_snps)
        s = engine.size_pairs(*args, own=(lo, hi), flags=flags, min_r2=min_r2)
        if res is None:
            res = {key: s[key] for key in ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")}
        else:
            for key in res:
                res[key][lo:hi] = s[key][lo:hi]
        row_ptr.append(s["row_ptr"][1:] + row_ptr[-1][-1])
    row_ptr = np.concatenate(row_ptr)
    rows = 0
    with open_pairs(path) as fh:
        for lo, hi in _lib.pairs_split_ranges(row_ptr, budget):
            t = engine._pairs(*args, (lo, hi), flags, min_r2, emit=True, cap=int(row_ptr[hi] - row_ptr[lo]))
            rows += write_pairs(fh, bim, t, lo, engine.n_org)
    log.info(f"Pair table: {rows:,} rows in {path}")
    return res


def m_values(bim: BIMFile, ld) -> tuple[int, int]:
    """M, MD as LDScoreReader derives them without an .M file (h2/common.py:128-130): rows
    surviving dropna + SNP de-duplication, and M * mean(WSDE / WSA)."""
    df = make_output(bim, ld, extra=True).sort_values(by=["CHR", "BP"]).dropna().drop_duplicates(subset="SNP")
    m = len(df["L2"])
    md = m * (df["WSDE"] / df["WSA"]).mean()
    return int(m), int(md)


def write_m_file(path: str, m: int, md: int) -> None:
    pd.DataFrame({"M": [m], "MD": [md]}).to_csv(path, sep="\t", index=False)


class _Result:
    """LDScoreResult-shaped holder for tables assembled from several ranks."""

    def __init__(self, d: dict):
        for k, v in d.items():
            setattr(self, k, v.tolist())


def _backend() -> str:
    """Collectives backend of the torchrun path: RCCL ("nccl", one GPU per rank) unless $NLDSC_DIST_BACKEND
    says "gloo" (CPU collectives; ranks may then share GPUs, e.g. a 2-rank rehearsal on one GPU)."""
    return os.environ.get("NLDSC_DIST_BACKEND", "nccl")


def _split_halo() -> bool:
    """$NLDSC_SPLIT_HALO=1: boundary pairs computed once across ranks (right halo's sums sent point to point); by
    default each rank loads a two-sided halo and computes them itself (the same band time at C3/8, no exchange)."""
    return os.environ.get("NLDSC_SPLIT_HALO", "0") != "0"


def _local_device() -> int:
    import torch
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return local if _backend() == "nccl" else local % max(1, torch.cuda.device_count())


def _process_group():
    """The torch.distributed module when launched by torchrun with WORLD_SIZE > 1, else None."""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return None
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        dev = _local_device()
        torch.cuda.set_device(dev)
        if _backend() == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{dev}"))
        else:
            dist.init_process_group(_backend())
    return dist


def _calculate_sharded(dist, params):
    from .. import distributed as D
    dev = _local_device()
    pos = np.asarray(params.positions, dtype=np.float64)
    keep = np.asarray(params.keep, dtype=np.int32) if len(params.keep) else None
    plan = D.split_plan(pos, params.ld_wind, dist.get_world_size()) if _split_halo() else None
    if plan is not None:  # boundary pairs once: halo sums sent to the next rank (point to point)
        full = D.calculate_sharded_split(params.bedfile, params.n_snp, params.n_org, params.ld_wind, params.maf,
                                         params.std_thr, params.rsq_thr, pos, plan, flags=params.flags, device=dev,
                                         keep=keep)
    elif _backend() == "nccl":  # the owned slices stay in device memory and are gathered over RCCL
        full = D.calculate_sharded_device(params.bedfile, params.n_snp, params.n_org, params.ld_wind, params.maf,
                                          params.std_thr, params.rsq_thr, pos, flags=params.flags, device=dev,
                                          keep=keep)
    else:  # gloo: host result arrays, CPU collectives
        run = D.engine_runner(params.bedfile, params.n_snp, params.n_org, params.ld_wind, params.maf,
                              params.std_thr, params.rsq_thr, pos, flags=params.flags, device=dev, keep=keep)
        full = D.calculate_sharded(run, pos, params.ld_wind, params.n_snp)
    return None if full is None else _Result(full)


@elapsed_time
def estimate_lds(bfile: str, ld_wind: float, wind_metric: str, maf_thr: float = 1e-5, std_thr: float = 1e-5,
                 rsq_thr: float | None = None, *, out: str | None = None, extra: bool = False, summary: bool = False,
                 verbose: int = 0, write_m: bool = False, flags: int = 0, device: int | None = None,
                 progress: bool | None = None, keep: str | None = None, remove: str | None = None,
                 annot: str | None = None, pairs_out: str | None = None, pairs_min_r2: float | None = None,
                 pairs_budget: int = PAIRS_BUDGET, covar: str | None = None, dom_dom: bool = False):
    """`dom_dom`: also the dominance-by-dominance LD scores L2DD_j = 1 + sum_k r2adj(R_j . R_k / N) (d-LDSC): the
    column L2DD after all other columns of the table; the run takes the closed-form vectors of rare variants, as a
    `covar` run does; not with `annot`, `pairs_out`, `covar` or the additive-only flag.
    `covar`: path of a PLINK covariate file (common.CovarFile): covariate-adjusted LD scores (cov-LDSC) on the
    orthonormal basis of its columns for the run's individuals (covar_basis_of_run), in PLINK's sample order.
    `pairs_out`: also write the pairwise LD table behind the scores there (write_pairs; `.gz` compresses), with
    `pairs_min_r2` only the pairs whose R2 or R2D exceeds it, in engine calls of at most `pairs_budget` pairs; the
    scores are the same, bit for bit.
    `keep` / `remove`: paths of `FID IID` lists (PLINK's / LDSC's --keep, --remove): the scores are computed on the
    .fam lines of the first minus those of the second, in PLINK's sample order (common.kept_individuals).
    `annot`: path of an LDSC `.annot` / `.annot.gz` file (common.AnnotFile): partitioned LD scores, the table gains
    L2_<name> and L2D_<name> columns and `write_m` also writes `<out>.M_annot`."""
    if dom_dom:
        reject_domdom_options(annot, pairs_out, covar, flags)
    if covar is not None:
        reject_covar_options(annot, pairs_out)
    if pairs_out is not None:
        reject_pairs_options(annot)
    if annot is not None:
        reject_sharded_annot()
    bed_, bim_, fam_ = PLINKFile.parse(bfile)
    annot_ = AnnotFile(annot, bim_) if annot is not None else None
    ld_wind_ = LDWindow(ld_wind, metric=wind_metric)
    maf_thr_ = MAF(maf_thr)
    std_thr_ = ResidualsSTDThreshold(std_thr)
    if rsq_thr is None:
        rsq_thr = 1.0 / bim_.n_snp
    rsq_thr_ = RSQThreshold(rsq_thr)
    kept = kept_individuals(fam_, keep, remove)
    if kept is None:
        log.info(f"Input: {bed_.data}, size: (M={bim_.n_snp}, N={fam_.n_org})")
    else:
        log.info(f"Input: {bed_.data}, size: (M={bim_.n_snp}, N = {len(kept)} of {fam_.n_org})")

    params = lds.LDScoreParams(
        bfile=bed_.data, n_snp=bim_.n_snp, n_org=fam_.n_org, ld_wind=ld_wind_.data, maf=maf_thr_.data,
        std_thr=std_thr_.data, rsq_thr=rsq_thr_.data,
        positions=np.asarray(getattr(bim_, ld_wind_.metric), dtype=np.float64).tolist())
    params.flags = int(flags)
    if kept is not None:
        params.keep = kept.tolist()
    if device is not None:
        params.device = int(device)
    if annot_ is not None:
        params.annot = annot_.data.ravel().tolist()
        log.info(f"Annotations: {len(annot_.names)} columns of {annot}")
    if dom_dom:
        params.dom_dom = True
    log.info("Running the estimator. It may take a long time.")
    from ..core.progress import Progress
    bar = Progress(bim_.n_snp, "SNPs", enabled=progress)
    bar.update(0, "reading the .bed and computing on the GPU", force=True)
    dist = _process_group()
    if covar is not None:  # the engine itself: the basis built once on the host, then one covariate run
        from .genome import _default_runner
        basis = covar_basis_of_run(covar, fam_, kept)
        run = _default_runner(-1 if device is None else int(device), kept, fam_.n_org)
        res, _ = run(bed_.data, bim_.n_snp, fam_.n_org, ld_wind_.data, maf_thr_.data, std_thr_.data, rsq_thr_.data,
                     np.asarray(params.positions, dtype=np.float64), int(flags), covar=basis)
        ld = _Result(res)
    elif pairs_out is not None:  # the engine itself: one load, the sizing and emitting calls of every owned range
        from .genome import _default_runner
        run = _default_runner(-1 if device is None else int(device), kept, fam_.n_org)
        res, _ = run(bed_.data, bim_.n_snp, fam_.n_org, ld_wind_.data, maf_thr_.data, std_thr_.data, rsq_thr_.data,
                     np.asarray(params.positions, dtype=np.float64), int(flags),
                     pairs=dict(path=pairs_out, bim=bim_, min_r2=pairs_min_r2, budget=pairs_budget))
        ld = _Result(res)
    elif dist is None:
        ld = lds.calculate(params)
    else:  # torchrun: position-sharded over the ranks' GPUs, tables gathered on rank 0
        ld = _calculate_sharded(dist, params)
        if ld is None:
            return None
    ws = np.asarray(ld.l2_ws)
    bar.close(f"{int(ws[ws > 0].sum()):,} SNP pairs")
    log.info("Estimation completed")

    if summary:
        show_summary(ld)
    if out:
        log.info("Writing data to disk...")
        write_scores(out, bim_, ld, extra=extra, annot_names=annot_.names if annot_ is not None else None,
                     dom_dom=dom_dom)
        if write_m:
            m, md = m_values(bim_, ld)
            write_m_file(str(Path(out).with_suffix(".M")), m, md)
            if annot_ is not None:
                write_m_annot_file(str(Path(out).with_suffix(".M_annot")),
                                   m_annot_values(bim_, ld, annot_.data, annot_.names))
        log.info(f"Completed. File: {out}")
        return None
    if annot_ is not None:
        return annot_output(bim_, ld, annot_.names, extra=extra)
    if dom_dom:
        return domdom_output(bim_, ld, extra=extra)
    return make_output(bim_, ld, extra=extra)
