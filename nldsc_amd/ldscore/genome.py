"""Whole-genome `nldsc ld`: one invocation over per-chromosome PLINK sets.

`--bfile chr@` expands `@` to the chromosome numbers whose `.bed/.bim/.fam` exist (1..22, then X/Y/MT).
Every chromosome is an independent unit (the reference accepts one chromosome per file,
nldsc/ldscore/common.py:114-117, and windows never cross chromosomes).  Under torchrun the units are
assigned to GPUs by longest-processing-time first on their estimated pair count; each rank writes the
outputs of its own chromosomes (`--out` must contain `@` too), so nothing crosses GPUs.  On each GPU
the next chromosome's `.bed` is read by a host thread while the current one is computed.
"""
from __future__ import annotations

import os
import threading
import time
from pathlib import Path

import numpy as np

from ..core.common import NLDSCParameterError, elapsed_time
from ..core.logger import log
from .common import (AnnotFile, FAMFile, BIMFile, LDWindow, MAF, ResidualsSTDThreshold, RSQThreshold,
                     kept_individuals)
from .routine import (PAIRS_BUDGET, annot_output, covar_basis_of_run, domdom_output, m_annot_values, m_values,
                      make_output, reject_domdom_options,
                      reject_covar_options, reject_pairs_options, reject_sharded_annot, run_pairs_to_file,
                      write_m_annot_file, write_m_file, write_scores)

CHROMS = [str(c) for c in range(1, 23)] + ["X", "Y", "XY", "MT"]


def expand_bfile(pattern: str) -> list[tuple[str, str]]:
    """[(chromosome, prefix)] for a pattern with '@' whose three PLINK files exist."""
    if "@" not in pattern:
        raise NLDSCParameterError("a whole-genome --bfile needs '@' in place of the chromosome number")
    p = pattern[:-4] if pattern.endswith((".bed", ".bim", ".fam")) else pattern
    out = []
    for c in CHROMS:
        stem = p.replace("@", c)
        if all(os.path.exists(stem + ext) for ext in (".bed", ".bim", ".fam")):
            out.append((c, stem))
    if not out:
        raise FileNotFoundError(f'No PLINK file set matches "{pattern}"')
    return out


class _Prefetch:
    """Reads a .bed file on a host thread (the read releases the GIL)."""

    def __init__(self, path: str):
        self.path, self.data, self.err = path, None, None
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _run(self):
        try:
            self.data = np.fromfile(self.path, dtype=np.uint8)
        except Exception as ex:  # noqa: BLE001
            self.err = ex

    def get(self) -> np.ndarray:
        self.t.join()
        if self.err is not None:
            raise self.err
        return self.data


def _readahead(path: str) -> None:
    """Ask the kernel to start reading `path` into the page cache (asynchronous readahead)."""
    try:
        fd = os.open(path, os.O_RDONLY)
        try:
            os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_WILLNEED)
        finally:
            os.close(fd)
    except (OSError, AttributeError):
        pass


def _default_runner(device: int, keep=None, n_org_file: int = 0):
    """The GPU engine, fed by its own file reader (file -> pinned slots -> pitched H2D copies overlapping
    the reads, ~20 GB/s from the page cache) instead of a host array copied from pageable memory.  `keep`: the
    individuals every chromosome is computed on (set once: Engine.set_keep), of n_org_file in the files."""
    from ..engine import Engine
    eng = Engine(device)
    if keep is not None:
        eng.set_keep(keep, n_org_file)

    def run(bed_path: str, n_snp: int, n_org: int, ld_wind, maf, std_thr, rsq_thr, positions, flags, annot=None,
            pairs=None, covar=None, dom_dom=False):
        eng.load_bed_file(bed_path, n_snp, n_org)
        if dom_dom:  # (--dom-dom: the usual arrays plus "l2dd")
            return eng.run_domdom(ld_wind, maf, std_thr, rsq_thr, positions, flags=flags), eng.timings()
        if covar is not None:  # (--covar: the orthonormal basis, one row per individual of the image)
            return eng.run(ld_wind, maf, std_thr, rsq_thr, positions, flags=flags, covar=covar), eng.timings()
        if pairs is not None:  # (--pairs-out: dict(path, bim, min_r2, budget))
            return run_pairs_to_file(eng, ld_wind, maf, std_thr, rsq_thr, positions, flags, **pairs), eng.timings()
        return eng.run(ld_wind, maf, std_thr, rsq_thr, positions, flags=flags, annot=annot), eng.timings()
    run.wants_path = True
    return run


@elapsed_time
def estimate_lds_genome(bfile: str, ld_wind: float, wind_metric: str, maf_thr: float = 1e-5,
                        std_thr: float = 1e-5, rsq_thr: float | None = None, *, out: str | None = None,
                        extra: bool = False, write_m: bool = False, flags: int = 0, device: int | None = None,
                        runner=None, rank: int | None = None, world: int | None = None,
                        progress: bool | None = None, keep: str | None = None,
                        remove: str | None = None, annot: str | None = None, pairs_out: str | None = None,
                        pairs_min_r2: float | None = None, pairs_budget: int = PAIRS_BUDGET,
                        covar: str | None = None, dom_dom: bool = False) -> dict:
    """Returns {chromosome: output DataFrame (None when written to `out`)} for the chromosomes this rank
    processed.  `keep` / `remove`: `FID IID` lists as in estimate_lds; every chromosome's .fam must resolve to the
    same individuals (a `runner` given by the caller then receives them as the keyword `keep`).  `annot`: an LDSC
    `.annot` / `.annot.gz` path with '@' in place of the chromosome, as in `bfile` (a runner then receives each
    chromosome's [M, C] matrix as the keyword `annot`).  `pairs_out`: a path with '@' for each chromosome's pairwise
    LD table, as in estimate_lds (a runner then receives dict(path, bim, min_r2, budget) as the keyword `pairs` and
    writes the table itself).  `covar`: one PLINK covariate file for every chromosome, as in estimate_lds: the basis is
    built once, for the first chromosome's .fam — with `covar` every chromosome's .fam must list the same individuals
    in the same order (a runner then receives the [n, q] basis as the keyword `covar`).  `dom_dom`: the
    dominance-by-dominance LD scores of every chromosome, as in estimate_lds (a runner then receives the keyword
    `dom_dom=True` and returns "l2dd" with the usual arrays)."""
    if dom_dom:
        reject_domdom_options(annot, pairs_out, covar, flags, sharded_ok=True)
    if covar is not None:
        reject_covar_options(annot, pairs_out, sharded_ok=True)
    if pairs_out is not None:
        reject_pairs_options(annot)
        if "@" not in pairs_out:
            raise NLDSCParameterError("a whole-genome run needs '@' in --pairs-out (one pair table per chromosome)")
    if annot is not None:
        reject_sharded_annot()
        if "@" not in annot:
            raise NLDSCParameterError("a whole-genome run needs '@' in --annot (one annotation file per chromosome)")
    units = expand_bfile(bfile)
    if out is not None and "@" not in out:
        raise NLDSCParameterError("a whole-genome run needs '@' in --out (one output per chromosome)")
    ld_wind_ = LDWindow(ld_wind, metric=wind_metric)
    maf_thr_, std_thr_ = MAF(maf_thr), ResidualsSTDThreshold(std_thr)
    if rank is None or world is None:
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    # cheap host pass: .bim/.fam of every unit, pair-work estimate for the assignment
    from ..distributed import assign_units, window_work
    meta = []
    kept, kept_n_file = None, 0
    fam0 = None  # (--covar: the first chromosome's .fam, whose individuals the basis rows are)
    for chrom, stem in units:
        bim, fam = BIMFile(stem + ".bim"), FAMFile(stem + ".fam")
        if covar is not None:
            if fam0 is None:
                fam0 = fam
            elif fam.ids != fam0.ids:
                raise NLDSCParameterError(f"--covar: {stem}.fam lists other individuals (or another order) than "
                                          f"{units[0][1]}.fam: every chromosome needs the same .fam")
        if keep is not None or remove is not None:
            k = kept_individuals(fam, keep, remove)
            if kept is None:
                kept, kept_n_file = k, fam.n_org
                log.info(f"N = {len(kept)} of {fam.n_org}")
            elif fam.n_org != kept_n_file or not np.array_equal(k, kept):
                raise NLDSCParameterError(f"--keep / --remove select other individuals in {stem}.fam than in "
                                          f"{units[0][1]}.fam: every chromosome needs the same .fam")
        pos = np.asarray(getattr(bim, ld_wind_.metric), dtype=np.float64)
        meta.append(dict(chrom=chrom, stem=stem, bim=bim, n_org=fam.n_org, pos=pos,
                         work=float(window_work(pos, ld_wind_.data).sum()) * fam.n_org))
    covar_kw = {} if covar is None else {"covar": covar_basis_of_run(covar, fam0, kept)}
    if dom_dom:
        covar_kw["dom_dom"] = True
    mine = assign_units([m["work"] for m in meta], world)[rank]
    log.info(f"[rank {rank}/{world}] {len(mine)} of {len(units)} chromosomes: "
             f"{', '.join(meta[u]['chrom'] for u in mine)}")
    if runner is None:
        if device is None:  # torchrun: one rank per GPU (ranks beyond the visible GPUs share them round-robin)
            from .. import _lib
            local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, _lib.lib().nldsc_device_count())
        else:
            local = int(device)
        runner = _default_runner(local, kept, kept_n_file)
        kept_kw = {}
    else:
        kept_kw = {} if kept is None else {"keep": kept}
    from ..core.progress import Progress
    total_snp = sum(meta[u]["bim"].n_snp for u in mine)
    bar = Progress(total_snp, "SNPs", label=f"ld rank {rank}" if world > 1 else "ld", enabled=progress,
                   any_rank=True)
    done_snp = 0
    results = {}
    # a path-fed runner (the engine's own reader) gets the next file read ahead into the page cache;
    # other runners get the bytes, read by a host thread while the current chromosome computes
    by_path = getattr(runner, "wants_path", False)
    pre = None
    if mine and not by_path:
        pre = _Prefetch(meta[mine[0]]["stem"] + ".bed")
    for k, u in enumerate(mine):
        m = meta[u]
        nxt = meta[mine[k + 1]]["stem"] + ".bed" if k + 1 < len(mine) else None
        if by_path:
            bed = m["stem"] + ".bed"
            if nxt is not None:
                threading.Thread(target=_readahead, args=(nxt,), daemon=True).start()
        else:
            bed = pre.get()
            pre = _Prefetch(nxt) if nxt is not None else None
        n_snp = m["bim"].n_snp
        rsq = RSQThreshold(1.0 / n_snp if rsq_thr is None else rsq_thr).data
        t0 = time.perf_counter()
        annot_ = AnnotFile(annot.replace("@", m["chrom"]), m["bim"]) if annot is not None else None
        annot_kw = {} if annot_ is None else {"annot": annot_.data}
        if pairs_out is not None:
            annot_kw["pairs"] = dict(path=pairs_out.replace("@", m["chrom"]), bim=m["bim"], min_r2=pairs_min_r2,
                                     budget=pairs_budget)
        res, tim = runner(bed, n_snp, m["n_org"], ld_wind_.data, maf_thr_.data, std_thr_.data, rsq, m["pos"], flags,
                          **kept_kw, **annot_kw, **covar_kw)
        ld = _Res(res)
        names = annot_.names if annot_ is not None else None
        if out is None:
            df = domdom_output(m["bim"], ld, extra=extra) if dom_dom else \
                make_output(m["bim"], ld, extra=extra) if names is None else annot_output(m["bim"], ld, names,
                                                                                          extra=extra)
        else:
            df = None
            path = out.replace("@", m["chrom"])
            write_scores(path, m["bim"], ld, extra=extra, annot_names=names, dom_dom=dom_dom)
            if write_m:
                mm, md = m_values(m["bim"], ld)
                write_m_file(str(Path(path).with_suffix(".M")), mm, md)
                if names is not None:
                    write_m_annot_file(str(Path(path).with_suffix(".M_annot")),
                                       m_annot_values(m["bim"], ld, annot_.data, names))
        results[m["chrom"]] = df
        log.info(f"[rank {rank}] chr{m['chrom']}: M={n_snp} N={m['n_org']} "
                 f"in {time.perf_counter() - t0:.2f} s")
        done_snp += n_snp
        bar.update(done_snp, f"{k + 1}/{len(mine)} chromosomes, chr{m['chrom']} done")
    bar.close(f"{len(mine)} chromosomes")
    return results


class _Res:
    def __init__(self, d: dict):
        for k, v in d.items():
            setattr(self, k, list(v))
