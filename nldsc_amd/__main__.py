"""`python -m nldsc_amd ld ...` — the `nldsc ld` command (nldsc/__main__.py:35-97) on the GPU engine."""
import sys

import click

from . import __version__
from .core.logger import log

__header__ = (f"\n==============================================================\n"
              f"* Non-additive LD Score Regression (NLDSC) — MI355X engine v{__version__}\n"
              f"* LD-score compute path re-implemented for AMD Instinct MI355X (gfx950)\n"
              f"* Interface of bayarpark/nldsc `nldsc ld` (GPL-3.0)\n"
              f"==============================================================\n")


def handle_exception(func):
    """Same failure shape as the reference (nldsc/__main__.py:17-26)."""
    def handler(*args, **kwargs):
        display = kwargs.pop("display", None)
        try:
            return func(*args, **kwargs)
        except Exception as ex:  # noqa: BLE001
            log.critical(f"The program crashed with {ex.__class__.__name__}, what: {str(ex)}\n"
                         f"Use `--display` flag for traceback", exc_info=display)
            raise SystemExit()
    handler.__name__ = func.__name__
    handler.__doc__ = func.__doc__
    return handler


@click.group()
@click.version_option(version=__version__)
def main():
    click.echo(__header__)


@main.command("ld", help="Estimate additive and non-additive LD Scores")
@click.option("--bfile", help="Path prefix for PLINK .bed/.bim/.fam file or path to one of them; '@' in place of "
                               "the chromosome number runs every chromosome (then --out needs '@' too)", metavar="FILE",
              required=True)
@click.option("-o", "--out", help="Output path of the LD score table", metavar="FILE")
@click.option("-kb", "--ld-wind-kb", help="Window size in kilo-base pairs (kb)", metavar="W")
@click.option("-cm", "--ld-wind-cm", help="Window size in centi-morgans (cM)", metavar="W")
@click.option("-maf", "--maf-thr", help="Minor allele frequency threshold (lower bound)", metavar="F")
@click.option("-std", "--std-thr", help="Standard deviation threshold for regression residuals", metavar="F",
              default=1e-4)
@click.option("-rsq", "--rsq-thr", help="R-squared threshold for regression residual. It affects only dominant "
                                        "window sizes and, therefore, non-additive sample size (MD)", metavar="F")
@click.option("--extra", help="Include additional information to the .L2 file", is_flag=True, default=False)
@click.option("--write-m", help="Also write <out>.M with M and MD (as the h2 reader derives them)", is_flag=True,
              default=False)
@click.option("--strict-plink-order", help="Use PLINK sample order in the last .bed byte (the reference does not)",
              is_flag=True, default=False)
@click.option("--keep", help="Use only the individuals listed in FILE (FID IID per line), as PLINK's --keep; "
                             "implies PLINK sample order (--strict-plink-order)", metavar="FILE", default=None)
@click.option("--remove", help="Leave out the individuals listed in FILE (FID IID per line), as PLINK's --remove; "
                               "implies PLINK sample order (--strict-plink-order)", metavar="FILE", default=None)
@click.option("--annot", help="Partitioned LD scores: FILE is an LDSC .annot / .annot.gz (with '@' for the chromosome "
                              "in a whole-genome run); adds L2_<name> / L2D_<name> columns and, with --write-m, "
                              "<out>.M_annot", metavar="FILE", default=None)
@click.option("--pairs-out", help="Also write the pairwise LD table behind the scores to FILE (.gz compresses; '@' for "
                                  "the chromosome in a whole-genome run): CHR SNP_A BP_A SNP_B BP_B R R2 RD R2D, one "
                                  "row per SNP_A and neighbour SNP_B in its window", metavar="FILE", default=None)
@click.option("--pairs-min-r2", help="Keep only the pairs of --pairs-out whose R2 or R2D exceeds F", metavar="F",
              type=float, default=None)
@click.option("--covar", help="Covariate-adjusted LD scores (cov-LDSC): FILE is a PLINK covariate file (FID IID c1 "
                              "c2 ..., optional header) with a row for every individual of the run; every genotype "
                              "vector is residualised on the covariates before the correlations; implies PLINK sample "
                              "order (--strict-plink-order); not with --annot or --pairs-out", metavar="FILE",
              default=None)
@click.option("--dom-dom", help="Also the dominance-by-dominance LD scores (d-LDSC): the column L2DD, the LD score of "
                                "the dominance deviations with each other, after all other columns; not with --annot, "
                                "--pairs-out, --covar or --additive-only", is_flag=True, default=False)
@click.option("--additive-only", help="Skip the dominance terms (L2D = NaN)", is_flag=True, default=False)
@click.option("--device", help="HIP device ordinal", type=int, default=None)
@click.option("--quiet", help="No progress lines on stderr", is_flag=True, default=False)
@click.option("--display", help="Display traceback", is_flag=True, default=False)
@handle_exception
def est_ld(bfile, out, ld_wind_kb, ld_wind_cm, maf_thr, std_thr, rsq_thr, extra, write_m, strict_plink_order,
           keep, remove, annot, pairs_out, pairs_min_r2, covar, dom_dom, additive_only, device, quiet):
    if sum(map(bool, [ld_wind_kb, ld_wind_cm])) != 1:
        raise RuntimeError("Please, specify exactly one --ld-wind option")
    elif ld_wind_kb:
        wind_metric, ld_wind = "kbp", ld_wind_kb
    else:
        wind_metric, ld_wind = "cm", ld_wind_cm
    from .ldscore import _ldscore, estimate_lds
    flags = (_ldscore.FLAG_STRICT_PLINK_ORDER if strict_plink_order else 0) | \
            (_ldscore.FLAG_ADDITIVE_ONLY if additive_only else 0)
    if "@" in bfile:  # whole genome: one output per chromosome, chromosomes spread over GPUs
        from .ldscore.genome import estimate_lds_genome
        estimate_lds_genome(bfile, ld_wind=ld_wind, wind_metric=wind_metric, maf_thr=maf_thr, std_thr=std_thr,
                            rsq_thr=rsq_thr, out=out, extra=extra, write_m=write_m, flags=flags, device=device,
                            progress=not quiet, keep=keep, remove=remove, annot=annot, pairs_out=pairs_out,
                            pairs_min_r2=pairs_min_r2, covar=covar, dom_dom=dom_dom)
        return
    estimate_lds(bfile, ld_wind=ld_wind, wind_metric=wind_metric, maf_thr=maf_thr, std_thr=std_thr,
                 rsq_thr=rsq_thr, out=out, extra=extra, summary=True, write_m=write_m, flags=flags, device=device,
                 progress=not quiet, keep=keep, remove=remove, annot=annot, pairs_out=pairs_out,
                 pairs_min_r2=pairs_min_r2, covar=covar, dom_dom=dom_dom)


@main.command("h2", help="(not part of this engine) heritability estimation")
def est_h2():
    raise SystemExit("`h2` is out of scope for nldsc_amd: run the reference's `nldsc h2` on the .L2 output.")


if __name__ == "__main__":
    sys.exit(main())
