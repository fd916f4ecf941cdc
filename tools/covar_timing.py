"""Cost of covariate-adjusted LD scores (nldsc_engine_run_covar) against the plain run, on a resident C3 image.

The image (synth.device_bed, N = 315 599, M = 80 000, 1 % missing calls, the bench's run parameters) is loaded once;
each case runs once to warm up and then `--reps` times, each call synchronous, wall clock around the call and the
engine's own stage timings beside it.  Cases: the plain run (PLINK sample order, closed-form rare variants: what a
covariate run implies), and covariate runs on q = 1, 10, 20, 40 orthonormal standard-normal covariates.  The projection
(covar_project_kernel and the per-SNP kernel after it) runs inside the statistics stage, so its GPU time is that
stage's time less the plain run's; the band is the stage of that name.  The projection is reported against two floors:
one read of the image at `--hbm-gbs`, and 6 M N q fp64 flop at `--fp64-tflops` (tools/study/mfma_f64_rate.hip measures
the part's v_mfma_f64_16x16x4_f64 rate); the band against profiles/annot_c3.json's all-ones annotated run, which has
the same launch structure.  Medians go to `--out` (profiles/covar_c3.json).

    python tools/covar_timing.py --fp64-tflops <measured> --out profiles/covar_c3.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-org", type=int, default=315_599)
    ap.add_argument("--n-snp", type=int, default=80_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--q", type=int, nargs="+", default=[1, 10, 20, 40])
    ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="achievable HBM rate of the image-read floor (GB/s)")
    ap.add_argument("--fp64-tflops", type=float, default=None, help="fp64 MFMA rate of the flop floor (measured)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from nldsc_amd import _lib, synth
    from nldsc_amd.engine import Engine
    N, M = args.n_org, args.n_snp
    img, pos = synth.device_bed(M, N)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    qmax = max(args.q)
    z = rng.standard_normal((N, qmax))
    basis = np.linalg.qr(z - z.mean(axis=0))[0]
    basis -= basis.mean(axis=0)
    cases = {"plain": None}
    cases.update({f"covar_q{q}": np.ascontiguousarray(basis[:, :q]) for q in args.q})
    run_args = (1.0, 1e-4, 1e-5, 1.0 / M)
    flags = _lib.FLAG_STRICT_PLINK_ORDER | _lib.FLAG_EXACT_RARE
    res = {}
    with Engine(0) as e:
        e.load_bed_device(img.data_ptr(), img.numel(), M, N)
        image_bytes = img.numel()
        del img
        torch.cuda.empty_cache()
        for name, covar in cases.items():
            ms, stats, band, tim = [], [], [], {}
            for k in range(args.reps + 1):
                t0 = time.perf_counter()
                e.run(*run_args, pos, flags=flags, covar=covar)
                ms.append(1e3 * (time.perf_counter() - t0))
                tim = e.timings()
                stats.append(tim["stats_ms"])
                band.append(tim["band_ms"])
            res[name] = {"q": 0 if covar is None else covar.shape[1],
                         "median_ms": round(statistics.median(ms[1:]), 3), "all_ms": [round(v, 3) for v in ms[1:]],
                         "warmup_ms": round(ms[0], 3), "stats_ms": round(statistics.median(stats[1:]), 3),
                         "band_ms": round(statistics.median(band[1:]), 3), "band_items": tim["band_items"],
                         "band_kernel": tim["band_kernel"], "ksplit": tim["ksplit"]}
    plain = res["plain"]
    annot_band = None
    try:
        with open(os.path.join(REPO, "profiles", "annot_c3.json")) as fh:
            annot_band = json.load(fh)["runs"]["annot_1_all_ones"]["band_ms"]
    except (OSError, KeyError, ValueError):
        pass
    read_floor = image_bytes / (args.hbm_gbs * 1e9) * 1e3
    for r in res.values():
        q = r["q"]
        r["band_vs_plain"] = round(r["band_ms"] / plain["band_ms"], 3)
        if q == 0:
            continue
        r["projection_ms"] = round(r["stats_ms"] - plain["stats_ms"], 3)
        r["band_vs_annot_all_ones"] = None if annot_band is None else round(r["band_ms"] / annot_band, 3)
        r["projection_read_floor_ms"] = round(read_floor, 3)
        r["projection_fp64_tflops"] = round(6.0 * M * N * q / (r["projection_ms"] * 1e-3) / 1e12, 2)
        if args.fp64_tflops:
            flop_floor = 6.0 * M * N * q / (args.fp64_tflops * 1e12) * 1e3
            r["projection_flop_floor_ms"] = round(flop_floor, 3)
            r["projection_vs_floor"] = round(r["projection_ms"] / max(flop_floor, read_floor), 2)
        # the call outside the GPU stages: the basis checked on the host (finite, orthonormal, centred), laid out in
        # the projection kernel's tile order and uploaded from pageable memory
        r["host_and_upload_ms"] = round(r["median_ms"] - plain["median_ms"] - r["projection_ms"]
                                        - (r["band_ms"] - plain["band_ms"]), 3)
    doc = {"what": "nldsc_engine_run / nldsc_engine_run_covar on a resident C3 image: wall clock per synchronous call "
                   "(median of the repetitions after one warm-up); projection_ms = the statistics stage's GPU time "
                   "less the plain run's (the projection kernels run inside it), band_ms the band's (HIP events); "
                   "floors: one read of the image at hbm_gbs, 6 M N q flop at fp64_tflops",
           "n_org": N, "n_snp": M, "reps": args.reps, "image_bytes": image_bytes, "hbm_gbs": args.hbm_gbs,
           "fp64_tflops": args.fp64_tflops, "annot_all_ones_band_ms": annot_band,
           "device": torch.cuda.get_device_name(0), "runs": res}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
