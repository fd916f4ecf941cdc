"""Cost of the dominance-by-dominance LD scores (nldsc_engine_run_domdom) on a resident C3 image.

The image (synth.device_bed, N = 315 599, M = 80 000, 1 % missing calls, the bench's run parameters) is loaded once.
Three cases run in one process, interleaved (plain, annotated, dom-dom, plain, ...), once to warm up and then `--reps`
times, each call synchronous, wall clock around the call and the engine's own stage timings beside it:

  plain        nldsc_engine_run: the default band kernels and their schedule;
  annot_1      nldsc_engine_run_annot with one all-ones column: every block pair through the K-split partial kernel
               (8 products) and a feature epilogue — the route a dom-dom run takes, one product fewer;
  domdom       nldsc_engine_run_domdom: the partial kernel with the ninth product h.h, the dom-dom epilogue.

The fair yardstick of the dom-dom band is the annotated one (`band_vs_annot_1`; the products alone would make it 9/8).
Medians go to `--out` (profiles/domdom_timing_c3.json).

    python tools/domdom_timing.py --out profiles/domdom_timing_c3.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-org", type=int, default=315_599)
    ap.add_argument("--n-snp", type=int, default=80_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from nldsc_amd import synth
    from nldsc_amd.engine import Engine
    N, M = args.n_org, args.n_snp
    img, pos = synth.device_bed(M, N)
    torch.cuda.synchronize()
    run_args = (1.0, 1e-4, 1e-5, 1.0 / M)
    ones = np.ones((M, 1))
    with Engine(0) as e:
        e.load_bed_device(img.data_ptr(), img.numel(), M, N)
        del img
        torch.cuda.empty_cache()
        cases = {"plain": lambda: e.run(*run_args, pos), "annot_1": lambda: e.run(*run_args, pos, annot=ones),
                 "domdom": lambda: e.run_domdom(*run_args, pos)}
        rec = {name: {"ms": [], "band": [], "fin": [], "tim": {}} for name in cases}
        last = {}
        for k in range(args.reps + 1):
            for name, call in cases.items():
                t0 = time.perf_counter()
                last[name] = call()
                r = rec[name]
                r["ms"].append(1e3 * (time.perf_counter() - t0))
                r["tim"] = e.timings()
                r["band"].append(r["tim"]["band_ms"])
                r["fin"].append(r["tim"]["finalize_ms"])
    res = {}
    for name, r in rec.items():
        tim = r["tim"]
        res[name] = {"median_ms": round(statistics.median(r["ms"][1:]), 3), "all_ms": [round(v, 3) for v in r["ms"][1:]],
                     "warmup_ms": round(r["ms"][0], 3), "band_ms": round(statistics.median(r["band"][1:]), 3),
                     "all_band_ms": [round(v, 3) for v in r["band"][1:]],
                     "finalize_ms": round(statistics.median(r["fin"][1:]), 3), "band_items": tim["band_items"],
                     "band_kernel": tim["band_kernel"], "ksplit": tim["ksplit"],
                     "flop_issued": tim["flop_issued"]}
    for r in res.values():
        r["vs_plain"] = round(r["median_ms"] / res["plain"]["median_ms"], 3)
        r["band_vs_plain"] = round(r["band_ms"] / res["plain"]["band_ms"], 3)
        r["band_vs_annot_1"] = round(r["band_ms"] / res["annot_1"]["band_ms"], 3)
    dd = last["domdom"]["l2dd"]
    doc = {"what": "nldsc_engine_run / _run_annot (one column) / _run_domdom on a resident C3 image, interleaved in one "
                   "process: wall clock per synchronous call (median of the repetitions after one warm-up) and the "
                   "band's and finalize's GPU time (HIP events); band_vs_annot_1 compares the dom-dom band with the "
                   "same K-split route at 8 products",
           "n_org": N, "n_snp": M, "reps": args.reps, "device": torch.cuda.get_device_name(0), "runs": res,
           "l2dd": {"finite": int(np.isfinite(dd).sum()), "mean": float(np.nanmean(dd)), "max": float(np.nanmax(dd))},
           "ordinary_arrays_bitwise_default_plain": bool(all(
               np.array_equal(last["domdom"][k], last["plain"][k], equal_nan=True)
               for k in ("l2", "l2d", "maf", "residuals_std", "l2_ws", "l2d_ws", "l2d_wse")))}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
