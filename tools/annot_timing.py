"""Cost of partitioned LD scores (nldsc_engine_run_annot) against the plain run, on a resident C3 image.

The image (synth.device_bed, N = 315 599, M = 80 000, 1 % missing calls, the bench's run parameters) is loaded once;
each case runs once to warm up and then `--reps` times, each call synchronous (the engine returns with the results on
the host), wall clock around the call and the engine's own stage timings beside it.  Cases: the plain run; an
annotated run with one all-ones column; with 8 binary columns at 10 % density; with 64 such columns.  Medians go to
`--out` (profiles/annot_c3.json), each case's time against the plain run's of the same process.

    python tools/annot_timing.py --out profiles/annot_c3.json
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from nldsc_amd import synth
    from nldsc_amd.engine import Engine
    N, M = args.n_org, args.n_snp
    img, pos = synth.device_bed(M, N)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    cases = {"plain": None, "annot_1_all_ones": np.ones((M, 1)),
             "annot_8_binary_10pct": (rng.random((M, 8)) < 0.1).astype(np.float64),
             "annot_64_binary_10pct": (rng.random((M, 64)) < 0.1).astype(np.float64)}
    run_args = (1.0, 1e-4, 1e-5, 1.0 / M)
    res = {}
    with Engine(0) as e:
        e.load_bed_device(img.data_ptr(), img.numel(), M, N)
        del img
        torch.cuda.empty_cache()
        for name, annot in cases.items():
            ms, band, fin, tim = [], [], [], {}
            for k in range(args.reps + 1):
                t0 = time.perf_counter()
                e.run(*run_args, pos, annot=annot)
                ms.append(1e3 * (time.perf_counter() - t0))
                tim = e.timings()
                band.append(tim["band_ms"])
                fin.append(tim["finalize_ms"])
            res[name] = {"n_annot": 0 if annot is None else annot.shape[1],
                         "median_ms": round(statistics.median(ms[1:]), 3), "all_ms": [round(v, 3) for v in ms[1:]],
                         "warmup_ms": round(ms[0], 3), "band_ms": round(statistics.median(band[1:]), 3),
                         "finalize_ms": round(statistics.median(fin[1:]), 3), "band_items": tim["band_items"],
                         "band_kernel": tim["band_kernel"], "ksplit": tim["ksplit"]}
    plain = res["plain"]
    for r in res.values():
        r["vs_plain"] = round(r["median_ms"] / plain["median_ms"], 3)
        r["band_vs_plain"] = round(r["band_ms"] / plain["band_ms"], 3)
        # what the call spends outside the band and finalize: the upload of the annotation matrix (pageable memory,
        # synchronous), the accumulators' memset, the copies of the [C][M] results
        r["outside_band_ms"] = round(r["median_ms"] - r["band_ms"] - r["finalize_ms"], 3)
    doc = {"what": "nldsc_engine_run / nldsc_engine_run_annot on a resident C3 image: wall clock per synchronous call "
                   "(median of the repetitions after one warm-up), the band's and finalize's GPU time (HIP events) and "
                   "the rest of the call",
           "n_org": N, "n_snp": M, "reps": args.reps, "device": torch.cuda.get_device_name(0), "runs": res}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
