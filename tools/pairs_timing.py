"""Cost of the pairwise LD table (nldsc_engine_run_pairs) against the plain run, on a resident C3 image.

The image (synth.device_bed, N = 315 599, M = 80 000, 1 % missing calls, the bench's run parameters) is loaded once;
each configuration runs once to warm up and then `--reps` times, each call synchronous, wall clock around it and the
engine's own stage timings beside it.  Configurations: the plain run; an annotated run with one all-ones column (what
the trip of the Gram tiles through memory and a second epilogue cost); the sizing call alone (count pass, no table); a
full pairs run without a filter — the sizing call, then one emitting call per owned range of at most `--budget` pairs;
the same with min_r2 = 0.2.  Per configuration: the wall clock, the band's GPU span (HIP events around the band: in a
pairs run it holds the host's two waits and the upload of row_ptr), and the rest of the calls — for an emitting call
mostly the copies of k, r, rd into pageable host arrays.  Medians go to `--out` (profiles/pairs_c3.json).

    python tools/pairs_timing.py --out profiles/pairs_c3.json
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget", type=int, default=32 * 1024 * 1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from nldsc_amd import _lib, synth
    from nldsc_amd.engine import Engine
    N, M = args.n_org, args.n_snp
    img, pos = synth.device_bed(M, N)
    torch.cuda.synchronize()
    run_args = (1.0, 1e-4, 1e-5, 1.0 / M)
    res = {}
    with Engine(0) as e:
        e.load_bed_device(img.data_ptr(), img.numel(), M, N)
        del img
        torch.cuda.empty_cache()

        def timed(call):
            """one synchronous engine call: (result, wall ms, band ms, finalize ms)"""
            t0 = time.perf_counter()
            out = call()
            ms = 1e3 * (time.perf_counter() - t0)
            tim = e.timings()
            return out, ms, tim["band_ms"], tim["finalize_ms"], tim, tim["total_ms"], tim["count_ms"] + tim["stats_ms"]

        def plain():
            return [timed(lambda: e.run(*run_args, pos))[1:]]

        def annot():
            ones = np.ones((M, 1))
            return [timed(lambda: e.run(*run_args, pos, annot=ones))[1:]]

        def sizing(min_r2=None):
            return [timed(lambda: e.size_pairs(*run_args, pos, min_r2=min_r2))[1:]]

        def full(min_r2=None):
            s, *first = timed(lambda: e.size_pairs(*run_args, pos, min_r2=min_r2))
            calls, pairs = [tuple(first)], 0
            for lo, hi in _lib.pairs_split_ranges(s["row_ptr"], args.budget):
                cap = int(s["row_ptr"][hi] - s["row_ptr"][lo])
                t, *rest = timed(lambda: e._pairs(*run_args, pos, (lo, hi), 0, min_r2, emit=True, cap=cap))
                assert t["n_pairs"] == cap
                pairs += cap
                calls.append(tuple(rest))
            full.pairs = pairs
            return calls

        cases = {"plain": plain, "annot_1_all_ones": annot, "pairs_sizing_only": sizing, "pairs_full": full,
                 "pairs_full_min_r2_0.2": lambda: full(0.2)}
        for name, fn in cases.items():
            runs = [fn() for _ in range(args.reps + 1)]
            wall = [sum(c[0] for c in r) for r in runs]
            band = [sum(c[1] for c in r) for r in runs]
            fin = [sum(c[2] for c in r) for r in runs]
            tim = runs[-1][-1][3]
            res[name] = {"engine_calls": len(runs[-1]), "median_ms": round(statistics.median(wall[1:]), 3),
                         "all_ms": [round(v, 3) for v in wall[1:]], "warmup_ms": round(wall[0], 3),
                         "band_ms": round(statistics.median(band[1:]), 3),
                         "finalize_ms": round(statistics.median(fin[1:]), 3),
                         "per_call_ms": [round(c[0], 3) for c in runs[-1]],
                         "per_call_band_ms": [round(c[1], 3) for c in runs[-1]],
                         "per_call_engine_total_ms": [round(c[4], 3) for c in runs[-1]],
                         "per_call_count_stats_ms": [round(c[5], 3) for c in runs[-1]],
                         "band_items_last_call": tim["band_items"], "ksplit_last_call": tim["ksplit"]}
            if name.startswith("pairs_full"):
                res[name]["pairs"] = full.pairs
                res[name]["table_bytes"] = 20 * full.pairs
    base = res["plain"]
    for r in res.values():
        r["vs_plain"] = round(r["median_ms"] / base["median_ms"], 3)
        r["band_vs_plain"] = round(r["band_ms"] / base["band_ms"], 3)
        r["outside_band_ms"] = round(r["median_ms"] - r["band_ms"] - r["finalize_ms"], 3)
    doc = {"what": "nldsc_engine_run / _run_annot / _run_pairs on a resident C3 image: wall clock of the synchronous "
                   "engine calls of one configuration (median of the repetitions after one warm-up), the band's GPU "
                   "span (HIP events; in a pairs run it holds the host's waits for the window width and the row "
                   "lengths) and the rest of the calls (for emitting calls: the copies of the table to the host)",
           "n_org": N, "n_snp": M, "reps": args.reps, "budget": args.budget,
           "device": torch.cuda.get_device_name(0), "runs": res}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
