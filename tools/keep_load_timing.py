"""Cost of loading a subset of the individuals (nldsc_engine_set_keep) against the plain load, on the C3 image.

The image (synth.device_bed, N = 315 599, M = 80 000) stays in device memory; each variant of
`nldsc_engine_load_bed_device` runs once to warm up and then `--reps` times, each call synchronous (the loader returns
after its kernels), wall clock around the call.  Variants: the plain load (no list), keep-everyone, a random half,
the first half (contiguous).  Medians go to `--out` (profiles/keep_load_c3.json), with the `load` figure of a
`bench.py --full` line of the same box when `--bench-json` names a file holding that line.

    python tools/keep_load_timing.py --out profiles/keep_load_c3.json [--bench-json bench_full.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def bench_load_ms(path):
    """oneshot_gpu_ms.load of the last JSON line of `path` that carries it."""
    found = None
    for line in open(path):
        line = line.strip()
        if not line.startswith("{"):
            continue
        try:
            doc = json.loads(line)
        except ValueError:
            continue
        stack = [doc]
        while stack:
            d = stack.pop()
            if isinstance(d, dict):
                if isinstance(d.get("oneshot_gpu_ms"), dict) and "load" in d["oneshot_gpu_ms"]:
                    found = float(d["oneshot_gpu_ms"]["load"])
                stack.extend(d.values())
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-org", type=int, default=315_599)
    ap.add_argument("--n-snp", type=int, default=80_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-json", default=None, help="file holding a `bench.py --full` result line of this box")
    ap.add_argument("--parent-load-ms", type=float, default=None,
                    help="the parent commit's oneshot_gpu_ms.load, when it was measured apart")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from nldsc_amd import synth
    from nldsc_amd.engine import Engine
    N, M = args.n_org, args.n_snp
    img, _ = synth.device_bed(M, N)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    lists = {"plain": None, "keep_everyone": np.arange(N, dtype=np.int32),
             "keep_random_half": np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32),
             "keep_first_half": np.arange(N // 2, dtype=np.int32)}
    res = {}
    with Engine(0) as e:
        for name, idx in lists.items():
            e.set_keep(idx, N)
            ms = []
            for k in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.load_bed_device(img.data_ptr(), img.numel(), M, N)
                ms.append(1e3 * (time.perf_counter() - t0))
            res[name] = {"n_keep": int(e.n_org), "median_ms": round(statistics.median(ms[1:]), 3),
                         "all_ms": [round(v, 3) for v in ms[1:]], "warmup_ms": round(ms[0], 3)}
        e.set_keep(None)
    plain = res["plain"]["median_ms"]
    nb = (N + 3) // 4
    for name, r in res.items():
        r["vs_plain"] = round(r["median_ms"] / plain, 3)
        nbk = (r["n_keep"] + 3) // 4
        # bytes moved: the plain load reads and writes the rows once; a keep-load reads the source, writes and
        # re-reads the compact rows, and writes the image of the kept
        r["bytes_vs_plain"] = 1.0 if name == "plain" else round((nb + 3 * nbk) / (2 * nb), 3)
    doc = {"what": "nldsc_engine_load_bed_device of a C3 image in device memory: plain, and with a keep list "
                   "(subset_samples_kernel + the unchanged load of the compact rows); wall clock per synchronous "
                   "call, median of the repetitions after one warm-up",
           "n_org": N, "n_snp": M, "reps": args.reps, "device": torch.cuda.get_device_name(0), "loads": res,
           "target": "keep_random_half <= 1.5 x plain", "target_met": res["keep_random_half"]["vs_plain"] <= 1.5}
    if args.bench_json:
        doc["bench_full_oneshot_load_ms"] = bench_load_ms(args.bench_json)
    if args.parent_load_ms is not None:
        doc["parent_commit_oneshot_load_ms"] = args.parent_load_ms
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
