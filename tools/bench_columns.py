#!/usr/bin/env python3
"""The columnar step on bench.py's intersect inputs (same generator, seeds and row counts):

    load_columns (BED3_SET) -> intersect -> Result.columns()

against the text step bench.py times (bg_load of BED text -> intersect -> format). The inputs
are loaded once as rows from the generated text and taken back as device columns with
InputSet.columns (the text -> columns bridge); that set and the text are freed before the
clock starts. Also reports k_cols_key alone (HIP events, bg_prof_enable) with its fraction of
the HBM roofline from its algorithmic bytes, and checks that the columnar result still formats
to bench.py's reference text. Prints one JSON line.

    python tools/bench_columns.py [--steps K] [--warmup W] [--scale F] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12  # MI355X
KEY_BYTES_PER_ROW = 20 + 16  # int32 + 2 x int64 read, 2 x int64 written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    import bench
    from bedops_amd.engine import BED3, BED3_SET, Engine

    W = bench.WORKLOADS["intersect"]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    L = bench.bedgen_lib()
    mask = (1 << len(bench.contigs(L))) - 1
    inputs = []
    for (seed, mode), n in zip(W["gen"], W["rows"]):
        p, nb, _ = bench.gen(L, int(n * args.scale), seed, mask, mode)
        buf = bench.to_device(torch, p, nb, dev)
        L.bedgen_free(p)
        torch.cuda.synchronize(dev)
        s = eng.load([((buf.data_ptr(), nb), BED3)])
        c = s.columns(0)
        s.free()
        eng.sync()
        del buf
        inputs.append((c["names"], c["chrom"], c["start"], c["end"], BED3_SET))
    rows = [int(i[1].numel()) for i in inputs]
    bench.log(f"bench_columns: {rows} rows as device columns")

    def step(keep=False):
        s = eng.load_columns(inputs)
        r = eng.op("-i", s, [0, 1])
        cols = r.columns()
        n = int(cols["start"].numel())
        text = r.text() if keep else None
        r.free()
        s.free()
        return n, text

    for _ in range(max(args.warmup, 2)):
        step()
    times = []
    for _ in range(args.steps):
        eng.sync()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out_rows, _ = step()
        eng.sync()
        times.append(time.perf_counter() - t0)
    eng.prof_enable("k_cols_key")
    step()
    calls, ms = eng.prof_read().get("k_cols_key", (0, 0.0))
    eng.prof_enable("*")  # every kernel of one warm step (HIP events slow the host side)
    step()
    table = {k: [v[0], round(v[1], 4)] for k, v in sorted(eng.prof_read().items(), key=lambda kv: -kv[1][1])}
    eng.prof_enable("")
    _, text = step(keep=True)
    sha = hashlib.sha256(text).hexdigest()[:16]
    eng.close()

    ts = sorted(times)
    med = ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])
    key_bytes = KEY_BYTES_PER_ROW * sum(rows)
    res = {"tool": "bench_columns", "workload": "intersect", "rows": rows, "steps": args.steps,
           "step": "load_columns(BED3_SET) -> intersect -> Result.columns()",
           "median_s": round(med, 6), "min_s": round(ts[0], 6), "max_s": round(ts[-1], 6),
           "runs_s": [round(t, 6) for t in times], "out_rows": out_rows,
           "intervals_per_s": round(sum(rows) / med, 1),
           "k_cols_key": {"launches": calls, "total_ms": round(ms, 4), "bytes": key_bytes,
                          "hbm_fraction": round(key_bytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4) if ms else None},
           "kernels_launches_ms": table, "output_sha16": sha,
           "matches_reference": (sha == W["ref"]["sha16"]) if args.scale == 1.0 else None}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
