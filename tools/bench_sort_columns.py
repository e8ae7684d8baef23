#!/usr/bin/env python3
"""Engine.sort_columns (bg_sort_columns) against the torch route on bench.py's intersect inputs
(same generator, seeds and row counts): the inputs are loaded once as text and taken back as
device columns with InputSet.columns, as tools/bench_columns.py does; then their rows are
shuffled and their name list is put out of strcmp order (`shuffled`, below). Timed, in one
process and alternating, on the same tensors:

    engine  Engine.sort_columns(names, chrom, start, end) of every input
    torch   rank lookup, then stable torch.sort by end, by start, by rank, and the gathers

The two results are compared for equality. Also reports k_sc_key and k_sc_gather alone (HIP
events, bg_prof_enable) with their share of the HBM roofline from their algorithmic bytes, and
every kernel of one profiled call. "Not slower" means: the engine's median is at or below the
torch median plus the torch route's own spread (max - min) in this session. Prints one JSON line.

    python tools/bench_sort_columns.py [--steps K] [--warmup W] [--scale F] [--out FILE]
"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12  # MI355X
KEY_BYTES_PER_ROW = 20  # int32 + 2 x int64 read
GATHER_BYTES_PER_ROW = 4 + 20 + 8 + 20  # payload and the gathered row read; order and the row written


def shuffled(names, cols, seed):
    """(names', cols', perm): the rows of `cols` = [chrom, start, end(, score)] (torch tensors on
    any device) in the order perm, a seeded permutation of range(cols[0].numel()), with `names`
    reordered by the same seed and chrom re-indexed to match. Everything is sized by the tensors
    themselves: a row count asked of a generator never comes here (generators may return fewer
    rows than asked). Lengths and chrom's range are checked on the host before any indexing."""
    import torch
    n = int(cols[0].numel())
    for k, c in enumerate(cols):
        if c.dim() != 1 or int(c.numel()) != n:
            raise ValueError(f"shuffled: column {k} has shape {tuple(c.shape)}, column 0 has {n} rows")
    if n and not (0 <= int(cols[0].min()) and int(cols[0].max()) < len(names)):
        raise ValueError("shuffled: chrom index outside names")
    g = torch.Generator()
    g.manual_seed(seed)
    perm = torch.randperm(n, generator=g).to(cols[0].device)
    q = list(range(len(names)))
    random.Random(seed).shuffle(q)  # names'[j] = names[q[j]]
    if len(q) > 1 and [names[j] for j in q] == sorted(names, key=lambda s: s.encode()):
        q = q[1:] + q[:1]  # (never leave the list in strcmp order)
    inv = torch.empty(max(len(q), 1), dtype=cols[0].dtype)
    inv[torch.tensor(q, dtype=torch.int64)] = torch.arange(len(q), dtype=cols[0].dtype)
    out = [c[perm] for c in cols]
    out[0] = inv.to(cols[0].device)[out[0].long()]
    return [names[j] for j in q], out, perm


def torch_route(rank, chrom, start, end):
    """the route without the library: order and the sorted columns by three stable sorts"""
    import torch
    r = rank[chrom.long()]
    o = torch.sort(end, stable=True).indices
    o = o[torch.sort(start[o], stable=True).indices]
    o = o[torch.sort(r[o], stable=True).indices]
    return {"order": o, "chrom": chrom[o], "start": start[o], "end": end[o]}


def _median(xs):
    ts = sorted(xs)
    return ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    steps, warmup = max(args.steps, 10), max(args.warmup, 2)

    import torch
    import bench
    from bedops_amd.engine import BED3, Engine

    W = bench.WORKLOADS["intersect"]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    L = bench.bedgen_lib()
    mask = (1 << len(bench.contigs(L))) - 1
    inputs = []
    for k, ((seed, mode), n) in enumerate(zip(W["gen"], W["rows"])):
        p, nb, _ = bench.gen(L, int(n * args.scale), seed, mask, mode)
        buf = bench.to_device(torch, p, nb, dev)
        L.bedgen_free(p)
        torch.cuda.synchronize(dev)
        s = eng.load([((buf.data_ptr(), nb), BED3)])
        c = s.columns(0)
        s.free()
        eng.sync()
        del buf
        names, cols, _ = shuffled(c["names"], [c["chrom"], c["start"], c["end"]], seed=1000 + k)
        del c
        by = sorted(range(len(names)), key=lambda j: names[j].encode())
        rank = torch.empty(len(names), dtype=torch.int64)
        rank[torch.tensor(by, dtype=torch.int64)] = torch.arange(len(names), dtype=torch.int64)
        inputs.append((names, cols, rank.to(dev)))
    torch.cuda.synchronize(dev)
    rows = [int(cols[0].numel()) for _, cols, _ in inputs]
    bench.log(f"bench_sort_columns: {rows} shuffled rows as device columns")

    def engine_step():
        return [eng.sort_columns(names, *cols) for names, cols, _ in inputs]

    def torch_step():
        out = [torch_route(rank, *cols) for _, cols, rank in inputs]
        torch.cuda.synchronize(dev)
        return out

    def timed(fn):
        eng.sync()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    for _ in range(warmup):
        engine_step()
        torch_step()
    te, tt = [], []
    for _ in range(steps):  # alternating, so that both routes see the same neighbours
        te.append(timed(engine_step)[0])
        tt.append(timed(torch_step)[0])
    _, got = timed(engine_step)
    _, want = timed(torch_step)
    equal = all(torch.equal(g[k], w[k]) for g, w in zip(got, want) for k in ("order", "chrom", "start", "end"))
    del got, want

    alone = {}
    for name, per_row in (("k_sc_key", KEY_BYTES_PER_ROW), ("k_sc_gather", GATHER_BYTES_PER_ROW)):
        eng.prof_enable(name)
        engine_step()
        calls, ms = eng.prof_read().get(name, (0, 0.0))
        nbytes = per_row * sum(rows)
        alone[name] = {"launches": calls, "total_ms": round(ms, 4), "bytes": nbytes,
                       "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4) if ms else None}
    eng.prof_enable("*")  # every kernel of one warm step (HIP events slow the host side)
    engine_step()
    table = {k: [v[0], round(v[1], 4)] for k, v in sorted(eng.prof_read().items(), key=lambda kv: -kv[1][1])}
    eng.prof_enable("")
    eng.close()

    me, mt = _median(te), _median(tt)
    spread = max(tt) - min(tt)
    res = {"tool": "bench_sort_columns", "workload": "intersect inputs, rows shuffled, names out of strcmp order",
           "rows": rows, "names": [len(i[0]) for i in inputs], "steps": steps, "warmup": warmup,
           "step": "every input: order + chrom, start, end in sort-bed order",
           "engine": {"route": "Engine.sort_columns", "median_s": round(me, 6), "min_s": round(min(te), 6),
                      "max_s": round(max(te), 6), "runs_s": [round(t, 6) for t in te]},
           "torch": {"route": "rank lookup + stable torch.sort by end, start, rank + gathers",
                     "median_s": round(mt, 6), "min_s": round(min(tt), 6), "max_s": round(max(tt), 6),
                     "runs_s": [round(t, 6) for t in tt]},
           "torch_spread_s": round(spread, 6), "engine_over_torch": round(me / mt, 4) if mt else None,
           "not_slower": me <= mt + spread, "results_equal": bool(equal),
           "rows_per_s": round(sum(rows) / me, 1) if me else None,
           "kernels_alone": alone, "kernels_launches_ms": table}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
