#!/usr/bin/env python3
"""Result.pairs (bg_result_map_pairs + bg_result_export_map_pairs) on bench.py's bedmap inputs
(same generator, seeds and row counts, times --scale), against the two other ways to the
(reference row, map row) index pairs of bedmap --bp-ovr 1. Timed in one process, alternating:

    pairs   the count (offsets, one scan) and the export (the fill kernel), timed separately, on a
            fresh bedmap --count result each step
    text    the only route without these calls: bedmap --echo-map-id on the text tables and
            bg_result_format, the text left on the device (parsing it back is not included)
    torch   a join in torch on the exported columns: searchsorted bounds from the map table's
            longest row, repeat_interleave over the candidate ranges, then the overlap mask

`pairs` and `torch` must give identical pairs (asserted). Every buffer is sized by the tensors
actually produced (generators may return fewer rows than asked). Also reports every kernel of
one profiled step (HIP events, bg_prof_enable) and the fill kernel's share of the HBM roofline
from its algorithmic bytes. Prints one JSON line.

    python tools/bench_map_pairs.py [--steps K] [--warmup W] [--scale F] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12  # MI355X
KEY_SHIFT = 40  # bg_internal.h BG_KEY_SHIFT


def torch_join(rc, rs, re, mc, ms, me):
    """the pairs of --bp-ovr 1 without the library: (offsets, ref_rows, map_rows), all sized by
    the columns given; rows sorted by (chrom, start), no zero-length rows"""
    import torch
    nr = int(rs.numel())
    rks, rke = (rc.long() << KEY_SHIFT) | rs, (rc.long() << KEY_SHIFT) | re
    mks = (mc.long() << KEY_SHIFT) | ms
    longest = int((me - ms).max()) if int(ms.numel()) else 1
    g = rc.long() << KEY_SHIFT
    lo = torch.searchsorted(mks, torch.maximum(g, rks - longest + 1))
    hi = torch.maximum(torch.searchsorted(mks, rke), lo)
    lens = hi - lo
    first = torch.cumsum(lens, 0) - lens
    ref = torch.repeat_interleave(torch.arange(nr, device=rs.device), lens)
    cand = torch.arange(int(ref.numel()), device=rs.device) - first[ref] + lo[ref]
    keep = (torch.minimum(re[ref], me[cand]) - torch.maximum(rs[ref], ms[cand])) >= 1
    ref, cand = ref[keep], cand[keep]
    off = torch.zeros(nr + 1, dtype=torch.int64, device=rs.device)
    off[1:] = torch.cumsum(torch.bincount(ref, minlength=nr), 0)
    return off, ref, cand


def _median(xs):
    ts = sorted(xs)
    return ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    steps, warmup = max(args.steps, 3), max(args.warmup, 1)

    import torch
    import bench
    from bedops_amd.engine import BED3_REST, BED5_REST, Engine

    W = bench.WORKLOADS["bedmap"]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    L = bench.bedgen_lib()
    mask = (1 << len(bench.contigs(L))) - 1
    bufs = []
    for (seed, mode), n in zip(W["gen"], W["rows"]):
        p, nb, _ = bench.gen(L, int(n * args.scale), seed, mask, mode)
        bufs.append((bench.to_device(torch, p, nb, dev), nb))
        L.bedgen_free(p)
    torch.cuda.synchronize(dev)
    # text tables with their remainders (the text route echoes ids); the same tables serve all routes
    s = eng.load([((bufs[0][0].data_ptr(), bufs[0][1]), BED3_REST), ((bufs[1][0].data_ptr(), bufs[1][1]), BED5_REST)])
    R, M = s.columns(0), s.columns(1)
    rows = [int(R["start"].numel()), int(M["start"].numel())]
    bench.log(f"bench_map_pairs: {rows} rows")

    def timed(fn):
        eng.sync()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    def pairs_step(keep=False):
        t_map, r = timed(lambda: eng.map_op(s, ["count"], 0, 1))
        t_cnt, total = timed(r.pairs_total)
        t_exp, p = timed(r.pairs)
        r.free()
        return {"map": t_map, "count": t_cnt, "export": t_exp}, (p if keep else int(total))

    def text_step():
        t_map, r = timed(lambda: eng.map_op(s, ["echo-map-id"], 0, 1))
        t_fmt, nbytes = timed(r.format)
        r.free()
        return {"map": t_map, "format": t_fmt}, nbytes

    def torch_step(keep=False):
        t, out = timed(lambda: torch_join(R["chrom"], R["start"], R["end"], M["chrom"], M["start"], M["end"]))
        return {"join": t}, (out if keep else None)

    for _ in range(warmup):
        pairs_step(), text_step(), torch_step()
    tp, tt, tj = [], [], []
    total = text_bytes = 0
    for _ in range(steps):  # alternating, so that every route sees the same neighbours
        a, total = pairs_step()
        b, text_bytes = text_step()
        c, _ = torch_step()
        tp.append(a), tt.append(b), tj.append(c)
    _, got = pairs_step(keep=True)
    _, want = torch_step(keep=True)
    equal = (torch.equal(got["offsets"], want[0]) and torch.equal(got["ref_rows"], want[1]) and
             torch.equal(got["map_rows"], want[2]))
    assert equal, "Result.pairs and the torch join give different pairs"
    del got, want

    # the fill kernel alone, then every kernel of one step (HIP events slow the host side)
    fill_bytes = 16 * total + 16 * rows[1] + 24 * rows[0]  # pairs written; map keys, ref keys + offsets read once
    eng.prof_enable("*")
    pairs_step()
    prof = eng.prof_read()
    eng.prof_enable("")
    table = {k: [v[0], round(v[1], 4)] for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
    kern = "k_pairs_flat" if "k_pairs_flat" in prof else "k_pairs_rows"  # (long map rows: the per-row kernel)
    calls, ms = prof.get(kern, (0, 0.0))
    fill = {"kernel": kern, "launches": calls, "total_ms": round(ms, 4), "bytes": fill_bytes,
            "hbm_fraction": round(fill_bytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4) if ms else None}
    s.free()
    eng.close()

    def summary(ts):
        return {k: {"median_ms": round(_median([t[k] for t in ts]), 4), "min_ms": round(min(t[k] for t in ts), 4),
                    "max_ms": round(max(t[k] for t in ts), 4)} for k in ts[0]}

    res = {"tool": "bench_map_pairs", "workload": "bedmap inputs, --bp-ovr 1", "scale": args.scale, "rows": rows,
           "pairs": total, "steps": steps, "warmup": warmup,
           "pairs_route": summary(tp), "text_route": dict(summary(tt), text_bytes=int(text_bytes)),
           "torch_route": summary(tj), "results_equal": bool(equal),
           "fill_kernel": fill, "kernels_launches_ms": table}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
