#!/usr/bin/env python3
"""Engine.closest_rows + Result.closest (bg_closest_rows, bg_result_export_closest) on bench.py's
closest-features inputs (same generator and seeds, its row counts times --scale), against the two
other ways to the nearest rows. Timed in one process, alternating:

    rows    closest_rows (the scan) and Result.closest() (k_closest_export, four columns), timed
            separately, on a fresh result each step
    text    the only route without these calls: closest_op(dist=True) on the text tables and
            bg_result_format, the text left on the device (parsing it back is not included)
    torch   a nearest-neighbour in torch on the exported columns: two searchsorted over the query
            rows' keyed ends and starts. That is closest-features --no-overlaps on query rows none
            of which is nested in another (ends ascending with starts), so it runs on that subset
            of the query rows, loaded with load_columns, and is compared with
            closest_rows(no_overlaps=True) on the same tables

`rows` and `text` must agree on the whole input (the text is copied back once and a sample of
its lines, about 100,000 evenly spaced, is parsed and compared by coordinates), and `rows` and
`torch` on the subset (both asserted). Every buffer is sized by the tensors actually held (the
generator may return fewer or more rows than asked). Also reports k_closest_export's own time (HIP events, bg_prof_enable) beside its
algorithmic bytes. Prints one JSON line.

    python tools/bench_closest_columns.py [--steps K] [--warmup W] [--scale F] [--out FILE]
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
NA = -(1 << 63)  # bedgpu.h BG_DIST_NA


def torch_nearest(rc, rs, re, qc, qs, qe):
    """closest-features --no-overlaps --dist without the library, for query rows sorted by
    (chrom, start) whose ends ascend too: {"left", "right", "left_dist", "right_dist"}, sized by
    the columns given. Left: the last query row that ends at or before the reference row's start;
    right: the first after it that starts at or after its end; both on its chromosome."""
    import torch
    nq = int(qs.numel())
    rks, rke = (rc.long() << KEY_SHIFT) | rs, (rc.long() << KEY_SHIFT) | re
    qks, qke = (qc.long() << KEY_SHIFT) | qs, (qc.long() << KEY_SHIFT) | qe
    li = torch.searchsorted(qke, rks, right=True) - 1
    ri = torch.maximum(torch.searchsorted(qks, rke), li + 1)  # (a row at distance < 0 is the left's)
    safe = lambda i: i.clamp(0, max(nq - 1, 0))
    if nq == 0:
        none = torch.full_like(rs, -1)
        return {"left": none, "right": none.clone(), "left_dist": torch.full_like(rs, NA),
                "right_dist": torch.full_like(rs, NA)}
    okl = (li >= 0) & (qc[safe(li)].long() == rc.long())
    okr = (ri < nq) & (qc[safe(ri)].long() == rc.long())
    ld = -((rs - qe[safe(li)]) + 1)
    rd = (qs[safe(ri)] - re) + 1
    return {"left": torch.where(okl, li, -1), "right": torch.where(okr, ri, -1),
            "left_dist": torch.where(okl, ld, NA), "right_dist": torch.where(okr, rd, NA)}


def unnested(qc, qs, qe):
    """mask of the query rows that end after every row before them on their chromosome (the rows
    left have ends ascending with their starts)"""
    import torch
    ke = (qc.long() << KEY_SHIFT) | qe
    if int(ke.numel()) == 0:
        return torch.zeros(0, dtype=torch.bool, device=ke.device)
    run = torch.cummax(ke, 0).values
    keep = torch.ones_like(ke, dtype=torch.bool)
    keep[1:] = ke[1:] > run[:-1]
    # (a row of the next chromosome always passes: its key is above every key before it)
    return keep


def parse_lines(text, every):
    """every `every`-th line `ref|left|dL|right|dR` of the text route -> (row, dL, dR) with None
    for NA; the rows themselves are compared by coordinates, the text carries no index"""
    out = []
    for k, ln in enumerate(text.decode().split("\n")[:-1]):
        if k % every:
            continue
        f = ln.split("|")
        row = lambda t: None if t == "NA" else tuple(t.split("\t")[:3])
        out.append((k, row(f[1]), None if f[2] == "NA" else int(f[2]), row(f[3]), None if f[4] == "NA" else int(f[4])))
    return out


def _median(xs):
    ts = sorted(xs)
    return ts[len(ts) // 2] if len(ts) % 2 else 0.5 * (ts[len(ts) // 2 - 1] + ts[len(ts) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    steps, warmup = max(args.steps, 3), max(args.warmup, 1)

    import torch
    import bench
    from bedops_amd.engine import BED3, BED3_REST, Engine

    W = bench.WORKLOADS["closest"]
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
    s = eng.load([((b.data_ptr(), nb), BED3_REST) for b, nb in bufs])
    R, Q = s.columns(0), s.columns(1)
    rows = [int(R["start"].numel()), int(Q["start"].numel())]
    keep = unnested(Q["chrom"], Q["start"], Q["end"])
    U = {k: Q[k][keep].contiguous() for k in ("chrom", "start", "end")}
    rows_sub = int(U["start"].numel())
    sc = eng.load_columns([(R["names"], R["chrom"], R["start"], R["end"], BED3),
                           (Q["names"], U["chrom"], U["start"], U["end"], BED3)])
    bench.log(f"bench_closest_columns: {rows} rows, {rows_sub} query rows not nested")

    def timed(fn):
        eng.sync()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        eng.sync()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3, out

    def rows_step(keep_out=False, st=s, no=False):
        t_scan, r = timed(lambda: eng.closest_rows(st, 0, 1, no_overlaps=no))
        t_exp, c = timed(r.closest)
        r.free()
        return {"scan": t_scan, "export": t_exp}, (c if keep_out else None)

    def text_step(keep_out=False):
        t_scan, r = timed(lambda: eng.closest_op(s, 0, 1, dist=True))
        t_fmt, nbytes = timed(r.format)
        out = r.text() if keep_out else nbytes
        r.free()
        return {"scan": t_scan, "format": t_fmt}, out

    def torch_step(keep_out=False):
        t, out = timed(lambda: torch_nearest(R["chrom"], R["start"], R["end"], U["chrom"], U["start"], U["end"]))
        return {"nearest": t}, (out if keep_out else None)

    for _ in range(warmup):
        rows_step(), text_step(), torch_step()
    tr, tt, tj = [], [], []
    text_bytes = 0
    for _ in range(steps):  # alternating, so that every route sees the same neighbours
        a, _ = rows_step()
        b, text_bytes = text_step()
        c, _ = torch_step()
        tr.append(a), tt.append(b), tj.append(c)

    # rows against torch, on the tables without nested query rows
    _, got = rows_step(keep_out=True, st=sc, no=True)
    _, want = torch_step(keep_out=True)
    torch_equal = all(torch.equal(got[k], want[k]) for k in want)
    assert torch_equal, "closest_rows(no_overlaps) and the torch nearest-neighbour differ"
    del got, want
    # rows against the text route, on the whole input: a sample of the lines, by coordinates
    _, got = rows_step(keep_out=True)
    _, text = text_step(keep_out=True)
    every = max(1, rows[0] // 100000)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    qn, qc, qs, qe = Q["names"], Q["chrom"].cpu().numpy(), Q["start"].cpu().numpy(), Q["end"].cpu().numpy()
    name = lambda i: None if i < 0 else (qn[int(qc[i])], str(int(qs[i])), str(int(qe[i])))
    dist = lambda d: None if d == NA else d
    checked = 0
    for k, l, dl, r, dr in parse_lines(text, every):
        mine = (k, name(int(g["left"][k])), dist(int(g["left_dist"][k])), name(int(g["right"][k])),
                dist(int(g["right_dist"][k])))
        assert mine == (k, l, dl, r, dr), f"row {k}: columns {mine[1:]} against text {(l, dl, r, dr)}"
        checked += 1
    del got, text, g

    # the export kernel alone (HIP events slow the host side): keys, left and right read, four
    # columns written, per reference row; the gathers re-read query keys that lanes share
    exp_bytes = (4 * 8 + 4 * 8) * rows[0]
    eng.prof_enable("*")
    rows_step()
    prof = eng.prof_read()
    eng.prof_enable("")
    table = {k: [v[0], round(v[1], 4)] for k, v in sorted(prof.items(), key=lambda kv: -kv[1][1])}
    calls, ms = prof.get("k_closest_export", (0, 0.0))
    kern = {"kernel": "k_closest_export", "launches": calls, "total_ms": round(ms, 4),
            "bytes_streamed": exp_bytes, "bytes_gathered_at_most": 4 * 8 * rows[0],
            "hbm_fraction_streamed": round(exp_bytes / (ms * 1e-3) / HBM_BYTES_PER_S, 4) if ms else None}
    sc.free()
    s.free()
    eng.close()

    def summary(ts):
        return {k: {"median_ms": round(_median([t[k] for t in ts]), 4), "min_ms": round(min(t[k] for t in ts), 4),
                    "max_ms": round(max(t[k] for t in ts), 4)} for k in ts[0]}

    res = {"tool": "bench_closest_columns", "workload": "closest inputs of bench.py", "scale": args.scale,
           "rows": rows, "query_rows_not_nested": rows_sub, "steps": steps, "warmup": warmup,
           "rows_route": summary(tr), "text_route": dict(summary(tt), text_bytes=int(text_bytes)),
           "torch_route": summary(tj), "rows_equal_torch": bool(torch_equal), "text_lines_checked": checked,
           "export_kernel": kern, "kernels_launches_ms": table}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
