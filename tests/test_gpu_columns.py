"""The columnar interface (bg_load_columns, bg_set_export_rows, bg_result_export_*): the same
data loaded as BED text and as numeric columns gives the same answer, as text and as columns,
so the sweep kernels are checked once more without the parser and the formatter in between.

Shapes: 1,500-row files over 4 chromosomes for the operations; for the ingest kernel, row
counts around every boundary it has (a lane's 4 rows, a wave's 256, a workgroup round of
BG_COLS_CHUNK rows, several rounds per workgroup through BEDGPU_COLS_BLOCKS) with more than
70 chromosomes whose order in `names` is not their strcmp order, chromosome changes on a wave
boundary, a round boundary and the last row, and coordinates above 2^32 and at the key limit."""
import os
import random
import re

import numpy as np
import pytest
import torch

import randbed
from conftest import ROOT

pytestmark = pytest.mark.gpu

# A torch wheel that bundles its own HIP runtime finds no device once libbedgpu's runtime has
# initialised it: a process that uses both starts torch's first, as
# bench.py does. In a whole-suite run other modules open engines before this module's tests
# run, and no fixture of this module can come before them, so torch's runtime is started
# here, when the module is collected; without a GPU this does nothing. The `eng` fixture
# checks that it is up and says so clearly otherwise.
if torch.cuda.is_available():
    torch.cuda.init()

BED3, BED5, BED3_SET = 0, 2, 3
UNSORTED, RANGE, ARG, NOMEM, UNSUPPORTED, CHROM = -3, -4, -6, -7, -8, -9
COORD_MAX = (1 << 40) - 1


def _define(path, name):
    src = open(os.path.join(ROOT, "bedops_amd", "csrc", path)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


# rows a workgroup of k_cols_key keys per round (BG_COLS_CHUNK = BG_NT * CK_ROWS), rows per wave
NT = _define("bg_internal.h", "BG_NT")
LANE_ROWS = _define("bg_columns.hip", "CK_ROWS")
CHUNK = NT * LANE_ROWS
WAVE = 64 * LANE_ROWS
SEG_CAP = _define("bg_internal.h", "BG_SEG_CAP")


@pytest.fixture(scope="module")
def eng():
    from bedops_amd import Engine
    try:
        torch.cuda.init()
        torch.zeros(1, device="cuda:0")
    except RuntimeError as err:
        pytest.fail("torch cannot reach the GPU (its HIP runtime must start before libbedgpu opens "
                    f"the device, INTEGRATION.md §4.1): {err}")
    e = Engine(0)
    yield e
    e.close()


def parse(text, score=False):
    """BED text -> (names, chrom, start, end[, score]); names in an order that is not strcmp's"""
    rows = [ln.split("\t") for ln in text.decode().splitlines()]
    names = sorted({r[0] for r in rows}, key=lambda s: s.encode())
    names = names[::-1][1:] + names[::-1][:1] if len(names) > 1 else names
    idx = {nm: k for k, nm in enumerate(names)}
    out = [names, np.array([idx[r[0]] for r in rows], dtype=np.int32),
           np.array([int(r[1]) for r in rows], dtype=np.int64),
           np.array([int(r[2]) for r in rows], dtype=np.int64)]
    if score:
        out.append(np.array([float(r[4]) for r in rows], dtype=np.float64))
    return tuple(out)


def col_input(text, kind, device=True):
    p = parse(text, score=kind == BED5)
    cols = [torch.as_tensor(c) for c in p[1:]]
    if device:
        cols = [c.to("cuda:0") for c in cols]
    return (p[0], *cols, kind)


def ivl_text(names, cols):
    c, s, e = (cols[k].cpu().numpy() for k in ("chrom", "start", "end"))
    return "".join(f"{names[c[i]]}\t{s[i]}\t{e[i]}\n" for i in range(len(c))).encode()


def _texts():
    rng = random.Random(20261021)
    mk = lambda n, **kw: randbed.rows(rng, n, span=60000, maxlen=200, **kw)
    a, b, c, r = mk(1500), mk(1500), mk(1200, zero_frac=0.05), mk(300)
    t = {"a": randbed.text(a).encode(), "b": randbed.text(b).encode(), "c": randbed.text(c).encode(),
         "r": randbed.text(r).encode(), "b5": randbed.text(b, rest="bed5", rng=rng).encode()}
    # one-decimal scores; no two map rows equal in (start, end): such rows are summed in the
    # reference's heap-address order, which a table without text cannot give (refused, below)
    seen, u = set(), []
    for row in b:
        if row not in seen:
            seen.add(row)
            u.append(row)
    t["d5"] = "".join(f"{ch}\t{s}\t{e}\tid{i}\t{rng.randint(0, 9999) / 10:.1f}\n"
                      for i, (ch, s, e) in enumerate(u)).encode()
    t["d5_ties"] = "".join(f"{ch}\t{s}\t{e}\tid{i}\t{rng.randint(0, 9999) / 10:.1f}\n"
                           for i, (ch, s, e) in enumerate(b + [b[-1]])).encode()
    return t


T = _texts()


# ------------------------------------------------------------------ 1. same answer both ways
MODES = [("-m", {}), ("-i", {}), ("-d", {}), ("-c", {"full_left": True}), ("-s", {}), ("-p", {}),
         ("-w", {"chop": (100, 30, True)}), ("-m", {"pad": (-20, 35)}), ("-i", {"chrom": "chr10"}),
         ("-d", {"pad": (10, 10), "chrom": "chr2"})]


@pytest.mark.parametrize("kind", [BED3, BED3_SET])
@pytest.mark.parametrize("mode,kw", MODES, ids=[m + "".join("," + k for k in kw) for m, kw in MODES])
def test_same_answer_as_text(eng, mode, kw, kind):
    from bedops_amd.engine import RESKIND_INTERVALS
    rows_needed = mode == "-p" or "pad" in kw or "chrom" in kw
    if kind == BED3_SET and rows_needed:
        kind = BED3  # (operations on rows: as Engine.bedops loads them)
    texts = [T["a"], T["b"], T["c"]] if mode in ("-m", "-s", "-p") else [T["a"], T["c"]]
    want = eng.bedops(mode, texts, **kw)
    assert len(want) > 0
    base = eng.live()
    s = eng.load_columns([col_input(t, kind, device=(i != 1)) for i, t in enumerate(texts)])
    try:
        if "chrom" in kw:
            s.restrict_chrom(kw["chrom"])
        if "pad" in kw:
            for i in range(len(texts)):
                s.pad(i, *kw["pad"])
        r = eng.op(mode, s, list(range(len(texts))), None, kw.get("full_left", False), kw.get("chop", (1, 0, False)))
        try:
            assert r.kind() == (RESKIND_INTERVALS, -1)
            cols = r.columns()
            assert r.text() == want
            assert ivl_text(s.chroms(), cols) == want
        finally:
            r.free()
    finally:
        s.free()
    assert eng.live() == base


# ------------------------------------------------------------------ 2. the ingest kernel's boundaries
def boundary_rows(n):
    """n sorted rows: chromosome changes at a wave boundary, a round boundary, the last row and
    every n // 72 rows besides; starts above 2^32 in every third chromosome; the key limit"""
    cuts = sorted({p for p in [WAVE, CHUNK, n - 1] + list(range(7, n, max(1, n // 72))) if 0 < p < n})
    chrom = np.searchsorted(np.array(cuts, dtype=np.int64), np.arange(n), side="right").astype(np.int64)
    first = np.array([0] + cuts, dtype=np.int64)[chrom] if n else np.zeros(0, dtype=np.int64)
    j = np.arange(n, dtype=np.int64) - first
    start = 10 * j + np.where(chrom % 3 == 1, (1 << 32) + 5, 0)
    end = start + np.where(j % 2 == 0, 15, 5)
    if n:
        start[-1], end[-1] = COORD_MAX - 3, COORD_MAX
    names = [f"c{k:03d}" for k in range(int(chrom.max()) + 1 if n else 0)]
    return names, chrom, start, end


def boundary_input(n, kind, device=True):
    names, chrom, start, end = boundary_rows(n)
    perm = list(range(len(names)))
    random.Random(n).shuffle(perm)  # names[perm[k]] is local name k
    inv = np.zeros(max(len(names), 1), dtype=np.int32)
    inv[perm] = np.arange(len(perm), dtype=np.int32)
    local = [names[p] for p in perm]
    cols = [torch.as_tensor(inv[chrom].astype(np.int32) if n else np.zeros(0, dtype=np.int32)),
            torch.as_tensor(start), torch.as_tensor(end)]
    if device:
        cols = [c.to("cuda:0") for c in cols]
    text = "".join(f"{names[chrom[i]]}\t{start[i]}\t{end[i]}\n" for i in range(n)).encode()
    return (local, *cols, kind), text, names


COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1]


# (a smaller grid only matters past one round)
GRIDS = [(n, None) for n in COUNTS] + [(n, b) for n in COUNTS if n > CHUNK for b in (1, 2)]


@pytest.mark.parametrize("n,blocks", GRIDS)
def test_row_counts_around_every_boundary(eng, monkeypatch, n, blocks):
    if blocks is not None:
        monkeypatch.setenv("BEDGPU_COLS_BLOCKS", str(blocks))  # several rounds per workgroup
    other = T["a"]
    for kind in (BED3, BED3_SET):
        inp, text, names = boundary_input(n, kind, device=(n % 2 == 0))
        if n >= CHUNK - 1:
            assert len(names) >= 70
        want = eng.bedops("-m", [text, other])
        s = eng.load_columns([inp, col_input(other, kind)])
        try:
            assert s.rows(0) == n
            r = eng.op("-m", s, [0, 1])
            try:
                assert r.text() == want
                assert ivl_text(s.chroms(), r.columns()) == want
            finally:
                r.free()
            if kind == BED3:  # the keyed rows themselves
                got = s.columns(0)
                assert ivl_text(got["names"], got) == text
        finally:
            s.free()


def test_more_names_than_the_lds_remap_holds(eng):
    """past CK_LDS_NAMES names the kernel reads the remap from global memory"""
    nn = _define("bg_columns.hip", "CK_LDS_NAMES") + 37
    names = [f"k{k:05d}" for k in range(nn)]
    used = list(range(0, nn, 3))  # one or two rows in every third name
    chrom = np.repeat(used, 2)[:-1]
    start = np.arange(len(chrom), dtype=np.int64) * 7
    text = "".join(f"{names[chrom[i]]}\t{start[i]}\t{start[i] + 9}\n" for i in range(len(chrom))).encode()
    local = names[::-1]
    inp = (local, torch.as_tensor((nn - 1 - chrom).astype(np.int32)).to("cuda:0"), torch.as_tensor(start),
           torch.as_tensor(start + 9), BED3)
    s = eng.load_columns([inp])
    try:
        assert s.chroms() == names
        got = s.columns(0)
        assert ivl_text(got["names"], got) == text
        r = eng.op("-m", s, [0])
        assert r.text() == eng.bedops("-m", [text])
        r.free()
    finally:
        s.free()


# ------------------------------------------------------------------ 3. segmented results
def test_segmented_result_exports_and_formats_in_either_order(eng):
    n = 3 * SEG_CAP + 1 + 200
    a = "".join(f"chr{1 + (i >= n // 2)}\t{10 * i}\t{10 * i + 6}\n" for i in range(n)).encode()
    b = "".join(f"chr{1 + (i >= n // 2)}\t{10 * i + 3}\t{10 * i + 9}\n" for i in range(n)).encode()
    want = eng.bedops("-i", [a, b])
    assert want.count(b"\n") >= 3 * SEG_CAP + 1
    for order in ("export-format", "format-export"):
        s = eng.load_columns([col_input(a, BED3_SET), col_input(b, BED3_SET)])
        try:
            r = eng.op("-i", s, [0, 1])
            try:
                if order == "export-format":
                    cols = r.columns()
                    text = r.text()
                else:
                    text = r.text()
                    cols = r.columns()
                assert text == want, order
                assert ivl_text(s.chroms(), cols) == want, order
                assert r.text() == want
            finally:
                r.free()
        finally:
            s.free()


# ------------------------------------------------------------------ 4. errors
def error_rows():
    n = 3 * CHUNK
    chrom = (np.arange(n) >= 2 * CHUNK + 100).astype(np.int32)
    start = 10 * np.arange(n, dtype=np.int64)
    return ["chrA", "chrB"], chrom, start, start + 4


def _unsorted_at(r):
    def f(c, s, e):
        s[r] = s[r - 1] - 5
    return f, r


def _second_run(c, s, e):
    c[-1] = 0


def _start_gt_end(c, s, e):
    e[500] = s[500] - 1


def _end_past(c, s, e):
    e[500] = 1 << 40


def _neg_start(c, s, e):
    s[0] = -1


def _two(c, s, e):
    e[2000] = 1 << 40
    s[700] = s[699] - 5


BAD = {"inside-a-wave": (*_unsorted_at(10), UNSORTED), "across-lanes": (*_unsorted_at(8), UNSORTED),
       "across-waves": (*_unsorted_at(WAVE), UNSORTED), "across-rounds": (*_unsorted_at(CHUNK), UNSORTED),
       "second-run": (_second_run, 3 * CHUNK - 1, UNSORTED), "start>end": (_start_gt_end, 500, RANGE),
       "end-past-keys": (_end_past, 500, RANGE), "negative-start": (_neg_start, 0, RANGE),
       "first-of-two": (_two, 700, UNSORTED)}


@pytest.mark.parametrize("blocks", [None, 1])
@pytest.mark.parametrize("case", list(BAD))
def test_bad_rows_fail_like_the_text_loader(eng, monkeypatch, case, blocks):
    from bedops_amd import BedgpuError
    if blocks is not None:
        monkeypatch.setenv("BEDGPU_COLS_BLOCKS", str(blocks))
    edit, row, code = BAD[case]
    names, c, s, e = error_rows()
    edit(c, s, e)
    if case != "negative-start":  # (BED text cannot say it)
        text = "".join(f"{names[c[i]]}\t{s[i]}\t{e[i]}\n" for i in range(len(c))).encode()
        with pytest.raises(BedgpuError) as et:
            eng.load([(text, BED3)]).free()
        assert et.value.code == code
        if case != "second-run":  # (the text loader names the chromosome there, not the line)
            assert f"data line {row + 1}:" in str(et.value)
    base = eng.live()
    for kind in (BED3, BED3_SET):
        for dev in ("cuda:0", "cpu"):
            with pytest.raises(BedgpuError) as ec:
                eng.load_columns([(["chrA"], *[torch.zeros(3, dtype=torch.int64)] * 3, BED3),
                                  (names, *[torch.as_tensor(x).to(dev) for x in (c, s, e)], kind)]).free()
            assert ec.value.code == code, str(ec.value)
            assert f"input 2, row {row}:" in str(ec.value)
            assert eng.live() == base


def test_host_side_argument_errors_leave_nothing_behind(eng):
    from bedops_amd import BedgpuError
    z = lambda n=4, dt=torch.int64: torch.zeros(n, dtype=dt)
    sc = torch.ones(4, dtype=torch.float64)
    nan = sc.clone()
    nan[2] = float("inf")
    cases = [((["chr1"], torch.tensor([0, 0, 1, 0]), z(), z(), BED3), ARG),
             ((["chr1"], torch.tensor([0, -1, 0, 0]), z(), z(), BED3), ARG),
             ((["chr1", ""], z(), z(), z(), BED3), ARG),
             ((["chr1", "chr2", "chr1"], z(), z(), z(), BED3), ARG),
             ((["chr 1"], z(), z(), z(), BED3), ARG),
             ((["chr\t1"], z(), z(), z(), BED3_SET), ARG),
             ((["c" * 128], z(), z(), z(), BED3), CHROM),
             ((["chr1"], z(), z(), z(), 1), ARG),
             ((["chr1"], z(), z(), z(), sc, 4), ARG),
             ((["chr1"], z(), z(), z(), sc, BED3), ARG),
             ((["chr1"], z(), z(), z(), BED5), ARG),
             ((["chr1"], z(), z(), z(), nan, BED5), UNSUPPORTED)]
    for inp, code in cases:
        base = eng.live()
        with pytest.raises(BedgpuError) as ei:
            eng.load_columns([inp])
        assert ei.value.code == code, (inp, str(ei.value))
        assert eng.live() == base
    # what the host cannot see in device arrays is found by the kernel
    base = eng.live()
    # (a bad chrom index after a row of a higher rank is still that, not "unsorted")
    after = (["chr1", "chr2"], torch.tensor([1, 1, 5, 1]), torch.tensor([5, 6, 0, 8]), torch.tensor([9, 9, 9, 9]), BED3)
    for inp, code in ((cases[0][0], ARG), (cases[-1][0], UNSUPPORTED), (after, ARG)):
        dev = tuple(x.to("cuda:0") if isinstance(x, torch.Tensor) else x for x in inp)
        with pytest.raises(BedgpuError) as ei:
            eng.load_columns([dev])
        assert ei.value.code == code, str(ei.value)
        assert "row 2" in str(ei.value)
        assert eng.live() == base
    s = eng.load_columns([(["c" * 127], z(), z(), z() + 1, sc, BED5)])  # (what is allowed)
    assert s.rows(0) == 4 and s.chroms() == ["c" * 127]
    s.free()


# ------------------------------------------------------------------ 5. element-of
@pytest.mark.parametrize("mode,spec", [("-e", "1"), ("-n", "50%"), ("-e", "100%")])
def test_element_of_rows_select_the_printed_lines(eng, mode, spec):
    from bedops_amd import BedgpuError
    from bedops_amd.engine import RESKIND_ROWS
    want = eng.bedops(mode, [T["a"], T["b"], T["c"]], spec=spec)
    assert 0 < want.count(b"\n") < T["a"].count(b"\n")
    base = eng.live()
    s = eng.load_columns([col_input(T["a"], BED3), col_input(T["b"], BED3_SET), col_input(T["c"], BED3)])
    try:
        r = eng.op(mode, s, [0, 1, 2], spec)
        try:
            assert r.kind() == (RESKIND_ROWS, 0)
            rows = r.columns()["rows"].cpu().numpy()
            lines = T["a"].splitlines(keepends=True)
            assert b"".join(lines[i] for i in rows) == want
            with pytest.raises(BedgpuError) as ei:
                r.text()
            assert ei.value.code == ARG
        finally:
            r.free()
    finally:
        s.free()
    assert eng.live() == base


# ------------------------------------------------------------------ 6. bedmap
OPS6 = ["count", "indicator", "sum", "mean", "min", "max"]


@pytest.mark.parametrize("crit,value", [("bp-ovr", 5), ("range", 150), ("fraction-both", 0.3)])
@pytest.mark.parametrize("scores", ["b5", "d5"])
def test_bedmap_text_and_values(eng, scores, crit, value):
    from bedops_amd.engine import RESKIND_MAP
    base = eng.live()
    for single in (False, True):
        texts = [T[scores]] if single else [T["r"], T[scores]]
        kinds = [BED5] if single else [BED3, BED5]
        s = eng.load_columns([col_input(t, k) for t, k in zip(texts, kinds)])
        try:
            for prec in (6, 15):
                kw = dict(precision=prec, criterion=crit, value=value, overlap_bp=value if crit == "bp-ovr" else 1)
                want = eng.bedmap(OPS6, texts[0], None if single else texts[1], **kw)
                r = eng.map_op(s, OPS6, 0, 0 if single else 1, **kw)
                try:
                    assert r.kind() == (RESKIND_MAP, 0)
                    assert r.text() == want
                    vals = [v.cpu().numpy() for v in r.columns()["values"]]
                    one = r.columns(op_index=3)["values"].cpu().numpy()
                    assert np.array_equal(one, vals[3], equal_nan=True)
                finally:
                    r.free()
                toks = [ln.split("|") for ln in want.decode().splitlines()]
                assert len(toks) == len(vals[0]) > 0
                for q, op in enumerate(OPS6):
                    fmt = "%d" if op in ("count", "indicator") else "%%.%df" % prec
                    got = ["NAN" if np.isnan(v) else fmt % v for v in vals[q]]
                    assert got == [t[q] for t in toks], (op, prec, single)
                assert any(t[2] == "NAN" for t in toks) or single
        finally:
            s.free()
    assert eng.live() == base


def test_bedmap_export_refusals(eng):
    from bedops_amd import BedgpuError
    s = eng.load_columns([col_input(T["r"], BED3), col_input(T["b5"], BED5)])
    try:
        r = eng.map_op(s, ["count", "stdev"], skip_unmapped=False)
        with pytest.raises(BedgpuError) as ei:
            r.columns(op_index=1)
        assert ei.value.code == UNSUPPORTED
        assert r.columns()["values"][1] is None
        with pytest.raises(BedgpuError) as ei:
            r.columns(op_index=2)
        assert ei.value.code == ARG
        r.free()
        r = eng.map_op(s, ["count"], skip_unmapped=True)
        with pytest.raises(BedgpuError) as ei:
            r.columns(op_index=0)
        assert ei.value.code == ARG
        r.free()
        m = eng.op("-m", s, [0, 1])
        for fn in (eng.L.bg_result_export_rows, ):
            assert fn(eng.ctx, m.h, None) == ARG
        assert eng.L.bg_result_export_map(eng.ctx, m.h, 0, None) == ARG
        m.free()
    finally:
        s.free()


# ------------------------------------------------------------------ 7. InputSet.columns round trip
def test_text_to_columns_and_back(eng):
    from bedops_amd import BedgpuError
    s = eng.load([(T["a"], BED3), (T["b5"], BED5), (T["c"], BED3_SET)])
    try:
        c0, c1 = s.columns(0), s.columns(1)
        assert "score" not in c0 and c1["score"].dtype == torch.float64
        assert ivl_text(c0["names"], c0) == T["a"]
        assert c1["score"].cpu().tolist() == [float(ln.split(b"\t")[4]) for ln in T["b5"].splitlines()]
        with pytest.raises(BedgpuError) as ei:
            s.columns(2)
        assert ei.value.code == ARG
    finally:
        s.free()
    s2 = eng.load_columns([(c0["names"], c0["chrom"], c0["start"], c0["end"], BED3),
                           (c1["names"], c1["chrom"], c1["start"], c1["end"], c1["score"], BED5)])
    try:
        for want, got in ((c0, s2.columns(0)), (c1, s2.columns(1))):
            assert got["names"] == want["names"]
            for k in want:
                if k != "names":
                    assert torch.equal(got[k], want[k]), k
    finally:
        s2.free()


# ------------------------------------------------------------------ 8. refusals
def test_consumers_of_row_text_refuse_column_tables(eng):
    from bedops_amd import BedgpuError
    base = eng.live()
    s = eng.load_columns([col_input(T["r"], BED3), col_input(T["b5"], BED5), col_input(T["d5_ties"], BED5)])
    try:
        calls = {"everything": lambda: eng.op("-u", s, [0, 1]),
                 "closest": lambda: eng.closest_op(s, 0, 1),
                 "echo": lambda: eng.map_op(s, ["echo", "count"]),
                 "echo-map-id": lambda: eng.map_op(s, ["echo-map-id"]),
                 "echo-map-score": lambda: eng.map_op(s, ["echo-map-score"]),
                 "max-element": lambda: eng.map_op(s, ["max-element"]),
                 "wmean": lambda: eng.map_op(s, ["wmean"]),
                 "tmean": lambda: eng.map_op(s, [("tmean", 0.1, 0.2)]),
                 "faster": lambda: eng.map_op(s, ["count"], faster=True),
                 "decimal-ties": lambda: eng.map_op(s, ["sum"], 0, 2)}
        for name, fn in calls.items():
            live = eng.live()
            with pytest.raises(BedgpuError) as ei:
                fn()
            assert ei.value.code == ARG, (name, str(ei.value))
            assert "has no text" in str(ei.value), name
            assert eng.live() == live, name
        # (integer sums do not depend on the order of equal rows)
        r = eng.map_op(s, ["count", "min"], 0, 2)
        assert r.rows() == s.rows(0)
        r.free()
    finally:
        s.free()
    assert eng.live() == base


def test_decimal_sums_need_rows_of_one_start_in_end_order(eng):
    """the loader orders rows by start only, so equal (start, end) rows need not be neighbours:
    (10,20) (10,30) (10,20) is refused like an adjacent tie; strictly increasing ends pass"""
    from bedops_amd import BedgpuError
    ref = (["chr1"], torch.tensor([0]), torch.tensor([0]), torch.tensor([100]), BED3)
    sc = torch.tensor([0.5, 1.25, 2.5])

    def run(ends):
        s = eng.load_columns([ref, (["chr1"], torch.zeros(3, dtype=torch.int32), torch.tensor([10, 10, 10]),
                                    torch.tensor(ends), sc, BED5)])
        try:
            r = eng.map_op(s, ["sum"])
            try:
                return r.text()
            finally:
                r.free()
        finally:
            s.free()

    base = eng.live()
    assert run([20, 30, 40]) == b"4.250000\n"
    for ends in ([20, 30, 20], [20, 20, 30], [30, 20, 40]):
        with pytest.raises(BedgpuError) as ei:
            run(ends)
        assert ei.value.code == ARG and "has no text" in str(ei.value)
    assert eng.live() == base


# ------------------------------------------------------------------ 9. allocation failures
@pytest.mark.parametrize("kinds", [(BED3, BED5), (BED3_SET, BED3_SET)])
def test_injected_allocation_failures(eng, kinds):
    from bedops_amd import BedgpuError
    texts = [T["a"], T["b5"]]

    def cycle():
        s = eng.load_columns([col_input(t, k, device=(i == 0)) for i, (t, k) in enumerate(zip(texts, kinds))])
        try:
            r = eng.op("-m", s, [0, 1])
            try:
                return r.text()
            finally:
                r.free()
        finally:
            s.free()

    want = eng.bedops("-m", texts)
    assert cycle() == want
    base = eng.live()
    failed = 0
    for n in range(1, 200):
        eng.fail_alloc_after(n)
        try:
            got = cycle()
        except BedgpuError as e:
            assert e.code == NOMEM, (n, str(e))
            assert "injected" in str(e), (n, str(e))
            assert eng.live() == base, n
            failed += 1
            continue
        finally:
            eng.fail_alloc_after(0)
        assert got == want and eng.live() == base
        break
    else:
        pytest.fail("no success within 200 allocations")
    assert failed >= 8  # (load_columns alone allocates more than that)
