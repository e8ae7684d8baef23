"""closest-features for column callers: bg_closest_rows (the scan of bg_closest on tables that
need no text) and bg_result_export_closest / Result.closest (the chosen rows and the distances
--dist prints, as int64 device columns; and the one element --shortest --dist prints).

Oracles, never the code under test:
  the text route   the same rows as BG_BED3_REST text whose remainder is the row's index, through
                   closest_op(dist=True) and the formatter (what the reference fixtures pin),
                   each `ref|left|dL|right|dR` line parsed back into indices and distances;
  a brute force    for pairwise disjoint query rows under pairwise disjoint reference rows, where
                   the reference's reader cache cannot matter: the last row ending at or before
                   the reference row, the first starting at or after its end, and the overlap
                   rules of ClosestFeature.cpp:332-388, checked once against the CPU oracle's text
                   before it is trusted.

Shapes: the designs of test_closest_paths_model (deep caches, clamped look-backs, every rung of
the recovery ladder); random rows over four chromosomes with zero-length and adjacent rows and
chromosomes that only one table has; reference row counts around the kernel's 4 rows per lane
and 1,024 rows per workgroup round (0, 1, 3, 4, 5, 1,023, 1,024, 1,025, 4,097), with the grid
capped at 1 and 2 workgroups so that a workgroup runs several rounds."""
import bisect
import ctypes
import random
import subprocess

import numpy as np
import pytest
import torch

import kernel_paths
import randbed
import test_closest_paths_model as D

pytestmark = pytest.mark.gpu

# (torch's HIP runtime starts before libbedgpu opens the device: INTEGRATION.md §4.1, and
# tests/test_gpu_map_pairs.py for why this happens at collection)
if torch.cuda.is_available():
    torch.cuda.init()

BED3, BED3_REST, BED5, BED3_SET = 0, 1, 2, 3
ARG, NOMEM = -6, -7
NA = -(1 << 63)
COLS4 = ("left", "right", "left_dist", "right_dist")


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


# ------------------------------------------------------------------ inputs
def id_text(rows):
    """BED3 + one more column: the row's index"""
    return "".join(f"{c}\t{s}\t{e}\ti{i}\n" for i, (c, s, e) in enumerate(rows)).encode()


def srt(rows):
    return sorted(rows, key=lambda r: (r[0].encode(), r[1], r[2]))


def col_input(rows, score=False):
    names = sorted({r[0] for r in rows}, key=lambda s: s.encode())[::-1]  # not strcmp order
    idx = {nm: k for k, nm in enumerate(names)}
    cols = [torch.tensor([idx[r[0]] for r in rows], dtype=torch.int32),
            torch.tensor([r[1] for r in rows], dtype=torch.int64),
            torch.tensor([r[2] for r in rows], dtype=torch.int64)]
    if score:
        cols.append(torch.tensor([float(i % 7) + 0.5 for i in range(len(rows))], dtype=torch.float64))
    return (names, *[c.to("cuda:0") for c in cols], BED5 if score else BED3)


def design_rows(name):
    """a design of test_closest_paths_model as (chromosome name, start, end) rows"""
    d = D.design(name)
    names = sorted(randbed.CHROMS, key=lambda s: s.encode()) if name in ("nested", "sparse") else D.NAMES
    conv = lambda rs: [(names[g], s, e) for g, s, e in rs]
    return conv(d.Q), conv(d.C)


def _random_inputs():
    out = {}
    rng = random.Random(20261021)
    # zero-length rows in both tables
    out["zero"] = (randbed.rows(rng, 1500, span=8000, maxlen=80, zero_frac=0.1),
                   randbed.rows(rng, 1500, span=8000, maxlen=80, zero_frac=0.1))
    # reference rows that start where a query row ends and end where one starts (end == start)
    c = randbed.rows(rng, 1200, span=30000, maxlen=40)
    q = randbed.rows(rng, 600, span=30000, maxlen=40)
    q += [(ch, e, e + 7) for ch, s, e in c[::5]] + [(ch, s - 3, s) for ch, s, e in c[2::5] if s >= 3]
    out["adjacent"] = (srt(q), c)
    # a reference chromosome the query file lacks, and the reverse
    out["chroms"] = (randbed.rows(rng, 1000, chroms=["chr1", "chr10", "chr2"], span=5000),
                     randbed.rows(rng, 1000, chroms=["chr10", "chr2", "chrX"], span=5000))
    # nested rows (the reader cache's history decides)
    out["nested"] = (randbed.rows(rng, 1200, span=20000, maxlen=1500),
                     randbed.rows(rng, 1200, span=20000, maxlen=1500))
    return out


RANDOM = _random_inputs()
INPUTS = [*D._BUILDERS, *("rand-" + k for k in RANDOM)]


def inputs(key):
    return RANDOM[key[5:]] if key.startswith("rand-") else design_rows(key)


# ------------------------------------------------------------------ the text route
def _idx(row_text):
    return int(row_text.rsplit("\t", 1)[1][1:])


def parse_all(text, n):
    """`ref|left|dL|right|dR` lines -> left, right, left_dist, right_dist"""
    lines = text.decode().split("\n")[:-1]
    assert len(lines) == n
    out = {k: np.empty(n, dtype=np.int64) for k in COLS4}
    for i, ln in enumerate(lines):
        ref, l, dl, r, dr = ln.split("|")
        assert _idx(ref) == i
        out["left"][i], out["left_dist"][i] = (-1, NA) if l == "NA" else (_idx(l), int(dl))
        out["right"][i], out["right_dist"][i] = (-1, NA) if r == "NA" else (_idx(r), int(dr))
        assert (l == "NA") == (dl == "NA") and (r == "NA") == (dr == "NA")
    return out


def parse_shortest(text, n):
    """`ref|element|d` lines -> rows, dist"""
    lines = text.decode().split("\n")[:-1]
    assert len(lines) == n
    out = {k: np.empty(n, dtype=np.int64) for k in ("rows", "dist")}
    for i, ln in enumerate(lines):
        ref, x, d = ln.split("|")
        assert _idx(ref) == i
        out["rows"][i], out["dist"][i] = (-1, NA) if x == "NA" else (_idx(x), int(d))
    return out


def host(cols):
    return {k: v.cpu().numpy() for k, v in cols.items()}


def same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == np.int64
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


_TEXT = {}


def text_route(eng, key, no_overlaps):
    """the parsed text of closest_op(dist=True) and of closest_op(shortest=True, dist=True) on the
    input's id texts, computed once and shared; the exports of those very result objects are
    compared with it on the way"""
    if (key, no_overlaps) in _TEXT:
        return _TEXT[key, no_overlaps]
    from bedops_amd import RESKIND_OTHER
    Q, C = inputs(key)
    s = eng.load([(id_text(Q), BED3_REST), (id_text(C), BED3_REST)])
    try:
        r = eng.closest_op(s, 0, 1, dist=True, no_overlaps=no_overlaps)
        want = parse_all(r.text(), len(Q))
        assert r.kind() == (RESKIND_OTHER, -1)  # as before bg_closest_rows
        same(host(r.closest()), want)
        r2 = eng.closest_op(s, 0, 1, shortest=True, dist=True, no_overlaps=no_overlaps)
        wants = parse_shortest(r2.text(), len(Q))
        same(host(r2.closest(shortest=True)), wants)
        # the flags the result was built with play no part in either export
        same(host(r.closest(shortest=True)), wants)
        same(host(r2.closest()), want)
        r.free()
        r2.free()
    finally:
        s.free()
    _TEXT[key, no_overlaps] = dict(want, **wants)
    return _TEXT[key, no_overlaps]


def rows_export(eng, Q, C, no_overlaps, cols=None):
    """closest_rows + both forms of Result.closest(); cols: None = id texts, else the kind the
    column tables are loaded as"""
    from bedops_amd import RESKIND_CLOSEST
    if cols is None:
        s = eng.load([(id_text(Q), BED3_REST), (id_text(C), BED3_REST)])
    else:
        s = eng.load_columns([col_input(Q, cols == BED5), col_input(C, cols == BED5)])
    try:
        r = eng.closest_rows(s, 0, 1, no_overlaps=no_overlaps)
        assert r.kind() == (RESKIND_CLOSEST, 0) and r.rows() == len(Q)
        got = dict(host(r.closest()), **host(r.closest(shortest=True)))
        assert sorted(r.columns()) == sorted(COLS4)
        r.free()
        return got
    finally:
        s.free()


# ------------------------------------------------------------------ 1. text-route parity
@pytest.mark.parametrize("no_overlaps", [False, True], ids=["overlaps", "no-overlaps"])
@pytest.mark.parametrize("key", INPUTS)
def test_export_matches_the_text_route(eng, key, no_overlaps):
    want = text_route(eng, key, no_overlaps)  # (asserts the exports of the text results inside)
    # what the columns promise whatever the input
    assert len(want["left"]) == len(inputs(key)[0])
    assert (want["left_dist"][want["left"] >= 0] <= 0).all() and (want["right_dist"][want["right"] >= 0] >= 0).all()


# ------------------------------------------------------------------ 2. column tables
@pytest.mark.parametrize("no_overlaps", [False, True], ids=["overlaps", "no-overlaps"])
@pytest.mark.parametrize("key", INPUTS)
def test_column_tables_give_the_text_routes_arrays(eng, key, no_overlaps):
    Q, C = inputs(key)
    want = text_route(eng, key, no_overlaps)
    same(rows_export(eng, Q, C, no_overlaps, cols=BED3), want)
    if key in ("stair300", "rand-zero", "rand-nested"):
        same(rows_export(eng, Q, C, no_overlaps, cols=BED5), want)
        same(rows_export(eng, Q, C, no_overlaps), want)  # closest_rows on the text tables


def test_a_column_result_has_no_text_and_a_text_one_prints_the_default(eng):
    from bedops_amd.engine import BedgpuError
    Q, C = inputs("rand-adjacent")
    s = eng.load_columns([col_input(Q), col_input(C)])
    try:
        r = eng.closest_rows(s)
        base = eng.live()
        _, ran = kernel_paths.launches(eng, lambda: pytest.raises(BedgpuError, r.format))
        with pytest.raises(BedgpuError) as ei:
            r.format()
        assert ei.value.code == ARG and "has no text" in ei.value.msg
        assert ran == {} and eng.live() == base  # refused before any launch
        assert eng.L.bg_result_write(eng.ctx, r.h, 1) == ARG
        r.free()
    finally:
        s.free()
    # text tables, one of them without its remainder: the same refusal
    s = eng.load([(id_text(Q), BED3_REST), (id_text(C), BED3)])
    try:
        r = eng.closest_rows(s)
        with pytest.raises(BedgpuError) as ei:
            r.format()
        assert ei.value.code == ARG and "input 2 has no text" in ei.value.msg
        same(host(r.closest()), {k: text_route(eng, "rand-adjacent", False)[k] for k in COLS4})
        r.free()
    finally:
        s.free()
    for no in (False, True):
        s = eng.load([(id_text(Q), BED3_REST), (id_text(C), BED3_REST)])
        try:
            r, r0 = eng.closest_rows(s, no_overlaps=no), eng.closest_op(s, no_overlaps=no)
            t = r.text()
            assert t == r0.text() and t.count(b"\n") == len(Q)
            # exporting and formatting do not disturb each other, in either order
            a = host(r.closest())
            assert r.text() == t
            same(host(r.closest()), a)
            r.free()
            r = eng.closest_rows(s, no_overlaps=no)
            same(host(r.closest()), a)
            assert r.text() == t
            same(host(r.closest(shortest=True)), {k: text_route(eng, "rand-adjacent", no)[k] for k in ("rows", "dist")})
            r.free()
            r0.free()
        finally:
            s.free()


# ------------------------------------------------------------------ 3. an independent brute force
def disjoint_tables():
    """query rows pairwise disjoint (some touching) and reference rows pairwise disjoint too, of
    every relation to the query rows: in gaps, touching, hanging over either end, inside one,
    over several. (Disjoint query rows alone do not take the history out: a long reference row
    that makes a row inside it its left empties the cache, and a short reference row nested in
    the long one then prints NA for the left it would have had. Found on the CPU, against the
    oracle.)"""
    rng = random.Random(5)
    C, Q = [], []
    for ch in ("chr1", "chr10", "chrX"):
        pos = rng.randint(0, 50)
        for _ in range(400):
            ln = rng.randint(1, 60)
            C.append((ch, pos, pos + ln))
            pos += ln + rng.choice([0, 0, 1, 5, 40, 200])
        end, pos = pos + 300, rng.randint(0, 30)
        while pos < end:
            ln = rng.choice([1, 2, 10, 30, 100, 400])
            Q.append((ch, pos, pos + ln))
            pos += ln + rng.choice([0, 0, 1, 3, 20, 90])
    Q += [("chr2", 5, 9), ("chr0", 1, 2)]  # chromosomes without query rows, after and before
    return srt(Q), srt(C)


def cf_dist(xs, xe, bs, be):
    """getDistance(x, ref), ClosestFeature.cpp:244-255"""
    if xe <= bs:
        return -((bs - xe) + 1)
    if be <= xs:
        return (xs - be) + 1
    return 0


def brute(Q, C, no_overlaps):
    """closest-features on disjoint query rows, from the reference's rules alone: without
    overlaps the last row that ends at or before the reference row's start and the first that
    starts at or after its end. With overlaps, of the rows that overlap it: one that starts at or
    before it is the left; one that reaches its end or beyond is the right; one strictly inside is
    the right when the reference row's centre lies in its first half (the last such row stays),
    else the left unless an overlapping left is there already (ClosestFeature.cpp:332-388)."""
    by = {}
    for i, (ch, s, e) in enumerate(C):
        by.setdefault(ch, []).append((s, e, i))
    n = len(Q)
    out = {k: np.full(n, -1 if "dist" not in k else NA, dtype=np.int64) for k in COLS4}
    out.update(rows=np.full(n, -1, dtype=np.int64), dist=np.full(n, NA, dtype=np.int64))
    for k, (ch, bs, be) in enumerate(Q):
        cs = by.get(ch, [])
        ends = [e for _, e, _ in cs]      # ascending too: the rows are disjoint
        starts = [s for s, _, _ in cs]
        p = bisect.bisect_right(ends, bs) - 1   # last with end <= bs
        nx = bisect.bisect_left(starts, be)     # first with start >= be
        left = cs[p] if p >= 0 else None
        right = None
        if not no_overlaps:
            zero_left = False
            for s, e, i in cs[p + 1:nx]:
                if s <= bs:
                    left, zero_left = (s, e, i), True
                elif be <= e:
                    right = (s, e, i)
                else:
                    cen = (be - 1.0 + bs) / 2.0
                    half = cen < s or (cen + 1 - s) / float(e - s) < 0.5
                    if half:
                        right = (s, e, i)
                    elif not zero_left:
                        left, zero_left = (s, e, i), True
        if right is None and nx < len(cs):
            right = cs[nx]
        dl = dr = None
        if left:
            out["left"][k], out["left_dist"][k] = left[2], (dl := cf_dist(left[0], left[1], bs, be))
        if right:
            out["right"][k], out["right_dist"][k] = right[2], (dr := cf_dist(right[0], right[1], bs, be))
        # --shortest: an overlapping left, then an overlapping right, else the nearer, ties left
        if left and (dl == 0 or not right or (dr != 0 and -dl <= dr)):
            out["rows"][k], out["dist"][k] = left[2], dl
        elif right:
            out["rows"][k], out["dist"][k] = right[2], dr
    return out


@pytest.mark.parametrize("no_overlaps", [False, True], ids=["overlaps", "no-overlaps"])
def test_disjoint_query_rows_against_a_brute_force(eng, oracle_bin, tmp_path, no_overlaps):
    Q, C = disjoint_tables()
    for T in (Q, C):
        assert all(a[0] != b[0] or a[2] <= b[1] for a, b in zip(T, T[1:]))
    want = brute(Q, C, no_overlaps)
    # the model against the CPU oracle's text, before it is trusted
    q, c = tmp_path / "q.bed", tmp_path / "c.bed"
    q.write_bytes(id_text(Q))
    c.write_bytes(id_text(C))
    args = ["--no-overlaps"] if no_overlaps else []
    run = lambda *a: subprocess.run([oracle_bin["closest"], "--dist", *a, *args, str(q), str(c)],
                                    stdout=subprocess.PIPE, check=True).stdout
    same(parse_all(run(), len(Q)), {k: want[k] for k in COLS4})
    same(parse_shortest(run("--closest"), len(Q)), {k: want[k] for k in ("rows", "dist")})
    assert (want["left_dist"] == 0).sum() > 50 and (want["right_dist"] == 0).sum() > 50 or no_overlaps
    assert (want["left"] < 0).any() and (want["right"] < 0).any()
    same(rows_export(eng, Q, C, no_overlaps, cols=BED3), want)
    same(rows_export(eng, Q, C, no_overlaps), want)


# ------------------------------------------------------------------ 4. the kernel's boundaries
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4097]
_SIZED = {}


def sized(eng, n):
    """n reference rows over three chromosomes, 1,200 query rows; the text route's arrays"""
    if n not in _SIZED:
        rng = random.Random(n)
        Q = randbed.rows(rng, n, chroms=["chr1", "chr10", "chr2"], span=12000, maxlen=60, zero_frac=0.02)
        C = randbed.rows(rng, 1200, chroms=["chr1", "chr10", "chr2"], span=12000, maxlen=60, zero_frac=0.02)
        key = f"rand-sized{n}"
        RANDOM[key[5:]] = (Q, C)
        _SIZED[n] = (Q, C, text_route(eng, key, False) if n else
                     {k: np.empty(0, dtype=np.int64) for k in (*COLS4, "rows", "dist")})
    return _SIZED[n]


@pytest.mark.parametrize("n", SIZES)
def test_reference_row_counts_around_the_lane_and_the_round(eng, n):
    Q, C, want = sized(eng, n)
    same(rows_export(eng, Q, C, False, cols=BED3), want)
    same(rows_export(eng, Q, C, False), want)


@pytest.mark.parametrize("blocks", ["1", "2"])
@pytest.mark.parametrize("n", [1025, 4097])
def test_a_capped_grid_runs_several_rounds(eng, monkeypatch, n, blocks):
    Q, C, want = sized(eng, n)
    monkeypatch.setenv("BEDGPU_COLS_BLOCKS", blocks)
    same(rows_export(eng, Q, C, False, cols=BED3), want)


def test_an_empty_query_table(eng):
    Q = randbed.rows(random.Random(3), 1030)
    for cols in (None, BED3):
        got = rows_export(eng, Q, [], False, cols=cols)
        for k in ("left", "right", "rows"):
            assert (got[k] == -1).all() and len(got[k]) == len(Q)
        for k in ("left_dist", "right_dist", "dist"):
            assert (got[k] == NA).all() and len(got[k]) == len(Q)


GUARD = 4  # elements on either side (the interior stays 16-byte aligned)


def raw_export(eng, r, n, which):
    """bg_result_export_closest with the columns in `which` (a set of positions 0-5), each in a
    tensor with guard elements around it; {position: interior as numpy}, guards checked"""
    bufs = {p: torch.full((n + 2 * GUARD,), -77, dtype=torch.int64, device="cuda:0") for p in which}
    ptr = [ctypes.c_void_p(bufs[p].data_ptr() + 8 * GUARD) if p in bufs else None for p in range(6)]
    eng.sync_torch()
    eng._check(eng.L.bg_result_export_closest(eng.ctx, r.h, *ptr))
    eng.sync()
    out = {}
    for p, t in bufs.items():
        h = t.cpu().numpy()
        assert (h[:GUARD] == -77).all() and (h[n + GUARD:] == -77).all(), p
        out[p] = h[GUARD:n + GUARD]
    return out


@pytest.mark.parametrize("n", [5, 1025])
def test_each_column_alone_and_the_guards(eng, n):
    Q, C, want = sized(eng, n)
    order = (*COLS4, "rows", "dist")
    s = eng.load_columns([col_input(Q), col_input(C)])
    try:
        r = eng.closest_rows(s)
        full, ran = kernel_paths.launches(eng, lambda: raw_export(eng, r, n, set(range(6))))
        assert ran == {"k_closest_export": 1}
        for p in range(6):
            assert (full[p] == want[order[p]]).all(), order[p]
            one, ran = kernel_paths.launches(eng, lambda: raw_export(eng, r, n, {p}))
            assert ran == {"k_closest_export": 1}
            assert (one[p] == full[p]).all(), order[p]
        _, ran = kernel_paths.launches(eng, lambda: raw_export(eng, r, n, set()))
        assert ran == {}  # every pointer NULL: no launch
        # a column that is not 16-byte aligned is refused
        t = torch.zeros(n + 2, dtype=torch.int64, device="cuda:0")
        assert eng.L.bg_result_export_closest(eng.ctx, r.h, ctypes.c_void_p(t.data_ptr() + 8), None, None, None,
                                              None, None) == ARG
        r.free()
    finally:
        s.free()


# ------------------------------------------------------------------ 5. contract and accounting
def test_refusals_leave_nothing_behind(eng):
    from bedops_amd.engine import BedgpuError
    Q, C = inputs("rand-chroms")
    s = eng.load([(id_text(Q), BED3), (id_text(C), BED3), (id_text(C), BED3_SET)])
    try:
        base = eng.live()
        for mk in (lambda: eng.op("-m", s, [0, 1]), lambda: eng.map_op(s, ["count"], 0, 1)):
            r = mk()
            r.rows()  # (a segmented interval result fetches its count here)
            held = eng.live()
            with pytest.raises(BedgpuError) as ei:
                r.closest()
            assert ei.value.code == ARG and "not a closest-features result" in ei.value.msg
            assert eng.live() == held
            r.free()
            assert eng.live() == base
        for ref, query in ((0, 2), (2, 0), (-1, 1), (0, 3), (3, 0), (0, -1)):
            with pytest.raises(BedgpuError) as ei:
                eng.closest_rows(s, ref, query)
            assert ei.value.code == ARG
            assert eng.live() == base
        with pytest.raises(BedgpuError) as ei:
            eng.closest_rows(s, 0, 2)
        assert "BG_BED3_SET" in ei.value.msg
        r = eng.closest_rows(s, 0, 1)
        assert eng.live()[0] > base[0]
        r.closest()
        r.free()
        assert eng.live() == base
    finally:
        s.free()


def test_injected_allocation_failures_balance(eng):
    from bedops_amd.engine import BedgpuError
    Q, C = inputs("rand-chroms")
    want = text_route(eng, "rand-chroms", False)
    s = eng.load_columns([col_input(Q), col_input(C)])
    try:
        base = eng.live()
        failed = 0
        for n in range(1, 50):
            eng.fail_alloc_after(n)
            try:
                r = eng.closest_rows(s)
            except BedgpuError as e:
                assert e.code == NOMEM and "injected" in e.msg, n
                failed += 1
                eng.fail_alloc_after(0)
                assert eng.live() == base, n
                continue
            finally:
                eng.fail_alloc_after(0)
            break
        else:
            pytest.fail("the injected failure never stopped firing")
        assert failed >= 3  # left / right, then the scan's state blocks
        held = eng.live()
        # the export takes no device block of the context's: an armed failure has nothing to hit
        # (were one added, the call must fail with NOMEM and leave the pair as it was)
        for n in range(1, 4):
            eng.fail_alloc_after(n)
            try:
                got = r.closest()
            except BedgpuError as e:
                assert e.code == NOMEM and "injected" in e.msg, n
                got = None
            finally:
                eng.fail_alloc_after(0)
            assert eng.live() == held, n
            if got is not None:
                same(host(got), {k: want[k] for k in COLS4})
        r.free()
        assert eng.live() == base
    finally:
        s.free()


@pytest.mark.parametrize("key", ["stair300", "clamp", "rand-nested"])
def test_the_scan_launches_what_closest_op_launches(eng, key):
    Q, C = inputs(key)
    s = eng.load([(id_text(Q), BED3_REST), (id_text(C), BED3_REST)])
    try:
        r0, a = kernel_paths.launches(eng, lambda: eng.closest_op(s))
        r1, b = kernel_paths.launches(eng, lambda: eng.closest_rows(s))
        assert a == b and a.get("k_closest_chunks", 0) >= 1
        assert all(k.startswith("k_closest_") and k != "k_closest_export" for k in b), b
        _, c = kernel_paths.launches(eng, r1.closest)
        assert c == {"k_closest_export": 1}
        _, c = kernel_paths.launches(eng, lambda: r0.closest(shortest=True))
        assert c == {"k_closest_export": 1}
        r0.free()
        r1.free()
    finally:
        s.free()
    sc = eng.load_columns([col_input(Q), col_input(C)])
    try:
        r2, d = kernel_paths.launches(eng, lambda: eng.closest_rows(sc))
        assert d == a
        r2.free()
    finally:
        sc.free()
