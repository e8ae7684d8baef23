"""The overlap join behind a bedmap result as index columns (bg_result_map_pairs,
bg_result_export_map_pairs, Result.pairs): for every reference row the map rows in S(r), as
indices into the map table, ascending.

Oracles (never the code under test): the text route the reference fixtures pin, --echo-map-id on
the same rows loaded as BED5 text whose id column is the map row's index, each line parsed into a
sorted list of ints; and for --bp-ovr an independent numpy brute force over all row pairs.

Shapes: 1,500 x 1,500 rows over 4 chromosomes for the criteria; for the flat kernel, reference
row counts around its workgroup of 256 rows (1, 255, 256, 257, 1,025) with a chromosome change
inside a workgroup, chromosomes present in one table only, rows without members at a workgroup's
first and last position, and one reference row holding 5,000 map rows (more than a round of 256
slots); map rows of length 10,000, 100,000 and chromosome length for the per-row kernel."""
import ctypes
import random

import numpy as np
import pytest
import torch

import kernel_paths
import randbed

pytestmark = pytest.mark.gpu

# A torch wheel that bundles its own HIP runtime finds no device once libbedgpu's runtime has
# initialised it: a process that uses both starts torch's first, as
# bench.py does. In a whole-suite run other modules open engines before this module's tests
# run, and no fixture of this module can come before them, so torch's runtime is started
# here, when the module is collected; without a GPU this does nothing. The `eng` fixture
# checks that it is up and says so clearly otherwise.
if torch.cuda.is_available():
    torch.cuda.init()

BED3, BED3_REST, BED5, BED5_REST = 0, 1, 2, 4
ARG, NOMEM = -6, -7
NT = 256  # reference rows per workgroup of k_pairs_flat (BG_NT)


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
def bed3(rows):
    return "".join(f"{c}\t{s}\t{e}\n" for c, s, e in rows).encode()


def id_text(rows):
    """BED5 text whose id is the row's index"""
    return "".join(f"{c}\t{s}\t{e}\t{i}\t0\n" for i, (c, s, e) in enumerate(rows)).encode()


def col_input(rows):
    names = sorted({r[0] for r in rows}, key=lambda s: s.encode())[::-1]  # not strcmp order
    idx = {nm: k for k, nm in enumerate(names)}
    cols = [torch.tensor([idx[r[0]] for r in rows], dtype=torch.int32),
            torch.tensor([r[1] for r in rows], dtype=torch.int64),
            torch.tensor([r[2] for r in rows], dtype=torch.int64)]
    return (names, *[c.to("cuda:0") for c in cols], BED3)


def srt(rows):
    return sorted(rows, key=lambda r: (r[0].encode(), r[1], r[2]))


def _base():
    rng = random.Random(20261020)
    mk = lambda n, **kw: randbed.rows(rng, n, span=60000, maxlen=200, **kw)
    m = mk(1500)
    r = srt(mk(1300) + rng.sample(m, 200))  # (rows equal to a map row, for --exact)
    zr, zm = mk(1500, zero_frac=0.05), mk(1500, zero_frac=0.05)
    # long map rows: two length classes; 11 (a chromosome-long row); more than 16
    lm4 = mk(1500) + [("chr1", 500, 10500), ("chr10", 20000, 30000), ("chr2", 100, 5100)]
    lm = lm4 + [("chr2", 100, 100100), ("chr2", 30000, 130000), ("chrX", 0, 5000000)]
    lm30 = lm + [("chr10", 3, 600000000)]
    return {"r": r, "m": m, "zr": zr, "zm": zm, "lm4": srt(lm4), "lm": srt(lm), "lm30": srt(lm30)}


B = _base()

CRITS = [("bp-ovr", 1), ("bp-ovr", 50), ("range", 100), ("fraction-ref", 0.5), ("fraction-map", 0.5),
         ("fraction-either", 0.5), ("fraction-both", 0.5), ("fraction-map", 1e-17), ("exact", None)]
CRIT_IDS = [f"{c}-{v}" for c, v in CRITS]


def crit_kw(crit, val):
    return {"criterion": crit, "overlap_bp": val} if crit == "bp-ovr" else {"criterion": crit, "value": val}


# ------------------------------------------------------------------ oracles
_ORACLE = {}


def text_route(eng, ref, mp, crit, val, faster=False):
    """the members of every reference row by --echo-map-id (mp None: single-file mode), as sorted
    lists of map-row indices; computed once per input and criterion"""
    key = (tuple(ref), None if mp is None else tuple(mp), crit, val, faster)
    if key not in _ORACLE:
        single = mp is None
        out = eng.bedmap(["echo-map-id"], id_text(ref) if single else bed3(ref), None if single else id_text(mp),
                         faster=faster, **crit_kw(crit, val))
        lines = out.decode().split("\n")[:-1]
        assert len(lines) == len(ref)
        _ORACLE[key] = [sorted(int(x) for x in ln.split(";") if x) for ln in lines]
    return _ORACLE[key]


def brute_bp(ref, mp, ovr):
    """--bp-ovr by all pairs (inputs without zero-length rows: the sweep window is then every
    overlapping row)"""
    mp = ref if mp is None else mp
    chroms = {c: k for k, c in enumerate(sorted({r[0] for r in ref + mp}))}
    rc, rs, re = (np.array([f(r) for r in ref], dtype=np.int64) for f in
                  (lambda r: chroms[r[0]], lambda r: r[1], lambda r: r[2]))
    mc, ms, me = (np.array([f(r) for r in mp], dtype=np.int64) for f in
                  (lambda r: chroms[r[0]], lambda r: r[1], lambda r: r[2]))
    out = []
    for i in range(len(ref)):
        ov = np.minimum(re[i], me) - np.maximum(rs[i], ms)
        out.append(np.nonzero((mc == rc[i]) & (ov >= ovr))[0].tolist())
    return out


# ------------------------------------------------------------------ the code under test
def map_result(eng, ref, mp, crit, val, cols=False, ops=("count",), faster=False, skip_unmapped=False):
    """(set, result) of bedmap <ops> on the rows loaded as text or as device columns"""
    single = mp is None
    if cols:
        s = eng.load_columns([col_input(ref)] + ([] if single else [col_input(mp)]))
    else:
        # (an --echo-map-* operation: the kinds Engine.bedmap loads for it)
        echo = any(o.startswith("echo-map") for o in ops)
        ids = "echo-map-id" in ops
        if single:
            s = eng.load([(id_text(ref) if ids else bed3(ref), BED3_REST if echo else BED3)])
        else:
            s = eng.load([(bed3(ref), BED3_REST if echo else BED3),
                          (id_text(mp) if ids else bed3(mp), BED5_REST if ids else BED3)])
    try:
        kw = crit_kw(crit, val)
        r = eng.map_op(s, list(ops), 0, 0 if single else 1, faster=faster, skip_unmapped=skip_unmapped,
                       overlap_bp=kw.get("overlap_bp", 1), criterion=kw["criterion"], value=kw.get("value"))
    except Exception:
        s.free()
        raise
    return s, r


def lists(p):
    off, mr = p["offsets"].cpu().numpy(), p["map_rows"].cpu().numpy()
    return [mr[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]


def check_shape(p, nref):
    """what every export must satisfy, whatever the members are"""
    off, mr, rr = (p[k].cpu().numpy() for k in ("offsets", "map_rows", "ref_rows"))
    assert off.dtype == mr.dtype == rr.dtype == np.int64
    assert len(off) == nref + 1 and off[0] == 0 and (np.diff(off) >= 0).all()
    assert len(mr) == len(rr) == off[-1]
    assert (rr == np.repeat(np.arange(nref, dtype=np.int64), np.diff(off))).all()
    for i in range(nref):  # ascending inside a row (strictly: a row is listed once)
        assert (np.diff(mr[off[i]:off[i + 1]]) > 0).all(), i


def pairs_of(eng, ref, mp, crit, val, kernel=None, **kw):
    """Result.pairs() of a fresh result, its shape checked against the count export; `kernel`:
    the fill kernel that has to run (and the other one not)"""
    s, r = map_result(eng, ref, mp, crit, val, **kw)
    try:
        total = r.pairs_total()
        p, ran = kernel_paths.launches(eng, r.pairs)
        check_shape(p, len(ref))
        assert total == int(p["offsets"][-1])
        if ref:  # (bg_result_export_map takes no empty buffer)
            cnt = r.columns(list(kw.get("ops", ("count",))).index("count"))["values"].cpu().numpy()
            assert (np.diff(p["offsets"].cpu().numpy()) == cnt.astype(np.int64)).all()
        if kernel and total:
            other = {"k_pairs_flat": "k_pairs_rows", "k_pairs_rows": "k_pairs_flat"}[kernel]
            assert ran.get(kernel) == 1 and other not in ran, ran
        return lists(p)
    finally:
        r.free()
        s.free()


# ------------------------------------------------------------------ 1. every criterion, both modes
@pytest.mark.parametrize("single", [False, True], ids=["two-file", "single-file"])
@pytest.mark.parametrize("crit,val", CRITS, ids=CRIT_IDS)
def test_pairs_match_the_text_route(eng, crit, val, single):
    ref, mp = (B["m"], None) if single else (B["r"], B["m"])
    want = text_route(eng, ref, mp, crit, val)
    assert sum(map(len, want)) > 100  # the case says something
    got = pairs_of(eng, ref, mp, crit, val, kernel="k_pairs_flat")
    assert got == want
    if crit == "bp-ovr":
        assert got == brute_bp(ref, mp, val)
    # the same tables from device columns: identical pairs
    assert pairs_of(eng, ref, mp, crit, val, kernel="k_pairs_flat", cols=True) == got


@pytest.mark.parametrize("single", [False, True], ids=["two-file", "single-file"])
@pytest.mark.parametrize("crit,val", [("bp-ovr", 1), ("range", 100)], ids=["bp-ovr", "range"])
def test_zero_length_rows(eng, crit, val, single):
    ref, mp = (B["zm"], None) if single else (B["zr"], B["zm"])
    assert any(s == e for _, s, e in ref)
    want = text_route(eng, ref, mp, crit, val)
    assert pairs_of(eng, ref, mp, crit, val, kernel="k_pairs_flat") == want
    assert pairs_of(eng, ref, mp, crit, val, cols=True) == want


@pytest.mark.parametrize("key,crit,val", [("lm", "bp-ovr", 1), ("lm", "range", 100), ("lm", "fraction-ref", 0.5),
                                          ("lm4", "bp-ovr", 1), ("lm30", "bp-ovr", 1)],
                         ids=["bp-ovr", "range", "fraction-ref", "two-classes", "18-classes"])
def test_long_rows_take_the_per_row_kernel(eng, key, crit, val):
    ref, mp = B["r"], B[key]
    want = text_route(eng, ref, mp, crit, val)
    got = pairs_of(eng, ref, mp, crit, val, kernel="k_pairs_rows")
    assert got == want
    if crit == "bp-ovr":
        assert got == brute_bp(ref, mp, val)
    assert pairs_of(eng, ref, mp, crit, val, kernel="k_pairs_rows", cols=True) == got
    # with the windows kept (NEED_WIN) the same pairs
    assert pairs_of(eng, ref, mp, crit, val, kernel="k_pairs_rows", ops=("count", "echo-map-size")) == got


# ------------------------------------------------------------------ 2. the flat kernel's boundaries
def boundary_tables(n):
    """n reference rows, 100 bp apart: chrA up to row min(150, n // 2), then chrB, the last three on
    chrZ (no map rows there); map rows every 37 bp on chrA and chrB, none near the reference rows
    at a workgroup's first and last position, and five on chr0 (no reference rows there)"""
    cut = min(150, n // 2)
    nz = 3 if n >= 10 else 0
    ref = [("chrA" if i < cut else "chrZ" if i >= n - nz else "chrB", 100 * i, 100 * i + 60) for i in range(n)]
    bare = [i for i in range(n) if i % NT in (0, NT - 1)]
    mp = [("chr0", 10 * k, 10 * k + 25) for k in range(5)]
    for ch in ("chrA", "chrB"):
        for st in range(0, 100 * n + 100, 37):
            if not any(100 * i - 50 < st < 100 * i + 60 for i in (st // 100, st // 100 + 1) if i in bare):
                mp.append((ch, st, st + 50))
    return ref, srt(mp), bare


@pytest.mark.parametrize("n", [1, NT - 1, NT, NT + 1, 4 * NT + 1])
def test_flat_kernel_boundaries(eng, n):
    ref, mp, bare = boundary_tables(n)
    want = brute_bp(ref, mp, 1)
    assert all(not want[i] for i in bare)
    if n > 1:
        cut = min(150, n // 2)  # a chromosome change inside the first workgroup
        assert sum(map(len, want)) > 0 and cut < NT and ref[cut - 1][0] != ref[cut][0]
    assert text_route(eng, ref, mp, "bp-ovr", 1) == want
    assert pairs_of(eng, ref, mp, "bp-ovr", 1, kernel="k_pairs_flat") == want
    assert pairs_of(eng, ref, mp, "bp-ovr", 1, kernel="k_pairs_flat", cols=True) == want
    assert pairs_of(eng, ref, mp, "range", 100, cols=True) == text_route(eng, ref, mp, "range", 100)


def test_one_row_holding_more_than_a_round(eng):
    # (a long REFERENCE row: the map rows stay short, so the flat kernel runs)
    ref = srt([("chrA", 40 * i, 40 * i + 30) for i in range(300)] + [("chrA", 5, 2000000)])
    mp = [("chrA", 300 * k, 300 * k + 100) for k in range(5200)]
    want = brute_bp(ref, mp, 1)
    assert max(map(len, want)) >= 5000
    assert pairs_of(eng, ref, mp, "bp-ovr", 1, kernel="k_pairs_flat") == want
    assert pairs_of(eng, ref, mp, "bp-ovr", 1, kernel="k_pairs_flat", cols=True) == want
    assert text_route(eng, ref, mp, "bp-ovr", 1) == want


@pytest.mark.parametrize("cols", [False, True], ids=["text", "columns"])
def test_empty_tables(eng, cols):
    got = pairs_of(eng, B["r"], [], "bp-ovr", 1, cols=cols)  # (check_shape: offsets all zero)
    assert got == [[] for _ in B["r"]]
    assert pairs_of(eng, [], B["m"], "bp-ovr", 1, cols=cols) == []


# ------------------------------------------------------------------ 3. consistency
@pytest.mark.parametrize("crit,val", [("bp-ovr", 1), ("range", 100), ("fraction-map", 1e-17), ("exact", None)],
                         ids=["bp-ovr", "range", "touch", "exact"])
def test_same_pairs_with_and_without_kept_windows(eng, crit, val):
    want = text_route(eng, B["r"], B["m"], crit, val)
    assert pairs_of(eng, B["r"], B["m"], crit, val, ops=("count",)) == want
    assert pairs_of(eng, B["r"], B["m"], crit, val, ops=("count", "echo-map-size")) == want


@pytest.mark.parametrize("crit,val", [("bp-ovr", 1), ("bp-ovr", 30), ("range", 50), ("fraction-both", 0.5),
                                      ("exact", None)], ids=["bp-ovr-1", "bp-ovr-30", "range", "fraction-both", "exact"])
def test_faster(eng, crit, val):
    # nested rows: every row of a nest of five contains the next
    rng = random.Random(7)
    ref = srt([("chr1", 1000 * k + 10 * j, 1000 * k + 400 - 10 * j) for k in range(40) for j in range(5)])
    mp = srt(ref[::3] + [("chr1", s + rng.randint(0, 40), e + rng.randint(0, 40)) for _, s, e in ref[::2]])
    want = text_route(eng, ref, mp, crit, val, faster=True)
    assert sum(map(len, want)) > 50
    assert pairs_of(eng, ref, mp, crit, val, faster=True, kernel="k_pairs_flat") == want


# ------------------------------------------------------------------ 4. the contract
def _raw(eng, r, offsets, ref_rows, map_rows, cap):
    ptr = lambda t: None if t is None else t.data_ptr()
    eng.sync_torch()
    rc = eng.L.bg_result_export_map_pairs(eng.ctx, r.h, ptr(offsets), ptr(ref_rows), ptr(map_rows), cap)
    eng.sync()
    return rc


def test_refusals_and_the_cap(eng):
    from bedops_amd.engine import BedgpuError
    s = eng.load([(bed3(B["r"]), BED3), (bed3(B["m"]), BED3)])
    try:
        ivl = eng.op("-m", s, [0, 1])
        n = ctypes.c_uint64()
        assert eng.L.bg_result_map_pairs(eng.ctx, ivl.h, ctypes.byref(n)) == ARG
        assert eng.L.bg_result_export_map_pairs(eng.ctx, ivl.h, None, None, None, 0) == ARG
        assert "not a bedmap result" in eng.L.bg_last_error(eng.ctx).decode()
        ivl.free()
        sk = eng.map_op(s, ["count"], 0, 1, skip_unmapped=True)
        with pytest.raises(BedgpuError) as ei:
            sk.pairs_total()
        assert ei.value.code == ARG and "skip-unmapped" in ei.value.msg
        assert eng.L.bg_result_export_map_pairs(eng.ctx, sk.h, None, None, None, 0) == ARG
        sk.free()
        r = eng.map_op(s, ["count"], 0, 1)
        want = r.pairs()
        total = r.pairs_total()
        assert total > 1000
        mk = lambda k: torch.full((k,), -7, dtype=torch.int64, device="cuda:0")
        # one element short: refused, and nothing written
        off, rr, mr = mk(len(B["r"]) + 1), mk(total + 2), mk(total + 2)
        assert _raw(eng, r, off, rr, mr, total - 1) == ARG
        assert "room for" in eng.L.bg_last_error(eng.ctx).decode()
        assert bool((rr == -7).all()) and bool((mr == -7).all())
        assert _raw(eng, r, off, None, None, 0) == 0  # no pair column asked for: cap does not matter
        assert torch.equal(off, want["offsets"])
        # exactly enough: the element after the buffer's cap stays
        assert _raw(eng, r, None, rr, mr, total) == 0
        assert torch.equal(rr[:total], want["ref_rows"]) and torch.equal(mr[:total], want["map_rows"])
        assert bool((rr[total:] == -7).all()) and bool((mr[total:] == -7).all())
        # NULL columns are skipped, one at a time
        rr2, mr2 = mk(total), mk(total)
        assert _raw(eng, r, None, rr2, None, total) == 0 and torch.equal(rr2, want["ref_rows"])
        assert _raw(eng, r, None, None, mr2, total) == 0 and torch.equal(mr2, want["map_rows"])
        p = r.pairs(ref_rows=False)
        assert sorted(p) == ["map_rows", "offsets"] and torch.equal(p["map_rows"], want["map_rows"])
        r.free()
    finally:
        s.free()


def test_count_is_idempotent(eng):
    s, r = map_result(eng, B["r"], B["m"], "bp-ovr", 1)
    try:
        total, first = kernel_paths.launches(eng, r.pairs_total)
        assert first.get("k_pairs_widen") == 1 and first.get("k_tile_scan", 0) >= 1
        again, second = kernel_paths.launches(eng, r.pairs_total)
        assert again == total and second == {}
        _, fill = kernel_paths.launches(eng, r.pairs)  # the export reuses the count
        assert "k_pairs_widen" not in fill and fill.get("k_pairs_flat") == 1
    finally:
        r.free()
        s.free()


@pytest.mark.parametrize("mp_key", ["m", "lm"], ids=["flat", "long-rows"])
def test_format_and_pairs_do_not_disturb_each_other(eng, mp_key):
    ref, mp = B["r"], B[mp_key]
    want = text_route(eng, ref, mp, "bp-ovr", 1)
    s, r = map_result(eng, ref, mp, "bp-ovr", 1, ops=("count", "echo-map-id"))
    try:
        t1 = r.text()
        p1 = r.pairs()
        assert r.text() == t1
        assert lists(p1) == want
    finally:
        r.free()
        s.free()
    s, r = map_result(eng, ref, mp, "bp-ovr", 1, ops=("count", "echo-map-id"))
    try:
        p1 = r.pairs()
        assert r.text() == t1
        p2 = r.pairs()
        assert all(torch.equal(p1[k], p2[k]) for k in p1) and lists(p2) == want
    finally:
        r.free()
        s.free()


# ------------------------------------------------------------------ 5. allocation discipline
def test_live_balances_and_injected_failures(eng):
    from bedops_amd.engine import BedgpuError
    want = text_route(eng, B["r"], B["m"], "bp-ovr", 1)
    s = eng.load([(bed3(B["r"]), BED3), (bed3(B["m"]), BED3)])
    try:
        base = eng.live()
        r = eng.map_op(s, ["count"], 0, 1)
        assert lists(r.pairs()) == want
        assert eng.live()[0] > base[0]  # (the offsets are the result's)
        r.free()
        assert eng.live() == base
        failed = 0
        for n in range(1, 50):
            r = eng.map_op(s, ["count"], 0, 1)
            held = eng.live()
            eng.fail_alloc_after(n)
            try:
                got = r.pairs()
            except BedgpuError as e:
                assert e.code == NOMEM and "injected" in e.msg, n
                eng.fail_alloc_after(0)
                assert eng.live() == held, n
                assert lists(r.pairs()) == want, n  # a following call succeeds
                failed += 1
                continue
            finally:
                eng.fail_alloc_after(0)
                r.free()
                assert eng.live() == base, n
            assert lists(got) == want
            break
        else:
            pytest.fail("the injected failure never stopped firing")
        assert failed >= 2  # the offsets and the scan's partial sums
    finally:
        s.free()
