"""bg_sort_columns (Engine.sort_columns, Engine.load_columns(sort=True)): one columnar input put
into the order bg_load_columns accepts, on the GPU.

The reference is numpy on the host: the names' ranks under bytewise comparison, then
np.lexsort((end, start, rank)), which is stable. `order` must equal that permutation exactly,
and every output column must be input[order].

Shapes: row counts around every boundary the kernels have (a lane's 4 rows, a wave's 256, a
workgroup round of SC_CHUNK rows, the radix sort's RS_TILE keys, several rounds per workgroup
through BEDGPU_COLS_BLOCKS), inputs with many rows equal in (chrom, start, end) and distinct
scores so that a stability error shows, key widths on both sides of every digit-pass count and
of the 64-bit packed key, and name lists on both sides of the LDS rank table's capacity."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import kernel_paths
from conftest import ROOT

pytestmark = pytest.mark.gpu

# torch's HIP runtime starts before libbedgpu opens the device (see tests/test_gpu_columns.py)
if torch.cuda.is_available():
    torch.cuda.init()

BED3, BED5, BED3_SET = 0, 2, 3
UNSORTED, RANGE, ARG, NOMEM, UNSUPPORTED, CHROM = -3, -4, -6, -7, -8, -9
COORD_MAX = (1 << 40) - 1


def _define(path, name):
    src = open(os.path.join(ROOT, "bedops_amd", "csrc", path)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, src).group(1))


NT = _define("bg_internal.h", "BG_NT")
LANE_ROWS = _define("bg_sortcols.hip", "SC_ROWS")
CHUNK = NT * LANE_ROWS  # rows a workgroup takes per round
WAVE = 64 * LANE_ROWS
RS_TILE = _define("bg_sort.hip", "RS_NT") * _define("bg_sort.hip", "RS_ITEMS")
LDS_NAMES = _define("bg_sortcols.hip", "SC_LDS_NAMES")
PLAN_CHECK = os.path.join(ROOT, "tools", "build", "sort_plan_check")


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


@pytest.fixture(scope="module")
def plan_passes():
    """digit passes (round 0 + round 1) of the host plan for (rows, names, max start, max length)"""
    subprocess.run(["make", "-s", "tools/build/sort_plan_check"], cwd=ROOT, check=True)

    def run(n, names, max_start, max_len):
        out = subprocess.run([PLAN_CHECK, str(n), str(names), str(max_start), str(max_len)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        m = re.search(r"packed=(\d) .* passes=(\d+),(\d+)\n", out)
        assert m, out
        return bool(int(m.group(1))), int(m.group(2)) + int(m.group(3))
    return run


# ------------------------------------------------------------------ the reference
def ranks(names):
    by = sorted(range(len(names)), key=lambda k: names[k].encode())
    r = np.zeros(max(len(names), 1), dtype=np.int64)
    r[by] = np.arange(len(names))
    return r


def reference(names, chrom, start, end):
    return np.lexsort((end, start, ranks(names)[chrom])) if len(chrom) else np.zeros(0, dtype=np.int64)


def check(eng, names, chrom, start, end, score=None, device=True):
    """sort on the GPU, compare with numpy; returns the order"""
    chrom, start, end = np.asarray(chrom, np.int32), np.asarray(start, np.int64), np.asarray(end, np.int64)
    cols = [chrom, start, end] + ([np.asarray(score, np.float64)] if score is not None else [])
    t = [torch.as_tensor(c) for c in cols]
    if device:
        t = [x.to("cuda:0") for x in t]
    got = eng.sort_columns(names, *t)
    want = reference(names, chrom, start, end)
    order = got["order"].cpu().numpy()
    assert got["order"].dtype == torch.int64 and got["order"].is_cuda
    assert np.array_equal(order, want)
    assert got["names"] == list(names)
    for k, c in zip(("chrom", "start", "end", "score"), cols):
        assert got[k].is_cuda and got[k].cpu().numpy().dtype == c.dtype, k
        assert np.array_equal(got[k].cpu().numpy(), c[want]), k
    assert ("score" in got) == (score is not None)
    return order


def tied_rows(n, seed, nnames=5):
    """n shuffled rows over few distinct (chrom, start, end) triples: every triple repeats, and the
    scores (the input row numbers) tell equal rows apart"""
    rng = np.random.default_rng(seed)
    names = [f"chr{k}" for k in (10, 2, 1, "X", 21)][:nnames]
    chrom = rng.integers(0, nnames, n)
    start = rng.integers(0, max(2, n // 64), n) * 10
    end = start + rng.integers(0, 3, n)
    return names, chrom, start, end, np.arange(n, dtype=np.float64)


# ------------------------------------------------------------------ T1. order and stability
COUNTS = [0, 1, 2, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1, RS_TILE - 1, RS_TILE,
          RS_TILE + 1, 4 * CHUNK + 1, 3 * RS_TILE + 5]
GRIDS = [(n, None) for n in COUNTS] + [(n, b) for n in COUNTS if n > CHUNK for b in (1, 2)]


def test_the_counts_are_the_boundaries():
    assert COUNTS == [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 3 * 2048 + 5]


@pytest.mark.parametrize("n,blocks", GRIDS)
def test_order_and_stability(eng, monkeypatch, n, blocks):
    if blocks is not None:
        monkeypatch.setenv("BEDGPU_COLS_BLOCKS", str(blocks))  # one workgroup runs several rounds
    names, chrom, start, end, score = tied_rows(n, seed=n)
    if n > 64:  # the point of the input: equal rows whose order only stability decides
        trip = np.stack([chrom, start, end])
        assert len(np.unique(trip, axis=1)[0]) < n // 2
    check(eng, names, chrom, start, end, score, device=(n % 2 == 1))
    check(eng, names, chrom, start, end)


# ------------------------------------------------------------------ T2. key widths
def width_rows(nnames, max_start, max_len, n=3000, seed=7):
    """rows whose largest start and length are exactly the given ones; names c000.. reversed"""
    rng = np.random.default_rng(seed)
    names = [f"c{k:04d}" for k in range(nnames)][::-1]
    chrom = rng.integers(0, nnames, n)
    m = min(n - 3, nnames)
    chrom[:m] = np.arange(m)  # every name has a row
    start = rng.integers(0, max_start + 1, n)
    ln = rng.integers(0, max_len + 1, n)
    ln = np.minimum(ln, COORD_MAX - start)
    start[-1], ln[-1] = max_start, 0
    start[-2], ln[-2] = min(max_start, COORD_MAX - max_len), max_len
    start[-3], ln[-3] = start[-2], max(0, max_len - 1)  # one (chrom, start), two ends
    chrom[-3] = chrom[-2]
    return names, chrom, start, start + ln


def two_round(eng, call):
    _, k = kernel_paths.launches(eng, call)
    assert k.get("k_sc_key") == 1 and k.get("k_sc_gather") == 1
    return k.get("k_sc_key2", 0) == 1, k.get("k_rs_scatter", 0)


@pytest.mark.parametrize("bits", [1, 8, 9, 16, 17])
def test_one_name_and_start_only_keys(eng, plan_passes, bits):
    names, chrom, start, end = width_rows(1, (1 << bits) - 1, 0)
    two, scat = two_round(eng, lambda: check(eng, names, chrom, start, end))
    assert not two and scat == (bits + 7) // 8 == plan_passes(len(chrom), 1, (1 << bits) - 1, 0)[1]


@pytest.mark.parametrize("nnames,max_len,packed", [(16, (1 << 20) - 1, True), (17, (1 << 20) - 1, False),
                                                   (16, 1 << 20, False)])
def test_the_64_bit_packed_key_and_its_65_bit_neighbours(eng, plan_passes, nnames, max_len, packed):
    names, chrom, start, end = width_rows(nnames, COORD_MAX, max_len)
    assert int(start.max()) == COORD_MAX and int((end - start).max()) == max_len
    two, scat = two_round(eng, lambda: check(eng, names, chrom, start, end))
    want_packed, passes = plan_passes(len(chrom), nnames, COORD_MAX, max_len)
    assert want_packed == packed and two == (not packed) and scat == passes
    check(eng, names, chrom, start, end, np.arange(len(chrom)), device=False)


@pytest.mark.parametrize("nnames", [LDS_NAMES, LDS_NAMES + 1, 3000])
def test_name_lists_around_the_lds_rank_table(eng, nnames):
    """past SC_LDS_NAMES names the kernels read the rank table from global memory"""
    names, chrom, start, end = width_rows(nnames, 50, 9, n=6000)
    assert len(set(chrom.tolist())) == nnames
    check(eng, names, chrom, start, end, np.arange(6000))
    # the same names with 40-bit starts and long rows: the two-round kernels with that table
    names, chrom, start, end = width_rows(nnames, COORD_MAX, (1 << 30) + 3, n=6000)
    two, _ = two_round(eng, lambda: check(eng, names, chrom, start, end))
    assert two


def test_name_orders(eng):
    rng = np.random.default_rng(3)
    n = 2000
    start = rng.integers(0, 500, n)
    end = start + rng.integers(0, 50, n)
    # list order the reverse of strcmp order
    names = sorted([f"s{k:02d}" for k in range(40)], key=lambda s: s.encode())[::-1]
    check(eng, names, rng.integers(0, 40, n), start, end)
    # strcmp is not natural order: chr10 < chr2, chr1 < chr10, chrX last, "chr" prefixes
    names = ["chr1", "chr2", "chr10", "chrX", "chr", "chr1_alt", "Chr3", "chr21"]
    chrom = rng.integers(0, len(names), n)
    order = check(eng, names, chrom, start, end)
    seq = [names[c] for c in chrom[order]]
    first = {nm: seq.index(nm) for nm in names}
    assert first["Chr3"] < first["chr"] < first["chr1"] < first["chr10"] < first["chr1_alt"] < first["chr2"] \
        < first["chr21"] < first["chrX"]


# ------------------------------------------------------------------ T3. the path is the planned one
def sorted_rows(n):
    """n distinct rows in order over 3 names (list order = strcmp order), some equal starts"""
    chrom = np.minimum(np.arange(n) * 3 // max(n, 1), 2)
    start = 10 * (np.arange(n) // 2)
    end = start + 1 + np.arange(n) % 2
    return ["a", "b", "c"], chrom, start, end


@pytest.mark.parametrize("blocks", [None, 1])
def test_sorted_input_runs_no_digit_pass(eng, monkeypatch, blocks):
    if blocks is not None:
        monkeypatch.setenv("BEDGPU_COLS_BLOCKS", str(blocks))
    for n in (2, CHUNK, 3 * CHUNK + 7):
        names, chrom, start, end = sorted_rows(n)
        order, k = kernel_paths.launches(eng, lambda: check(eng, names, chrom, start, end, np.arange(n)))
        assert np.array_equal(order, np.arange(n))
        assert k == {"k_sc_key": 1, "k_sc_gather": 1}, k


@pytest.mark.parametrize("blocks", [None, 1])
@pytest.mark.parametrize("where", ["last-row", "wave-boundary", "round-boundary", "span-boundary", "ends-only"])
def test_one_swapped_pair_is_seen(eng, monkeypatch, plan_passes, where, blocks):
    if blocks is not None:
        monkeypatch.setenv("BEDGPU_COLS_BLOCKS", str(blocks))
    n = 3 * CHUNK + 7
    names, chrom, start, end = sorted_rows(n)
    r = {"last-row": n - 1, "wave-boundary": WAVE, "round-boundary": CHUNK, "span-boundary": 2 * CHUNK,
         "ends-only": 2 * CHUNK + 1}[where]
    if where == "ends-only":  # rows r - 1 and r share (chrom, start): only their ends are out of order
        assert chrom[r] == chrom[r - 1] and start[r] == start[r - 1] and end[r] > end[r - 1]
    for c in (chrom, start, end):
        c[[r - 1, r]] = c[[r, r - 1]]
    order, k = kernel_paths.launches(eng, lambda: check(eng, names, chrom, start, end))
    want = np.arange(n)
    want[[r - 1, r]] = want[[r, r - 1]]
    assert np.array_equal(order, want)
    packed, passes = plan_passes(n, 3, int(start.max()), int((end - start).max()))
    assert packed and passes > 0 and k.get("k_rs_scatter") == passes and k.get("k_sc_pack") == 1


def test_trivial_inputs_run_no_digit_pass(eng):
    for n in (0, 1):
        names, chrom, start, end, score = tied_rows(n, seed=1)
        _, k = kernel_paths.launches(eng, lambda: check(eng, names, chrom, start, end, score))
        assert "k_rs_scatter" not in k and "k_sc_pack" not in k


# ------------------------------------------------------------------ T4. round trip through the loader
def bed_text(names, chrom, start, end, score=None):
    o = reference(names, chrom, start, end)
    if score is None:
        return "".join(f"{names[chrom[i]]}\t{start[i]}\t{end[i]}\n" for i in o).encode()
    return "".join(f"{names[chrom[i]]}\t{start[i]}\t{end[i]}\tid\t{int(score[i])}\n" for i in o).encode()


def shuffled_input(n, seed):
    rng = np.random.default_rng(seed)
    names = ["chr2", "chr10", "chrX", "chr1"]
    chrom = rng.integers(0, 4, n).astype(np.int32)
    start = rng.integers(0, 40000, n).astype(np.int64)
    end = start + rng.integers(1, 200, n)
    score = rng.integers(-50, 1000, n).astype(np.float64)
    return names, chrom, start, end, score


def test_load_columns_sort_gives_the_text_engines_answers(eng):
    from bedops_amd import BedgpuError
    a, b = shuffled_input(1500, 11), shuffled_input(1300, 12)
    ta, tb = bed_text(*a[:4]), bed_text(*b[:4])
    tb5 = bed_text(*b)
    dev = lambda x: tuple(torch.as_tensor(c).to("cuda:0") for c in x[1:])
    base = eng.live()
    s = eng.load_columns([(a[0], *dev(a)[:3], BED3), (b[0], *b[1:4], BED3)], sort=True)
    try:
        assert isinstance(s.order, list) and len(s.order) == 2
        for x, o in zip((a, b), s.order):
            assert o.dtype == torch.int64
            assert np.array_equal(o.cpu().numpy(), reference(*x[:4]))
            assert torch.equal(o, eng.sort_columns(x[0], *x[1:4])["order"])
        for mode in ("-m", "-i"):
            r = eng.op(mode, s, [0, 1])
            try:
                assert r.text() == eng.bedops(mode, [ta, tb]) and len(r.text()) > 0
            finally:
                r.free()
    finally:
        s.free()
    s = eng.load_columns([(a[0], *dev(a)[:3], BED3), (b[0], *dev(b), BED5)], sort=True)
    try:
        r = eng.map_op(s, ["count", "sum"])
        try:
            want = eng.bedmap(["count", "sum"], ta, tb5)
            assert r.text() == want and b"|" in want
        finally:
            r.free()
    finally:
        s.free()
    assert eng.live() == base
    # without sort the same rows are refused, and a sorted input has no order
    with pytest.raises(BedgpuError) as ei:
        eng.load_columns([(a[0], *dev(a)[:3], BED3)])
    assert ei.value.code == UNSORTED
    o = reference(*a[:4])
    s = eng.load_columns([(a[0], a[1][o], a[2][o], a[3][o], BED3)])
    try:
        assert s.order is None and s.rows(0) == 1500
    finally:
        s.free()
    assert eng.live() == base


# ------------------------------------------------------------------ T5. refusals
def raw_sort(eng, names, cols, kind, outs):
    """bg_sort_columns through ctypes: cols / outs are device tensors or None; returns the code"""
    from bedops_amd.engine import _Columns
    nm = (ctypes.c_char_p * max(len(names), 1))(*[x.encode() for x in names])
    a = _Columns()
    a.n = cols[0].numel()
    a.chrom, a.start, a.end = (c.data_ptr() for c in cols[:3])
    a.score = cols[3].data_ptr() if len(cols) > 3 and cols[3] is not None else None
    a.names, a.nnames, a.on_device, a.kind = nm, len(names), 1, kind
    eng.sync_torch()
    rc = eng.L.bg_sort_columns(eng.ctx, ctypes.byref(a), *[o.data_ptr() if o is not None else None for o in outs])
    eng.sync()
    return rc


def good_rows():
    n = 3 * CHUNK
    rng = np.random.default_rng(5)
    return ["chrB", "chrA"], rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 9000, n), \
        rng.integers(9000, 9100, n)


def _chrom(row, v):
    def f(c, s, e):
        c[row] = v
    return f, row, ARG


def _neg(c, s, e):
    s[700] = -1


def _past(c, s, e):
    e[CHUNK + 1] = 1 << 40


def _inverted(c, s, e):
    s[5], e[5] = 100, 99


def _two(c, s, e):
    e[2000] = 1 << 40
    c[1200] = 2
    s[2999] = -4


N3 = 3 * CHUNK
BAD = {"chrom=-1,first": _chrom(0, -1), "chrom=len,first": _chrom(0, 2), "chrom=-1,last": _chrom(N3 - 1, -1),
       "chrom=len,last": _chrom(N3 - 1, 2), "chrom=-1,mid-tile": _chrom(CHUNK + 517, -1),
       "chrom=len,mid-tile": _chrom(CHUNK + 517, 2), "negative-start": (_neg, 700, RANGE),
       "end=2^40": (_past, CHUNK + 1, RANGE), "start>end": (_inverted, 5, RANGE), "lower-of-three": (_two, 1200, ARG)}


@pytest.mark.parametrize("blocks", [None, 1])
@pytest.mark.parametrize("case", list(BAD))
def test_bad_rows_are_named(eng, monkeypatch, case, blocks):
    from bedops_amd import BedgpuError
    if blocks is not None:
        monkeypatch.setenv("BEDGPU_COLS_BLOCKS", str(blocks))
    edit, row, code = BAD[case]
    names, c, s, e = good_rows()
    good = (c.copy(), s.copy(), e.copy())
    edit(c, s, e)
    base = eng.live()
    for dev in ("cuda:0", "cpu"):
        with pytest.raises(BedgpuError) as ei:
            eng.sort_columns(names, *[torch.as_tensor(x).to(dev) for x in (c, s, e)])
        assert ei.value.code == code, str(ei.value)
        assert f"row {row}:" in str(ei.value)
        assert eng.live() == base
        check(eng, names, *good)  # the engine is as good as before


def test_host_side_refusals(eng):
    from bedops_amd import BedgpuError
    z = lambda n=4, dt=torch.int64: torch.zeros(n, dtype=dt, device="cuda:0")
    sc = torch.ones(4, dtype=torch.float64, device="cuda:0")
    base = eng.live()
    for names, code in ((["chr1", "chr1"], ARG), (["chr1", ""], ARG), (["chr 1"], ARG), (["c" * 128], CHROM)):
        with pytest.raises(BedgpuError) as ei:
            eng.sort_columns(names, z(4, torch.int32), z(), z())
        assert ei.value.code == code, (names, str(ei.value))
        assert eng.live() == base
        check(eng, ["c" * 127], [0, 0], [5, 3], [9, 9])
    cols = [z(4, torch.int32), z(), z()]
    out = [torch.empty(4, dtype=torch.int64, device="cuda:0"), None, None, None, None]
    assert raw_sort(eng, ["chr1"], cols + [sc], BED3, out) == ARG      # a score with BED3
    assert raw_sort(eng, ["chr1"], cols + [None], BED5, out) == ARG    # BED5 without one
    assert raw_sort(eng, ["chr1"], cols + [None], 1, out) == ARG       # a kind with a remainder
    assert raw_sort(eng, ["chr1"], cols + [None], BED3, out[:4] + [sc.clone()]) == ARG  # a score asked of BED3
    assert raw_sort(eng, ["chr1"], cols + [None], BED3, out) == 0
    assert out[0].cpu().tolist() == [0, 1, 2, 3]
    assert raw_sort(eng, ["chr1"], cols + [None], BED3_SET, out) == 0  # (the kind says nothing about order)
    assert eng.live() == base


# ------------------------------------------------------------------ T6. host arrays, NULL outputs
def test_host_arrays_give_the_device_result(eng):
    names, chrom, start, end, score = tied_rows(CHUNK + 77, seed=9)
    want = check(eng, names, chrom, start, end, score)
    got = eng.sort_columns(names, chrom.astype(np.int32), start, end, score)  # numpy
    assert np.array_equal(got["order"].cpu().numpy(), want)
    assert np.array_equal(got["score"].cpu().numpy(), score[want])
    got = eng.sort_columns(names, chrom.tolist(), torch.as_tensor(start), torch.as_tensor(end))  # a list, CPU tensors
    assert np.array_equal(got["order"].cpu().numpy(), want) and "score" not in got
    assert np.array_equal(check(eng, names, chrom, start, end, score, device=False), want)


@pytest.mark.parametrize("n,in_order", [(CHUNK + 5, False), (CHUNK + 5, True), (3, False)])
def test_any_subset_of_outputs(eng, n, in_order):
    names, chrom, start, end, score = tied_rows(n, seed=21)
    if in_order:
        o = reference(names, chrom, start, end)
        chrom, start, end, score = chrom[o], start[o], end[o], score[o]
    want = reference(names, chrom, start, end)
    src = [chrom.astype(np.int32), start.astype(np.int64), end.astype(np.int64), score]
    cols = [torch.as_tensor(c).to("cuda:0") for c in src]
    exp = [want] + [c[want] for c in src]
    dts = [torch.int64, torch.int32, torch.int64, torch.int64, torch.float64]
    for mask in range(32):
        outs = [torch.full((n,), -7, dtype=dt, device="cuda:0") if mask >> q & 1 else None for q, dt in enumerate(dts)]
        assert raw_sort(eng, names, cols, BED5, outs) == 0, mask
        for o, w in zip(outs, exp):
            if o is not None:
                assert np.array_equal(o.cpu().numpy(), w), mask


# ------------------------------------------------------------------ T7. allocation balance
@pytest.mark.parametrize("plan", ["packed", "two-round"])
def test_allocation_balance_and_injected_failures(eng, plan):
    from bedops_amd import BedgpuError
    if plan == "packed":
        names, chrom, start, end, score = tied_rows(2 * CHUNK + 9, seed=4)
        device = True
    else:
        names, chrom, start, end = width_rows(17, COORD_MAX, (1 << 20) - 1, n=2 * CHUNK + 9)
        score, device = np.arange(len(chrom), dtype=np.float64), False  # (host arrays: the staging blocks too)
    base = eng.live()
    check(eng, names, chrom, start, end, score, device=device)
    assert eng.live() == base
    failed = 0
    for k in range(1, 200):
        eng.fail_alloc_after(k)
        try:
            check(eng, names, chrom, start, end, score, device=device)
        except BedgpuError as e:
            assert e.code == NOMEM and "injected" in str(e), (k, str(e))
            assert eng.live() == base, k
            failed += 1
            continue
        finally:
            eng.fail_alloc_after(0)
        assert eng.live() == base
        break
    else:
        pytest.fail("no success within 200 allocations")
    # the rank table, the status, key and payload, and each digit round's three blocks at least
    assert failed >= (7 if plan == "packed" else 10)
    check(eng, names, chrom, start, end, score, device=device)
    assert eng.live() == base
