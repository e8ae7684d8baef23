"""Every numeric bedmap operation as a column (bg_result_export_map_values, Result.values):
per reference row the double the formatter prints, NaN where it prints NAN.

Oracles (never the call under test): what the reference printed (tests/golden/ref_*.json.gz);
an independent numpy model (map_values_model.model: all-pairs members for --bp-ovr, then the
reference's rules in float64), compared with ==; and, for the criteria the model does not cover,
the text route those fixtures pin (Engine.bedmap), compared as text at 12 decimals.

Every export runs with BEDGPU_SEL_SMALL unset, 0 (every row by the wave's radix select) and
1000000 (every row by the counting lanes); the three must agree exactly.

Shapes: rows of 0, 1, 2, 3, SEL_SMALL - 1, SEL_SMALL, SEL_SMALL + 1, 64, 65, 257 and 5,000
members; 1, 63, 64, 65 and 257 reference rows, a long row at a wave's first and last lane and two
in one wave, a chromosome change inside a wave, chromosomes in one table only; 1,500 x 1,500
rows for the criteria and modes."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

import kernel_paths
import map_values_model as M
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

BED3, BED3_REST, BED5, BED5_REST = 0, 1, 2, 4
ARG, NOMEM, UNSUPPORTED = -6, -7, -8
SEL_SMALL = int(re.search(r"#define\s+SEL_SMALL\s+(\d+)",
                          open(os.path.join(ROOT, "bedops_amd", "csrc", "bg_mapstat.hip")).read()).group(1))
TIERS = (None, "0", "1000000")
KNOWN_RESIDUAL = {("bedmap", 160)}  # (tests/test_gpu_ref_fixtures.py)


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


@pytest.fixture(autouse=True)
def _no_tier_left_set():
    yield
    os.environ.pop("BEDGPU_SEL_SMALL", None)


def set_tier(t):
    # (the library reads the hook at every call)
    if t is None:
        os.environ.pop("BEDGPU_SEL_SMALL", None)
    else:
        os.environ["BEDGPU_SEL_SMALL"] = t


def values3(eng, r, nops):
    """the result's values under the three tier settings, as numpy arrays: they must agree
    exactly (NaN in the same places), and the call must leave bg_live as it found it"""
    base = eng.live()
    got = []
    for t in TIERS:
        set_tier(t)
        got.append([None if v is None else v.cpu().numpy() for v in r.values()])
        assert eng.live() == base, t
    set_tier(None)
    for other in got[1:]:
        for q in range(nops):
            assert got[0][q] is not None and got[0][q].dtype == np.float64
            assert np.array_equal(got[0][q], other[q], equal_nan=True), q
    return got[0]


def same(a, b):
    """== element by element, NaN exactly where the other has NaN"""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def crit_kw(crit, val):
    return {"criterion": crit, "overlap_bp": val} if crit == "bp-ovr" else {"criterion": crit, "value": val}


# ------------------------------------------------------------------ 1. what the reference printed
def test_reference_fixtures(eng):
    from bedops_amd.engine import BedgpuError
    ran, per_op, skipped = 0, {op: 0 for op in M.NEW_OPS}, []
    for suite, k, p, texts, cols in M.fixture_cases():
        if (suite, k) in KNOWN_RESIDUAL:
            continue
        single = len(texts) == 1
        s = eng.load([(texts[0].encode(), BED5_REST)] if single else
                     [(texts[0].encode(), BED3), (texts[1].encode(), BED5_REST)])
        try:
            try:
                r = eng.map_op(s, p["ops"], 0, 0 if single else 1, precision=p["prec"], delim=p["delim"],
                               faster=p["faster"], **crit_kw(p["crit"], p["val"]))
            except BedgpuError as e:  # (an argument the GPU path does not take, such as --kth 1)
                skipped.append((suite, k, e.msg))
                continue
            try:
                vals = values3(eng, r, len(p["ops"]))
            finally:
                r.free()
        finally:
            s.free()
        for q, op in enumerate(p["ops"]):
            assert len(vals[q]) == len(cols[q])
            assert M.fmt(op[0], p["prec"], vals[q]) == cols[q], (suite, k, op)
        for op in {o[0] for o in p["ops"]} & set(M.NEW_OPS):
            per_op[op] += 1
        ran += 1
    print("reference fixtures: %d cases; per new operation %s; not expressible %s" % (ran, per_op, skipped))
    assert ran >= 170, (ran, skipped)
    assert all(n >= 10 for n in per_op.values()), per_op


# ------------------------------------------------------------------ 2. segments of every size
def col_input(rows, scores=None):
    names = sorted({r[0] for r in rows}, key=lambda s: s.encode())[::-1]  # not strcmp order
    idx = {nm: k for k, nm in enumerate(names)}
    cols = [torch.tensor([idx[r[0]] for r in rows], dtype=torch.int32),
            torch.tensor([r[1] for r in rows], dtype=torch.int64),
            torch.tensor([r[2] for r in rows], dtype=torch.int64)]
    if scores is not None:
        cols.append(torch.tensor(np.asarray(scores, dtype=np.float64)))
    return (names, *[c.to("cuda:0") for c in cols], BED3 if scores is None else BED5)


def _bits(b):
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def score_of(kind, rng, j):
    if kind == "equal":
        return 7.25
    if kind == "two":
        return 3.0 if rng.random() < 0.5 else -1.5
    if kind == "mixed":  # decimals of both signs, and zeros of both signs
        return rng.choice([0.0, -0.0]) if rng.random() < 0.1 else rng.uniform(-1000.0, 1000.0)
    if kind == "low-byte":  # doubles next to 1.0 that differ in the last byte only
        return _bits(0x3FF0000000000000 + rng.randrange(256))
    if kind == "high-byte":
        return rng.choice([1e-300, 1e300, -1e-300, -1e300])
    return float(rng.randint(-50, 50))  # "ints"


def segment_tables(counts, kind, seed):
    """reference row i (100 bases, 1,000 apart) with counts[i] map rows inside it and no other;
    chrA up to the middle of the first wave, then chrB, the last row on chrZ (no map rows there);
    five map rows on chr0 (no reference rows there)"""
    rng = random.Random(seed)
    n = len(counts)
    cut = min(40, n // 2)
    chrom = lambda i: "chrZ" if (n > 3 and i == n - 1) else ("chrA" if i < cut else "chrB")
    ref = [(chrom(i), 1000 * i, 1000 * i + 100) for i in range(n)]
    mp = [("chr0", 10 * k, 10 * k + 25) for k in range(5)]
    for i, c in enumerate(counts):
        if chrom(i) == "chrZ":
            continue
        for _ in range(c):
            st = 1000 * i + rng.randrange(0, 80)
            mp.append((chrom(i), st, st + rng.randint(1, 20)))
    mp.sort(key=lambda r: (r[0].encode(), r[1], r[2]))
    scores = [score_of(kind, rng, j) for j in range(len(mp))]
    return ref, mp, scores


ORDER_OPS = ["count", "median", ("kth", 0.25), ("kth", 0.05), ("kth", 0.999), ("mad",), ("mad", 1.4826),
             "bases", "bases-uniq", "bases-uniq-f", "echo-ref-size"]
SUM_OPS = ["sum", "mean", "variance", "stdev", "cv"]
CS = [0, 1, 2, 3, SEL_SMALL - 1, SEL_SMALL, SEL_SMALL + 1, 64, 65, 257]


def counts_for(n):
    c = [CS[(7 * i) % len(CS)] for i in range(n)]
    if n >= 64:
        c[0], c[63] = 65, 257      # a long row at a wave's first lane and at its last
    if n >= 257:
        c[64 + 5], c[64 + 9] = 64, 65   # two in one wave
        c[128:192] = [SEL_SMALL + 1 + (i % 3) for i in range(64)]  # a wave of nothing but long rows
        c[256] = 0  # (chrZ)
    if n == 1:
        c[0] = 65
    return c


def check_segments(eng, counts, kind, ops, seed=1):
    ref, mp, scores = segment_tables(counts, kind, seed)
    want = M.model(ops, ref, mp, scores, M.brute_bp(ref, mp, 1))
    assert [len(m) for m in M.brute_bp(ref, mp, 1)][:len(counts) - 1] == counts[:len(counts) - 1]
    s = eng.load_columns([col_input(ref), col_input(mp, scores)])
    try:
        r = eng.map_op(s, ops, 0, 1)
        try:
            got = values3(eng, r, len(ops))
        finally:
            r.free()
    finally:
        s.free()
    for q, op in enumerate(ops):
        assert want[q] is not None
        assert same(got[q], want[q]), (op, kind, np.nonzero(~((got[q] == want[q]) | (np.isnan(got[q]) & np.isnan(want[q]))))[0][:5])


@pytest.mark.parametrize("kind", ["equal", "two", "mixed", "low-byte", "high-byte", "ints"])
def test_scores_of_every_kind(eng, kind):
    check_segments(eng, counts_for(65), kind, ORDER_OPS + (SUM_OPS if kind == "ints" else []), seed=11)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_reference_row_counts(eng, n):
    check_segments(eng, counts_for(n), "mixed", ORDER_OPS, seed=n)
    check_segments(eng, counts_for(n), "ints", ORDER_OPS + SUM_OPS, seed=n + 1)


def test_a_row_of_5000_members(eng):
    # (few operations: at BEDGPU_SEL_SMALL=1000000 one lane counts 5,000 x 5,000 per rank)
    counts = [3, 5000, 2, 0, 70, 5000 - 1, 1, 0]
    check_segments(eng, counts, "mixed", ["count", ("kth", 0.3), ("mad", 1.4826)], seed=5)


def test_kth_and_mad_rules(eng):
    """kth * n integral (up == down: the mean of two elements) and not, n == 1, kth near 1; MAD of
    1 (NAN), 2, 3 members, even and odd, with and without the multiplier"""
    counts = [1, 2, 3, 4, 5, 8, 10, 20, 40, 100, 0, 7]
    ops = ["count", ("kth", 0.05), ("kth", 0.25), ("kth", 0.5), ("kth", 0.1), ("kth", 0.9999999), "median",
           ("mad",), ("mad", 1.4826), ("mad", 3)]
    ref, mp, scores = segment_tables(counts, "ints", 3)
    want = M.model(ops, ref, mp, scores, M.brute_bp(ref, mp, 1))
    assert want[1][0] == want[6][0] and not np.isnan(want[1][0])   # n == 1: the element itself
    assert np.isnan(want[7][0]) and not np.isnan(want[7][1])       # MAD of one member: NAN
    check_segments(eng, counts, "ints", ops, seed=3)
    check_segments(eng, counts, "mixed", ops, seed=4)


# ------------------------------------------------------------------ 3. criteria and modes
def _base():
    rng = random.Random(20261022)
    mk = lambda n, **kw: randbed.rows(rng, n, span=60000, maxlen=200, **kw)
    srt = lambda rows: sorted(rows, key=lambda r: (r[0].encode(), r[1], r[2]))
    m = mk(1500)
    r = srt(mk(1300) + rng.sample(m, 200))  # (rows equal to a map row, for --exact)
    lm4 = mk(1500) + [("chr1", 500, 10500), ("chr10", 20000, 30000), ("chr2", 100, 5100)]
    lm = lm4 + [("chr2", 100, 100100), ("chr2", 30000, 130000), ("chrX", 0, 5000000)]
    lm30 = lm + [("chr10", 3, 600000000)]
    b = {"r": r, "m": m, "zr": mk(1500, zero_frac=0.05), "zm": mk(1500, zero_frac=0.05),
         "lm4": srt(lm4), "lm": srt(lm), "lm30": srt(lm30)}
    sc = {k: [float(rng.randint(0, 999)) for _ in v] for k, v in b.items()}
    return b, sc


B, SC = _base()
CRITS = [("bp-ovr", 1), ("bp-ovr", 50), ("range", 100), ("fraction-ref", 0.5), ("fraction-map", 0.5),
         ("fraction-either", 0.5), ("fraction-both", 0.5), ("fraction-map", 1e-17), ("exact", None)]
CRIT_IDS = [f"{c}-{v}" for c, v in CRITS]
MODE_OPS = ["count", "sum", "mean", "variance", "stdev", "cv", "median", ("kth", 0.3), ("mad", 1.4826),
            "bases", "bases-uniq", "bases-uniq-f", "echo-ref-size", "min", "max", "indicator"]
PREC = 12


def bed3(rows):
    return "".join(f"{c}\t{s}\t{e}\n" for c, s, e in rows).encode()


def bed5(rows, scores):
    return "".join(f"{c}\t{s}\t{e}\tid{i}\t{int(v)}\n" for i, ((c, s, e), v) in enumerate(zip(rows, scores))).encode()


def check_mode(eng, rkey, mkey, crit, val, cols=False, faster=False, kernel=None):
    """mkey None: single-file mode"""
    single = mkey is None
    ref = B[rkey]
    mp, sc = (ref, SC[rkey]) if single else (B[mkey], SC[mkey])
    text = eng.bedmap(MODE_OPS, bed5(ref, sc) if single else bed3(ref), None if single else bed5(mp, sc),
                      precision=PREC, faster=faster, **crit_kw(crit, val))
    toks = [ln.split("|") for ln in text.decode().split("\n")[:-1]]
    assert len(toks) == len(ref)
    assert sum(int(t[0]) for t in toks) > 100  # the case says something
    if cols:
        s = eng.load_columns([col_input(ref, sc)] if single else [col_input(ref), col_input(mp, sc)])
    else:
        s = eng.load([(bed5(ref, sc), BED5_REST)] if single else [(bed3(ref), BED3), (bed5(mp, sc), BED5_REST)])
    try:
        r = eng.map_op(s, MODE_OPS, 0, 0 if single else 1, precision=PREC, faster=faster, **crit_kw(crit, val))
        try:
            got = values3(eng, r, len(MODE_OPS))
            if kernel:
                _, ran = kernel_paths.launches(eng, lambda: r.values(MODE_OPS.index("median")))
                assert ran.get(kernel) == 1 and ran.get("k_seg_select") == 1, ran
        finally:
            r.free()
    finally:
        s.free()
    for q, op in enumerate(MODE_OPS):
        assert M.fmt(op[0] if isinstance(op, tuple) else op, PREC, got[q]) == [t[q] for t in toks], (op, crit)
    if crit == "bp-ovr" and not faster and not any(s_ == e_ for _, s_, e_ in ref + mp):
        want = M.model([o if isinstance(o, tuple) else (o,) for o in MODE_OPS], ref, mp, sc, M.brute_bp(ref, mp, val))
        for q, op in enumerate(MODE_OPS):
            assert same(got[q], want[q]), op
    return got


@pytest.mark.parametrize("cols", [False, True], ids=["text", "columns"])
@pytest.mark.parametrize("crit,val", CRITS, ids=CRIT_IDS)
def test_criteria(eng, crit, val, cols):
    check_mode(eng, "r", "m", crit, val, cols=cols, kernel="k_pairs_flat")


@pytest.mark.parametrize("cols", [False, True], ids=["text", "columns"])
@pytest.mark.parametrize("crit,val", [("bp-ovr", 1), ("range", 100), ("exact", None)], ids=["bp-ovr", "range", "exact"])
def test_single_file_mode(eng, crit, val, cols):
    check_mode(eng, "m", None, crit, val, cols=cols)


@pytest.mark.parametrize("single", [False, True], ids=["two-file", "single-file"])
@pytest.mark.parametrize("crit,val", [("bp-ovr", 1), ("range", 100)], ids=["bp-ovr", "range"])
def test_zero_length_rows(eng, crit, val, single):
    assert any(s == e for _, s, e in B["zr"]) and any(s == e for _, s, e in B["zm"])
    got = check_mode(eng, "zm" if single else "zr", None if single else "zm", crit, val)
    f = got[MODE_OPS.index("bases-uniq-f")]  # a zero-length reference row: whatever 0 / 0 or x / 0 gives
    assert np.isnan(f).any() or np.isinf(f).any()


@pytest.mark.parametrize("crit,val", [("bp-ovr", 1), ("bp-ovr", 30), ("range", 50), ("fraction-both", 0.5),
                                      ("exact", None)], ids=["bp-ovr-1", "bp-ovr-30", "range", "fraction-both", "exact"])
def test_faster(eng, crit, val):
    check_mode(eng, "r", "m", crit, val, faster=True)


@pytest.mark.parametrize("key", ["lm4", "lm", "lm30"])
def test_long_rows_take_the_per_row_fill(eng, key):
    check_mode(eng, "r", key, "bp-ovr", 1, kernel="k_pairs_rows")
    check_mode(eng, "r", key, "range", 100, cols=True, kernel="k_pairs_rows")


# ------------------------------------------------------------------ 4. the contract
def _raw(eng, r, q, ptr):
    eng.sync_torch()
    rc = eng.L.bg_result_export_map_values(eng.ctx, r.h, q, ptr)
    eng.sync()
    return rc


def id_text(rows):
    return "".join(f"{c}\t{s}\t{e}\t{i}\t{i % 17}\n" for i, (c, s, e) in enumerate(rows)).encode()


def test_codes_and_no_launch_on_refusals(eng):
    from bedops_amd.engine import BedgpuError
    n = len(B["r"])
    buf = torch.full((n + 4,), 12345.0, dtype=torch.float64, device="cuda:0")
    ptr = buf.data_ptr() + 16
    s = eng.load([(bed3(B["r"]), BED3_REST), (id_text(B["m"]), BED5_REST)])
    try:
        err = lambda: eng.L.bg_last_error(eng.ctx).decode()
        ivl = eng.op("-m", s, [0, 1])
        rc, ran = kernel_paths.launches(eng, lambda: _raw(eng, ivl, 0, ptr))
        assert rc == ARG and ran == {} and "not a bedmap result" in err()
        ivl.free()
        sk = eng.map_op(s, ["count", "median"], 0, 1, skip_unmapped=True)
        rc, ran = kernel_paths.launches(eng, lambda: _raw(eng, sk, 1, ptr))
        assert rc == ARG and ran == {} and "skip-unmapped" in err()
        sk.free()
        ops = ["count", "stdev", ("tmean", 0.1, 0.1), "wmean", "echo", "echo-map-id", "echo-ref-name",
               "echo-ref-row-id", "median", "max-element", "echo-map-score"]
        r = eng.map_op(s, ops, 0, 1)
        base = eng.live()
        for q in (-1, len(ops)):
            rc, ran = kernel_paths.launches(eng, lambda: _raw(eng, r, q, ptr))
            assert rc == ARG and ran == {} and "no such operation" in err()
        for q in (0, 8):  # misaligned, whichever kernel would run
            rc, ran = kernel_paths.launches(eng, lambda: _raw(eng, r, q, ptr + 8))
            assert rc == ARG and ran == {} and "aligned" in err()
        assert _raw(eng, r, 0, None) == ARG
        for q, word in ((2, "heap"), (3, "heap"), (4, "text"), (5, "text"), (6, "text"), (7, "text"), (9, "text"),
                        (10, "text")):
            rc, ran = kernel_paths.launches(eng, lambda: _raw(eng, r, q, ptr))
            assert rc == UNSUPPORTED and ran == {} and word in err(), (q, err())
        assert eng.live() == base
        assert bool((buf == 12345.0).all())  # nothing was written by any of them
        # bg_result_export_map is as it was: stdev refused there, served here, on the same result
        with pytest.raises(BedgpuError) as ei:
            r.columns(op_index=1)
        assert ei.value.code == UNSUPPORTED
        assert r.columns()["values"][1] is None
        vals = r.values()
        assert [v is not None for v in vals] == [True, True, False, False, False, False, False, False, True, False,
                                                 False]
        assert torch.equal(r.values(0), r.columns(0)["values"])
        assert bool((vals[1][vals[0] > 1] >= 0).all()) and bool(torch.isnan(vals[1][vals[0] <= 1]).all())
        # launches: one for an aggregate; count + fill + select for an order statistic, and the
        # count is this call's temporary; with the caller's count, the fill and the select only
        _, ran = kernel_paths.launches(eng, lambda: r.values(1))
        assert ran == {"k_map_stat": 1}, ran
        _, ran = kernel_paths.launches(eng, lambda: r.values(8))
        assert ran.get("k_pairs_widen") == 1 and ran.get("k_pairs_flat") == 1 and ran.get("k_seg_select") == 1, ran
        assert eng.live() == base
        r.pairs_total()
        held = eng.live()
        assert held[0] == base[0] + 1
        _, ran = kernel_paths.launches(eng, lambda: r.values(8))
        assert ran == {"k_pairs_flat": 1, "k_seg_select": 1}, ran
        assert eng.live() == held
        r.free()
    finally:
        s.free()


def test_values_stay_inside_the_buffer(eng):
    for n in (1, 63, 257):
        ref, mp, scores = segment_tables(counts_for(n), "ints", 9)
        s = eng.load_columns([col_input(ref), col_input(mp, scores)])
        try:
            r = eng.map_op(s, ["median", "stdev", ("mad",)], 0, 1)
            for q in range(3):
                for t in TIERS:
                    set_tier(t)
                    buf = torch.full((n + 4,), 12345.0, dtype=torch.float64, device="cuda:0")
                    assert _raw(eng, r, q, buf.data_ptr() + 16) == 0
                    assert buf[:2].tolist() == [12345.0] * 2 and buf[n + 2:].tolist() == [12345.0] * 2
                    assert torch.equal(buf[2:n + 2].nan_to_num(nan=-1.0), r.values(q).nan_to_num(nan=-1.0))
            r.free()
        finally:
            s.free()


@pytest.mark.parametrize("mkey", ["m", "lm"], ids=["flat", "long-rows"])
def test_format_and_values_do_not_disturb_each_other(eng, mkey):
    ops = ["count", "median", "stdev", ("mad", 1.4826), ("kth", 0.3)]
    load = lambda: eng.load([(bed3(B["r"]), BED3), (bed5(B[mkey], SC[mkey]), BED5_REST)])
    s = load()
    try:
        r = eng.map_op(s, ops, 0, 1)
        t1 = r.text()
        v1 = r.values()
        assert r.text() == t1
        r.free()
        r = eng.map_op(s, ops, 0, 1)
        v2 = r.values()
        assert r.text() == t1
        v3 = r.values()
        r.free()
    finally:
        s.free()
    for a, b, c in zip(v1, v2, v3):
        assert same(a.cpu().numpy(), b.cpu().numpy()) and same(a.cpu().numpy(), c.cpu().numpy())
    toks = [ln.split("|") for ln in t1.decode().split("\n")[:-1]]
    for q, op in enumerate(ops):
        assert M.fmt(op[0] if isinstance(op, tuple) else op, 6, v1[q].cpu().numpy()) == [t[q] for t in toks]


def test_live_balances_and_injected_failures(eng):
    from bedops_amd.engine import BedgpuError
    s = eng.load([(bed3(B["r"]), BED3), (bed5(B["m"], SC["m"]), BED5_REST)])
    try:
        r = eng.map_op(s, ["count", "median"], 0, 1)
        base = eng.live()
        want = r.values(1)
        assert eng.live() == base
        failed = 0
        for n in range(1, 50):
            eng.fail_alloc_after(n)
            try:
                got = r.values(1)
            except BedgpuError as e:
                assert e.code == NOMEM and "injected" in e.msg, n
                eng.fail_alloc_after(0)
                assert eng.live() == base, n
                failed += 1
                continue
            finally:
                eng.fail_alloc_after(0)
            assert eng.live() == base
            assert same(got.cpu().numpy(), want.cpu().numpy())
            break
        else:
            pytest.fail("the injected failure never stopped firing")
        assert failed >= 3  # the offsets, the scan's partial sums, the members' scores
        assert same(r.values(1).cpu().numpy(), want.cpu().numpy())  # a following call succeeds
        r.free()
    finally:
        s.free()
