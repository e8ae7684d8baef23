"""The two hand-written decimal conversions on the device against exact references
(tests/decimal_cases.py; tests/test_decimal_cases.py holds the references against glibc):

  formatter  bg_format.hip's fixed_digits / sci_digits / div_pow10 / put_fixed / put_sci, the
             small and the general bedmap kernel (RES_MAPS / RES_MAP), and bg_decfmt.h's
             put_real_exact as compiled for the device: every value of format_values() printed
             at every precision 0..17, fixed and --sci, byte for byte "%.*f" / "%.*e"
  loader     bg_load.hip's parse_score<false> + parse_score_fast_ws + k_score_big (the normal
             route, k_parse_rv) and parse_score<true> with decimal_exact / round_u128 +
             parse_score_fast (the wide route, k_parse, which a load takes only when it is
             redone for short lines): every spelling of score_spellings() bit for bit float(s)

Every reference row [10i, 10i+5) holds exactly one map row, so --min, --max and --median print
the score itself. Kernel names are those of the BG_LAUNCH sites (tests/kernel_paths.py):
k_parse = k_parse_rv, k_parse_wide = k_parse."""
import collections

import numpy as np
import pytest
import torch

import decimal_cases as dc
import kernel_paths

pytestmark = pytest.mark.gpu

# torch's HIP runtime has to start before libbedgpu's opens the device (INTEGRATION.md §4.1,
# as in tests/test_gpu_columns.py): load_columns and InputSet.columns go through torch
if torch.cuda.is_available():
    torch.cuda.init()

SLOW_CLASSES = ("pow10", "lim64", "tiny")
SLOW_PRECS = (18, 19, 25, 60, 330)


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
def values():
    return dc.format_values()


def _load_values(eng, vals):
    """reference rows [10i, 10i+5) (BED3) and the same rows with the scores (BED5)"""
    from bedops_amd.engine import BED3, BED5
    n = len(vals)
    chrom = np.zeros(n, dtype=np.int32)
    start = np.arange(n, dtype=np.int64) * 10
    score = np.array([v for v, _ in vals], dtype=np.float64)
    return eng.load_columns([(["chr1"], chrom, start, start + 5, BED3),
                             (["chr1"], chrom, start, start + 5, score, BED5)])


def _check(eng, s, vals, ops, p, sci):
    r = eng.map_op(s, ops, precision=p, sci=sci)
    try:
        got = r.text().decode().split("\n")
    finally:
        r.free()
    assert got[-1] == "" and len(got) == len(vals) + 1, (len(got), ops, p, sci)
    for (v, cls), line in zip(vals, got):
        want = dc.fmt_ref(v, p, sci)
        if line != "|".join([want] * len(ops)):
            pytest.fail(f"{float.hex(v)} ({cls}) at p={p} {'--sci' if sci else 'fixed'} {ops}: "
                        f"printed {line!r}, glibc prints {want!r} (route {dc.route(v, p, sci)})")


def test_every_value_at_every_fast_precision(eng, values):
    """p = 0..17: ["min"] runs the small kernel (RES_MAPS; the lim64 values make it hand the
    whole result to the general one), ["max", "median"] the general kernel, ["min"] --sci
    sci_digits: 54 results from one loaded set"""
    base = eng.live()
    s = _load_values(eng, values)
    try:
        for p in dc.PRECS:
            _check(eng, s, values, ["min"], p, False)
            _check(eng, s, values, ["max", "median"], p, False)
            _check(eng, s, values, ["min"], p, True)
    finally:
        s.free()
    assert eng.live() == base


def test_small_kernel_alone_and_its_fallback(eng, values):
    """without a value fixed_digits refuses the small kernel's text stands: it must print what
    the general kernel prints; one refused value and the result is redone by the general one"""
    p = 6
    small = [(v, c) for v, c in values if c in ("tie", "nines", "tiny") and dc.route(v, p, False) == "fixed_digits"]
    assert len(small) > 1000
    base = eng.live()
    for vals, general in ((small, False), (small[:600] + [(2.0 ** 64, "lim64")] + small[600:], True)):
        s = _load_values(eng, vals)
        try:
            def run():
                _check(eng, s, vals, ["min"], p, False)
            _, k = kernel_paths.launches(eng, run)
            print(k)
            # (the count pass runs once per kernel kind tried, the write pass once)
            assert k.get("k_fmt_count", 0) == (2 if general else 1) and k.get("k_fmt_write", 0) == 1, k
        finally:
            s.free()
    assert eng.live() == base


def test_exact_walk_on_the_device_at_long_precisions(eng, values):
    """p = 18, 19, 25, 60, 330 on the classes around the paths' limits: put_real_exact as the
    device compiles it, and rows long enough for the formatter's oversized-tile path"""
    vals = [(v, c) for v, c in values if c in SLOW_CLASSES]
    base = eng.live()
    s = _load_values(eng, vals)
    try:
        for p in SLOW_PRECS:
            for sci in (False, True):
                _check(eng, s, vals, ["min"], p, sci)
        _check(eng, s, vals, ["max", "median"], 25, False)
    finally:
        s.free()
    assert eng.live() == base


def test_text_route_echo_map_score(eng, values):
    """scores read from BED5 text spelled repr(v) and printed by --echo-map-score, and the map
    row itself by --echo-map ("%lf": six digits whatever --prec says) and --min-element (the
    score at --prec)"""
    step = max(1, len(values) // 400)
    vals = [(v, c) for v, c in values[::step]] + [(v, c) for v, c in values if c == "lim64"][:40]
    ref = "".join("chr1\t%d\t%d\n" % (10 * i, 10 * i + 5) for i in range(len(vals))).encode()
    mp = "".join("chr1\t%d\t%d\tid%d\t%r\n" % (10 * i, 10 * i + 5, i, v) for i, (v, _) in enumerate(vals)).encode()
    base = eng.live()
    for p in (0, 6, 17, 25):
        for sci in (False, True):
            got = eng.bedmap(["echo-map-score"], ref, mp, precision=p, sci=sci).decode().split("\n")
            assert len(got) == len(vals) + 1
            for (v, cls), line in zip(vals, got):
                v = float(repr(v))
                assert line == dc.fmt_ref(v, p, sci), (float.hex(v), cls, p, sci)
            got = eng.bedmap(["min-element", "echo-map"], ref, mp, precision=p, sci=sci).decode().split("\n")
            for i, ((v, cls), line) in enumerate(zip(vals, got)):
                row = "chr1\t%d\t%d\tid%d\t" % (10 * i, 10 * i + 5, i)
                want = row + dc.fmt_ref(v, p, sci) + "|" + row + dc.fmt_ref(v, 6, False)
                assert line == want, (float.hex(v), cls, p, sci)
    assert eng.live() == base


# ------------------------------------------------------------------------------- loader
def _scores(eng, inputs, table):
    """(score bit patterns of `table`, {kernel: launches}) of one load"""
    def run():
        s = eng.load(inputs)
        try:
            return s.columns(table)["score"].cpu().numpy().view(np.int64).copy()
        finally:
            s.free()
    return kernel_paths.launches(eng, run)


def _compare(pairs, got, route):
    assert len(got) == len(pairs)
    bad = [(s, cls, g) for (s, cls), g in zip(pairs, got.tolist()) if g != dc.bits(float(s))]
    if bad:
        s, cls, g = bad[0]
        have = float.hex(np.array([g], dtype=np.int64).view(np.float64)[0])
        pytest.fail(f"{s!r} ({cls}, {route} route: {dc.score_route(s, route == 'wide')}): loaded as {have}, "
                    f"strtod gives {float.hex(float(s))}; {len(bad)} differ in all, by class "
                    f"{dict(collections.Counter(c for _, c, _ in bad))}")


@pytest.fixture(scope="module")
def table():
    return dc.score_table()


def test_loader_wide_route(eng, table):
    """the load redone with the wide parser (k_parse: parse_score<true>, decimal_exact,
    round_u128, parse_score_fast) after short lines in another input; bit-exact scores, and the
    same as the normal route's"""
    from bedops_amd.engine import BED3, BED5
    pairs, text, _ = table
    base = eng.live()
    got, k = _scores(eng, [(dc.short_lines(), BED3), (text, BED5)], 1)
    print(k)
    assert k.get("k_parse", 0) == 2 and k.get("k_parse_wide", 0) == 2, k
    assert list(k).index("k_parse") < list(k).index("k_parse_wide")
    _compare(pairs, got, "wide")
    normal, k = _scores(eng, [(text, BED5)], 0)
    assert "k_parse_wide" not in k
    assert (got == normal).all()
    assert eng.live() == base


def test_loader_normal_route(eng, table):
    from bedops_amd.engine import BED5
    pairs, text, _ = table
    base = eng.live()
    got, k = _scores(eng, [(text, BED5)], 0)
    print(k)
    assert k.get("k_parse", 0) == 1 and "k_parse_wide" not in k and k.get("k_score_big", 0) == 1, k
    _compare(pairs, got, "normal")
    assert eng.live() == base


def test_fast_spellings_launch_no_exact_conversion(eng):
    """int and dec spellings of at most 19 digits. The wide parser converts every one itself
    (decimal_exact where the significand passes 2^53). The row parser k_parse_rv is built
    without the 128-bit arithmetic (parse_score<false>), so there a significand above 2^53 is
    one for k_score_big, by design (bg_load.hip, parse_score's comment): with those left out it
    launches none either, with them exactly one."""
    from bedops_amd.engine import BED3, BED5
    short = lambda s, c: c in ("int", "dec") and dc.significand(s)[2] <= 19
    exact = lambda s, c: short(s, c) and dc.significand(s)[0] <= 2 ** 53
    base = eng.live()
    for keep, route, big in ((short, "wide", 0), (exact, "normal", 0), (short, "normal", 1)):
        pairs, text, _ = dc.score_table(keep)
        assert len(pairs) > 500
        inputs = [(dc.short_lines(), BED3), (text, BED5)] if route == "wide" else [(text, BED5)]
        got, k = _scores(eng, inputs, len(inputs) - 1)
        print(route, k)
        assert k.get("k_score_big", 0) == big, (route, k)
        assert ("k_parse_wide" in k) == (route == "wide")
        _compare(pairs, got, route)
    assert eng.live() == base


@pytest.mark.parametrize("route", ["normal", "wide"])
def test_refused_spellings(eng, route):
    from bedops_amd import BedgpuError
    from bedops_amd.engine import BED3, BED5
    ok = [s for s, c in dc.score_spellings() if c in ("int", "dec")][:400]
    bad = [s for s, c in dc.score_spellings() if c == "refused"]
    assert len(bad) == 6
    base = eng.live()
    for b in bad:
        text, _ = dc.score_file(ok[:200] + [b] + ok[200:])
        inputs = [(dc.short_lines(), BED3), (text, BED5)] if route == "wide" else [(text, BED5)]
        with pytest.raises(BedgpuError):
            eng.load(inputs).free()
        assert eng.live() == base, b
