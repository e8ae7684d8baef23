"""tests/decimal_cases.py on the CPU: its references against glibc, and the populations its
generators must hold for tests/test_gpu_decimal_roundtrip.py to mean something.

References: CPython's "%.*f" / "%.*e" and float() are what the GPU tests compare the device
with; here they are compared with glibc snprintf and strtod, which the reference program
prints and reads scores with (Formats.hpp:42-50, Bed.hpp:829-860), on every generated value
and spelling. Populations: conditions on the generators (ties of both parities, values on both
sides of every path limit, carries, tile-edge straddles), counted with exact arithmetic."""
import collections
import ctypes
import math
from fractions import Fraction

import pytest

import decimal_cases as dc

LIBC = ctypes.CDLL("libc.so.6")
LIBC.snprintf.restype = ctypes.c_int
LIBC.strtod.restype = ctypes.c_double
LIBC.strtod.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]


@pytest.fixture(scope="module")
def values():
    return dc.format_values()


@pytest.fixture(scope="module")
def spellings():
    return dc.score_spellings()


def test_format_reference_is_glibc_snprintf(values):
    buf = ctypes.create_string_buffer(1024)
    diffs = n = 0
    for p in list(dc.PRECS) + [18, 25, 60]:
        for sci, fmt in ((False, b"%.*f"), (True, b"%.*e")):
            for v, _ in values:
                k = LIBC.snprintf(buf, 1024, fmt, ctypes.c_int(p), ctypes.c_double(v))
                assert 0 < k < 1024
                n += 1
                if buf.value.decode() != dc.fmt_ref(v, p, sci):
                    diffs += 1
                    print(float.hex(v), p, sci, buf.value, dc.fmt_ref(v, p, sci))
    print(f"{n} formats, {diffs} differences")
    assert diffs == 0


def test_parse_reference_is_glibc_strtod(spellings):
    diffs = n = 0
    for s, cls in spellings:
        if cls == "refused":
            continue
        text, end = ctypes.create_string_buffer(s.encode()), ctypes.c_void_p()
        got = LIBC.strtod(ctypes.addressof(text), ctypes.byref(end))
        n += 1
        if dc.bits(got) != dc.bits(float(s)) or end.value - ctypes.addressof(text) != len(s):  # (all of it read)
            diffs += 1
            print(s, cls, float.hex(got), float.hex(float(s)))
    print(f"{n} parses, {diffs} differences")
    assert diffs == 0


def test_values_are_finite_signed_and_of_every_class(values):
    assert all(math.isfinite(v) for v, _ in values)
    have = {(dc.bits(v), c) for v, c in values}
    assert all((dc.bits(-v), c) in have for v, c in values)  # both signs, -0.0 included
    assert (dc.bits(-0.0), "tiny") in have
    n = collections.Counter(c for _, c in values)
    assert set(n) == {"pow10", "nines", "tie", "lim64", "tiny", "random"}
    assert n["random"] == 2 * 4000


@pytest.mark.parametrize("p", dc.PRECS)
def test_ties_of_both_parities(values, p):
    """exact ties at p: |v| * 10^p ends in exactly 1/2; >= 8 magnitudes whose kept digit is even
    (the tie rounds down) and >= 8 whose kept digit is odd (it rounds up)"""
    kept = {0: set(), 1: set()}
    for v, _ in values:
        x = Fraction(abs(v)) * 10 ** p
        if x.denominator == 2:
            kept[(x.numerator // 2) & 1].add(abs(v))
    assert len(kept[0]) >= 8 and len(kept[1]) >= 8, (len(kept[0]), len(kept[1]))


@pytest.mark.parametrize("p", dc.PRECS)
def test_both_sides_of_the_fixed_digits_limit(values, p):
    """of the lim64 values made for p (2^64 / 10^p and two doubles on each side), >= 4 signed
    values that fixed_digits takes and >= 4 it refuses (the exact walk)"""
    near = {v for v in dc._around(Fraction(2 ** 64, 10 ** p), 2)}
    n = collections.Counter(dc.route(v, p, False) for v, c in values if c == "lim64" and abs(v) in near)
    assert n["fixed_digits"] >= 4 and n["exact"] >= 4, n
    # the source's test, restated once more without its shifts: |v| * 10^p truncated < 2^64
    for v, _ in values:
        inside = int(Fraction(abs(v)) * 10 ** p) < 2 ** 64
        assert (dc.route(v, p, False) == "fixed_digits") == inside, float.hex(v)


def _carries(v, p):
    """fixed notation prints |v| with one more integer digit than |v| has"""
    return len(dc.fmt_ref(abs(v), p, False).split(".")[0]) > len(str(int(abs(v))))


def _carrying_doubles(p, k, most=4):
    """the doubles in [10^k - 0.5 * 10^-p, 10^k), from the top, `most` at the most"""
    out, v = [], math.nextafter(10.0 ** k, 0.0)
    while len(out) < most and Fraction(v) >= Fraction(10) ** k - Fraction(1, 2 * 10 ** p):
        if _carries(v, p):  # (all but an exact tie that rounds down)
            out.append(v)
        v = math.nextafter(v, 0.0)
    return out


@pytest.mark.parametrize("p", dc.PRECS)
def test_carries_into_a_new_integer_digit(values, p):
    """>= 4 signed values whose rounding adds an integer digit (9.99.. -> 10.00..), for every p
    at which four exist. A double below 10^k (k >= 1) that rounds up to it lies within
    0.5 * 10^-p of it, and the doubles below 10 are 2^-49 = 1.8e-15 apart (further below 100,
    1000, ..): p <= 13 has many, p = 14 exactly two magnitudes (10 - 2^-49 and 10 - 2^-48, four
    signed values), p >= 15 none. Where fewer than four exist the generator holds all of them."""
    got = {v for v, _ in values if _carries(v, p)}
    exist = {v for k in range(1, 23) for v in _carrying_doubles(p, k)}
    if 2 * len(exist) >= 4:
        assert len(got) >= 4
        assert p <= 14
    else:
        assert p >= 15 and not exist and not got
    # (the carry out of the fraction that no digit count shows, 0.99.. -> 1.00.., for p <= 15)
    ones = [v for v, _ in values if abs(v) < 1 and dc.fmt_ref(abs(v), p, False)[0] == "1"]
    assert len(ones) >= 4 or p >= 16


@pytest.mark.parametrize("p", dc.PRECS)
def test_sci_roundings_that_raise_the_exponent(values, p):
    """>= 4 signed values that print with a higher exponent than they have, for every p at
    which four exist. Such a value lies below 10^k by at most 0.5 * 10^(-1-p) of it, and
    doubles are at least 2^-53 = 1.1e-16 of their value apart: from p = 15 on only the largest
    double below 10^k can do it, for the few k where it happens to lie that close. Where fewer
    than four exist the generator holds all of them."""
    up = {v for v, _ in values
          if v and int(dc.fmt_ref(v, p, True).split("e")[1]) > dc.exact_log10(v)}
    if p < 15:
        assert len(up) >= 4
    else:
        exist = {s * v for k in range(-320, 309) for v in [dc.below_pow10(k)] if dc.sci_raises(v, k, p)
                 for s in (1, -1)}
        print(p, len(exist), "doubles in range raise the exponent")
        assert exist <= up and (len(up) >= 4 or up == exist)
    # and on both sides of sci_digits' two limits
    below, above = math.nextafter(1e-16, 0.0), math.nextafter(2.0 ** 128, 0.0)
    have = {v for v, _ in values}
    assert {below, 1e-16, above, 2.0 ** 128} <= have
    assert dc.route(below, p, True) == "exact" and dc.route(2.0 ** 128, p, True) == "exact"
    assert dc.route(above, p, True) == "sci_digits"
    assert dc.route(1e-16, p, True) == ("sci_digits" if p <= 6 else "exact")  # (m * 10^(p+16) < 2^128)
    n = collections.Counter(dc.route(v, p, True) for v, _ in values)
    assert n["sci_digits"] >= 1000 and n["exact"] >= 1000


def test_spelling_classes(spellings):
    n = collections.Counter(c for _, c in spellings)
    assert set(n) == {"int", "dec", "clinger", "exact128", "big", "refused"}
    assert all(n[c] >= 50 for c in n if c != "refused"), n
    for s, c in spellings:
        assert (dc.score_route(s, True) == "refused") == (c == "refused"), s
    # what each class is for, by the loader's own routing (score_route)
    wide = collections.Counter((c, dc.score_route(s, True)) for s, c in spellings)
    normal = collections.Counter((c, dc.score_route(s, False)) for s, c in spellings)
    assert wide["exact128", "exact128"] >= 50 and wide["int", "exact128"] >= 40 and wide["dec", "exact128"] >= 20
    assert normal["exact128", "exact128"] == 0 and normal["exact128", "big"] >= 50
    assert wide["big", "big"] == n["big"] and wide["clinger", "clinger"] >= 50
    assert wide["clinger", "exact128"] >= 20 and wide["clinger", "big"] >= 20  # 10^23..37, inexact
    # first past the 128-bit path on each side
    pws = {dc.significand(s)[1] for s, c in spellings if c == "exact128"}
    assert pws >= set(range(-27, 29))
    # 19 digits next to a midpoint, and 20: the first the fast decimal parser refuses
    sig = collections.Counter((c, dc.significand(s)[2]) for s, c in spellings if c != "refused")
    assert sig["dec", 19] >= 8 and sig["dec", 20] >= 8 and sig["exact128", 19] >= 100
    assert max(k for (c, k) in sig) == 200


def test_score_file_layout():
    pairs, text, offs = dc.score_table()
    lines = text.decode().splitlines()
    assert len(lines) == len(pairs) == len(offs)
    for i, ((s, _), o, ln) in enumerate(zip(pairs, offs, lines)):
        f = ln.split("\t")
        assert f[0] == dc.CHROM and int(f[1]) == 10 * i and f[4] == s and len(f) == (6 if i % 4 == 3 else 5)
        assert text[o:o + len(s)].decode() == s and len(f[3]) == 1 + i % 9
    assert {o % 4 for o in offs} == {0, 1, 2, 3}
    for cls in ("int", "dec"):
        for edge in (dc.TW, dc.TT):
            across = [s for (s, c), o in zip(pairs, offs) if c == cls and o // edge != (o + len(s) - 1) // edge]
            assert across, (cls, edge)
    short = dc.short_lines()
    assert all(len(ln) == 6 for ln in short.splitlines(keepends=True))
    assert short.count(b"\n") > dc.TW // 8  # more lines than a sub-tile of the row parser holds
