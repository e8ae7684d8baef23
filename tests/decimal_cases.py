"""Values and score spellings for the two hand-written decimal conversions, with their
references: the formatter's "%.{p}lf" / "%.{p}e" (bedops_amd/csrc/bg_format.hip: fixed_digits,
sci_digits, div_pow10, put_fixed, put_sci, and bg_decfmt.h's exact walk behind them) and the
loader's score parse (bg_load.hip: parse_score, parse_score_fast_ws, parse_score_fast,
k_score_big). Pure Python, fixed seeds, no GPU.

The references are CPython's own conversions, which are correctly rounded: `"%.*f" % (p, v)`,
`"%.*e" % (p, v)` and `float(s)`. tests/test_decimal_cases.py holds them against glibc
snprintf / strtod (what the reference program prints and reads scores with) on every value
and spelling generated here, so the GPU tests can use them without a reference binary."""
import math
import random
import struct
from fractions import Fraction

PRECS = tuple(range(18))  # the formatter's fast paths: p <= 17
TT = 8192  # bg_load.hip: k_parse's tile
TW = 4096  # bg_load.hip: k_parse_rv's sub-tile


def fmt_ref(v, p, sci):
    return ("%.*e" if sci else "%.*f") % (p, v)


def _ulps(v, k):
    """the double k steps above (k < 0: below) the positive double v"""
    for _ in range(abs(k)):
        v = math.nextafter(v, math.inf if k > 0 else 0.0)
    return v


def _around(x, k):
    """the double nearest to the positive Fraction x, and k neighbours on each side"""
    d = float(x)
    return [_ulps(d, j) for j in range(-k, k + 1)]


# mismatches the GPU tests exposed, kept whatever the seeds do: (value, class)
FOUND_VALUES = [
    # 1e9 - 2^-20 under --sci at p = 14: |v| * 10^5 rounds up to exactly 10^14, which sci_digits
    # took for a first digit 1 at its first exponent estimate: "1.00000000000000e+09" where
    # glibc prints "9.99999999999999e+08"
    (float.fromhex("0x1.dcd64fffffff8p+29"), "nines"),
]
# (spelling, class)
FOUND_SPELLINGS = []

NINES_K = (0, 1, 2, 4, 9)  # fixed notation: 9.99.. just under 10^k
NINES_SCI_K = (-5, -1, 0, 1, 2, 7, 15, 20)  # --sci: 9.99..e(k-1) just under 10^k


def below_pow10(k):
    """the largest double below 10^k"""
    d = float(Fraction(10) ** k)
    return d if Fraction(d) < Fraction(10) ** k else math.nextafter(d, 0.0)


def sci_raises(v, k, p):
    """v < 10^k prints as 1.00..e(k) under "%.{p}e": it lies within half a unit of the last digit"""
    return Fraction(10) ** k - Fraction(v) <= Fraction(10) ** (k - 1 - p) / 2


def format_values():
    """[(v, class)]: finite doubles, every magnitude with both signs"""
    rng = random.Random(20240611)
    mags = []

    def add(cls, *vs):
        for v in vs:
            v = abs(float(v))
            assert math.isfinite(v)
            mags.append((v, cls))

    # tie: odd n / 2^j has exactly j fraction digits, the last one a 5: an exact tie at
    # p = j - 1; ten with an even kept digit and ten with an odd one for every j
    for j in range(1, 19):
        want = {0: 10, 1: 10}
        while want[0] or want[1]:
            n = rng.getrandbits(rng.randint(1, min(52, j + 30))) | 1
            v = Fraction(n, 2 ** j)
            kept = int(v * 10 ** (j - 1)) & 1
            if want[kept]:
                want[kept] -= 1
                add("tie", float(v))
    add("tie", 0.5, 1.5, 2.5, 3.5, 1e15 + 0.5, 2.0 ** 52 - 0.5, 2.0 ** 52 - 1.5)
    # pow10: sci_digits' log10 estimate at every decade it serves and past both of its limits
    for k in range(-20, 40):
        d = float("1e%d" % k)
        add("pow10", math.nextafter(d, 0.0), d, math.nextafter(d, math.inf))
    add("pow10", *_around(Fraction(2) ** 128, 1))
    # nines: the doubles around 10^k - 0.5 * 10^-p (fixed: a new integer digit) and around
    # 10^k - 0.5 * 10^(k-1-p) (--sci: the exponent goes up)
    for p in PRECS:
        for k in NINES_K:
            add("nines", *_around(Fraction(10) ** k - Fraction(1, 2 * 10 ** p), 4))
        for k in NINES_SCI_K:
            add("nines", *_around(Fraction(10) ** k - Fraction(10) ** (k - 1 - p) / 2, 1))
    for k in range(-320, 309):  # (p >= 15: the few doubles that close under a power of ten)
        v = below_pow10(k)
        if sci_raises(v, k, 15):
            add("nines", v)
    # lim64: |v| * 10^p on either side of 2^64, where fixed_digits refuses
    for p in PRECS:
        add("lim64", *_around(Fraction(2 ** 64, 10 ** p), 2))
    # tiny: |v| * 10^p around 1/2 (the first value that prints a nonzero digit), the
    # formatter's shift limits and the ends of the double range
    for p in PRECS:
        add("tiny", *_around(Fraction(1, 2 * 10 ** p), 1))
    add("tiny", 2.0 ** -75, 2.0 ** -110, 2.0 ** -128, 5e-324, 2.2250738585072014e-308,
        1.7976931348623157e308, 0.0, 2.0 ** 53 - 1, 2.0 ** 53 + 2, 2.0 ** 53, 2.0 ** 63, 2.0 ** 64 - 2048)
    # random: any finite bit pattern, and magnitudes where the fast paths work
    n = 0
    while n < 2000:
        v = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(63)))[0]
        if math.isfinite(v):
            add("random", v)
            n += 1
    for _ in range(2000):
        add("random", 10.0 ** rng.uniform(-20.0, 25.0))
    for v, cls in FOUND_VALUES:
        add(cls, v)
    out, seen = [], set()
    for v, cls in mags:
        if (v, cls) in seen:
            continue
        seen.add((v, cls))
        out += [(v, cls), (-v, cls)]
    return out


def _split(v):
    """|v| = m * 2^ex as fixed_digits / sci_digits split it"""
    bits = struct.unpack("<Q", struct.pack("<d", abs(v)))[0]
    bexp, m = bits >> 52, bits & ((1 << 52) - 1)
    if bexp == 0:
        return m, -1074
    return m | (1 << 52), bexp - 1075


def exact_log10(v):
    """floor(log10(|v|)) of a nonzero double, exactly"""
    x = Fraction(abs(v))
    e = len(str(x.numerator)) - len(str(x.denominator))
    while Fraction(10) ** e > x:
        e -= 1
    while Fraction(10) ** (e + 1) <= x:
        e += 1
    return e


def route(v, p, sci):
    """the device path bg_format.hip's put_real sends finite v to, restated in exact
    arithmetic: "fixed_digits", "sci_digits" or "exact" (bg_decfmt.h's put_real_exact)"""
    if p > 17:
        return "exact"
    m, ex = _split(v)
    if not sci:  # fixed_digits
        X = m * 10 ** p
        if ex >= 0:
            return "fixed_digits" if ex < 64 and (X << ex) < 2 ** 64 else "exact"
        if -ex >= 128:
            return "fixed_digits"
        return "fixed_digits" if (X >> -ex) < 2 ** 64 else "exact"
    # sci_digits, at the exponent its correction steps end on
    if m == 0:
        return "sci_digits"
    if abs(v) < 1e-16:
        return "exact"
    E = exact_log10(v)
    if round_half_even(Fraction(abs(v)) * Fraction(10) ** (p - E)) >= 10 ** (p + 1):
        E += 1
    sc = p - E
    num, den = m, 1
    if sc >= 0:
        for _ in range(sc):
            if num > (2 ** 128 - 1) // 10:
                return "exact"
            num *= 10
    else:
        if -sc > 38:
            return "exact"
        den = 10 ** -sc
    if ex >= 0:
        if num << ex >= 2 ** 128:
            return "exact"
    else:
        if -ex >= 128 or (den >> (127 + ex)) != 0:
            return "exact"
    return "sci_digits"


def round_half_even(x):
    q, r = divmod(x.numerator, x.denominator)
    if 2 * r > x.denominator or (2 * r == x.denominator and (q & 1)):
        q += 1
    return q


# ------------------------------------------------------------------------------ spellings
def significand(s):
    """(m, pw, sig): the spelling's value as m * 10^pw the way parse_score trims it (leading
    zeros dropped, trailing zeros only while pw < 0) and its significant digits as written;
    None for what is not [+-]digits[.digits][e[+-]digits]"""
    import re
    g = re.fullmatch(r"[+-]?(\d*)(?:\.(\d*))?(?:[eE]([+-]?\d+))?", s)
    if not g or not (g.group(1) or g.group(2)):
        return None
    ip, fp, ex = g.group(1) or "", g.group(2) or "", int(g.group(3) or 0)
    digits = (ip + fp).lstrip("0")
    m, pw = int(digits or "0"), ex - len(fp)
    while pw < 0 and m and m % 10 == 0:
        m //= 10
        pw += 1
    return m, pw, len(digits)


def score_route(s, wide):
    """which conversion of bg_load.hip the spelling's value comes from, on the normal route
    (k_parse_rv, parse_score<false>) or the wide one (k_parse, parse_score<true>): "clinger"
    (one rounding of exact operands, the fast parsers included), "exact128" (decimal_exact),
    "big" (k_score_big) or "refused" """
    t = significand(s)
    if t is None:
        return "refused"
    m, pw, sig = t
    if sig > 200:
        return "refused"
    if sig > 19:
        return "big"
    if m == 0:
        return "clinger"
    if m <= 2 ** 53 and -22 <= pw <= 22:
        return "clinger"
    if m <= 2 ** 53 and 22 < pw and m * 10 ** (pw - 22) <= 2 ** 53:
        return "clinger"
    if wide and -26 <= pw <= 27:
        return "exact128"
    return "big"


def _digits(rng, n, first_nonzero=True):
    s = "".join(rng.choice("0123456789") for _ in range(n))
    if first_nonzero and s[0] == "0":
        s = rng.choice("123456789") + s[1:]
    return s


def _plain(n, f):
    """n / 10^f (n > 0) written without an exponent"""
    s = str(n)
    if f <= 0:
        return s + "0" * -f
    s = s.rjust(f + 1, "0")
    return s[:-f] + "." + s[-f:]


def _midpoint(a):
    """the exact midpoint of the positive double a and the next one, as (n, f): n / 10^f with
    n not a multiple of 10 unless f <= 0"""
    x = (Fraction(a) + Fraction(math.nextafter(a, math.inf))) / 2
    den, f = x.denominator, 0
    while den % 2 == 0:  # the denominator is a power of two
        den //= 2
        f += 1
    n = x.numerator * 5 ** f
    assert den == 1
    while f > 0 and n % 10 == 0:
        n //= 10
        f -= 1
    return n, f


def score_spellings():
    """[(spelling, class)]; float(spelling) is the reference for every class but "refused" """
    rng = random.Random(777001)
    out = []

    def add(cls, *ss):
        for s in ss:
            out.append((s, cls))

    # ---- int
    for nd in range(1, 13):
        add("int", "1" + "0" * (nd - 1), "9" * nd, *[_digits(rng, nd) for _ in range(6)])
    for nd in range(13, 20):
        add("int", "1" + "0" * (nd - 1), "9" * nd, *[_digits(rng, nd) for _ in range(4)])
    add("int", str(2 ** 53 - 1), str(2 ** 53), str(2 ** 53 + 1), str(2 ** 53 + 2), str(2 ** 53 + 3))
    for b in range(54, 64):  # exact ties of 17..19 digits: halfway between two doubles of [2^b, 2^(b+1))
        got = {0: 0, 1: 0}
        while got[0] < 2 or got[1] < 2:
            k = rng.randrange(2 ** 52, 2 ** 53)
            n = (2 * k + 1) << (b - 53)
            if n < 10 ** 19 and got[k & 1] < 2:
                got[k & 1] += 1
                add("int", str(n))
    add("int", "007", "0000000000123", "00000000000000000000042", "000", "0", "+5", "-5", "+123456789012",
        "-123456789012", "-9007199254740993", "+18014398509481985", "-0", "0.0", "-0.000", "5.", ".5",
        "-5.", "+.5")
    # ---- dec
    for ni in range(1, 13):
        for nf in range(1, 13):
            add("dec", *[_digits(rng, ni) + "." + _digits(rng, nf, False) for _ in range(6)])
    for ni, nf in ((7, 12), (12, 7), (10, 9), (9, 10), (8, 12), (12, 8), (10, 10), (11, 9)):  # 19 and 20 digits
        add("dec", *[_digits(rng, ni) + "." + _digits(rng, nf, False) for _ in range(4)])
    add("dec", "1.500", "12.000", "0.1000000", "0.000", "10.0001", "007.25", "123456.7890000", "0.000001",
        "9007199254.740991", "9007199254.7409920", "900719925474.0992", "90071992547.409930",
        "9007199254.740993", "900719925474.0993", "9007199254.7409930", "9.007199254740994",
        "-1.5", "+2.25", "-0.1", "-123456789012.123456")
    # ---- clinger: m <= 2^53 times a power of ten at and just past the exact powers
    for pw in (-22, -23, 22):
        for _ in range(40):
            add("clinger", "%de%d" % (rng.randrange(1, 2 ** 53) | 1, pw))
        add("clinger", "%de%d" % (2 ** 53, pw), "9007199254740991e%d" % pw)
    for pw in range(23, 38):
        room = 2 ** 53 // 10 ** (pw - 22)
        for _ in range(8):  # m * 10^(pw-22) stays <= 2^53: still one exact rounding
            add("clinger", "%de%d" % (rng.randrange(1, room + 1), pw))
        add("clinger", "%de%d" % (room, pw), "%de%d" % (room + 1, pw))
        for _ in range(8):  # it does not
            add("clinger", "%de%d" % (rng.randrange(room + 1, 2 ** 53) | 1, pw))
    add("clinger", "1e3", "2.5e-2", "1E5", "2.5E+10", "1.25e-22", "7e22", "1e23", "1e37", "3e-23")
    # ---- exact128: 17..19 significant digits times 10^-26..27 (decimal_exact on the wide route)
    for pw in list(range(-26, 28)) + [-27, 28]:
        for _ in range(4):
            v = float("%se%d" % (_digits(rng, 17), pw))
            add("exact128", repr(v), "%.17e" % v)
    for i in range(200):  # next to the midpoint of two doubles, in 19 digits
        # (between 2^47 and 2^63 the midpoint itself has at most 19: an exact tie, and both sides)
        a = 10.0 ** rng.uniform(-7.0, 44.0) if i < 160 else float(rng.randrange(2 ** 47, 2 ** 63))
        n, f = _midpoint(a)
        s = str(n)
        if len(s) <= 19:
            if n > 2 ** 53:
                add("exact128", _plain(n, f), _plain(n + 1, f), _plain(n - 1, f))
            continue
        cut, pw = int(s[:19]), len(s) - 19 - f
        for m in (cut, cut + 1):
            add("exact128", _plain(m, -pw) if -18 <= pw < 0 else "%de%d" % (m, pw))
    # ---- big: past 19 significant digits, or past the 128-bit exponents
    n200 = 0
    while n200 < 80:
        a = math.ldexp(rng.uniform(1.0, 2.0), rng.randint(-150, 150))
        n, f = _midpoint(a)
        if not 20 <= len(str(n)) <= 199:
            continue
        n200 += 1
        add("big", _plain(n, f), _plain(n + 1, f), _plain(n - 1, f))
    add("big", "1" + _digits(rng, 198, False) + "7", "0." + "3" + _digits(rng, 198, False) + "1",
        "9" * 200, "1" + "0" * 198 + "1e-180", "0." + "0" * 60 + "123456789", "0." + "0" * 150 + "7",
        "0." + "0" * 30 + "12345678901234567890123", "1.5e300", "123e-310", "4.9e-324", "1e-320",
        "12345678901234567890e10", "1.2345678901234567890123e-5", "1e38", "1e-27", "123456789012345678e28",
        "1.7976931348623158e308", "1.7976931348623159e308", "2.4703282292062327e-324",
        "2.4703282292062328e-324", "1e309", "1e-400", "-1e309", "-1e-400")
    # ---- refused
    add("refused", "1" * 201, "1e", "1e+", "1.2.3", "0x10", "nan")
    for s, cls in FOUND_SPELLINGS:
        add(cls, s)
    return out


CHROM = "c"  # one byte: the wide route's 6-byte lines ("c\t0\t1\n") sit on the same chromosome


def _head(i):
    return "%s\t%d\t%d\t%s\t" % (CHROM, 10 * i, 10 * i + 5, "abcdefghi"[:1 + i % 9])


def score_file(spellings):
    """(text, offsets): a sorted one-chromosome BED5 text with one line per spelling, in order,
    and the byte offset of each score. Ids run over lengths 1..9 and every fourth line carries
    a further column."""
    parts, offs, pos = [], [], 0
    for i, s in enumerate(spellings):
        head = _head(i)
        line = head + s + ("\tmore\n" if i % 4 == 3 else "\n")
        offs.append(pos + len(head))
        parts.append(line)
        pos += len(line)
    return "".join(parts).encode(), offs


def score_table(keep=None, seed=99):
    """(pairs, text, offsets): the accepted spellings (those keep(spelling, class) picks) in a
    fixed mixed order, so that every class meets every tile position, and their score_file"""
    rest = [(s, c) for s, c in score_spellings() if c != "refused" and (keep is None or keep(s, c))]
    random.Random(seed).shuffle(rest)
    # where a score can lie across a sub-tile edge (a multiple of TW; every second one is a tile
    # edge of the wide parser), the next "int" or "dec" spelling long enough to do so is taken:
    # edges 0, 1 mod 4 get an int, edges 2, 3 a dec
    pairs, pos = [], 0
    while rest:
        start = pos + len(_head(len(pairs)))
        edge = start // TW + 1
        room = edge * TW - start  # a score longer than this crosses the edge
        want = "int" if edge % 4 < 2 else "dec"
        pick = next((k for k, (s, c) in enumerate(rest) if c == want and len(s) > room), 0) if room < 20 else 0
        s, c = rest.pop(pick)
        pairs.append((s, c))
        pos = start + len(s) + (6 if len(pairs) % 4 == 0 else 1)
    text, offs = score_file([s for s, _ in pairs])
    return pairs, text, offs


def short_lines(n=3000):
    """a sorted BED3 table of 6-byte lines on score_file's chromosome: more lines than a 4 KiB
    sub-tile of the row parser holds, so a load that includes it is redone with the wide parser"""
    rows = sorted((i % 9, i % 9 + 1) for i in range(n))
    return "".join("%s\t%d\t%d\n" % (CHROM, a, b) for a, b in rows).encode()


def bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]
