"""Generated --ec inputs that put defects where bg_check's parallel form (bg_check.hip) can go
wrong: on the seams of its 8 KiB tiles, 2 KiB waves and 32-byte threads, behind header blocks
longer than a tile, in files with several defects, at every kind of file end, in very long
fields, past the first level of the tile-count scan and in runs of newlines. Pure Python: the
CPU test (tests/test_ec_cases.py) checks the inputs themselves, the GPU test
(tests/test_gpu_check_tiles.py) runs bg_check on them.

Every family is a list of Case(name, data, nfields, has_rest, nest); META[name] holds what the
generator knows about the case by construction:
  expect   the BGC_* name of the first failure, or None for a file that passes
  row      its 1-based line number (when the generator placed it)
  at       the byte offset of that line's first byte (when the generator placed it)
  defects  family D: [(row, BGC name), ...] of every defect in file order
"""
import os
import re
from typing import NamedTuple

import test_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bedops_amd", "csrc")

# bg_check.hip's and bg_scan.hip's geometry, stated here; test_ec_cases.py greps the sources for
# them (source_constants), so a retune fails there instead of quietly moving the seams
TILE = 8192          # CK_TILE: bytes per workgroup
THREAD_BYTES = 32    # bytes per thread
WAVE_BYTES = 2048    # 64 lanes x 32 bytes
SCAN_TILE = 1024     # entries per workgroup of bg_scan_sum_u64's first level
BASE_BYTES = 5 * TILE


class Case(NamedTuple):
    name: str
    data: bytes
    nfields: int
    has_rest: int
    nest: int


META = {}


def _case(name, data, nf, rest, nest=0, **meta):
    META[name] = meta
    return Case(name, data, nf, rest, nest)


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_constants():
    """(tile, bytes per thread, bytes per wave, scan tile) as the sources define them"""
    ck, scan, internal = _src("bg_check.hip"), _src("bg_scan.hip"), _src("bg_internal.h")
    tile = int(re.search(r"#define CK_TILE (\d+)", ck).group(1))
    per_thread = {int(x) for x in re.findall(r"threadIdx\.x \* (\d+)", ck)}
    assert len(per_thread) == 1, per_thread
    nt = int(re.search(r"#define BG_NT (\d+)", internal).group(1))
    items = int(re.search(r"#define SCAN_ITEMS (\d+)", scan).group(1))
    assert re.search(r"#define SCAN_TILE \(BG_NT \* SCAN_ITEMS\)", scan)
    thread = per_thread.pop()
    assert nt * thread == tile, (nt, thread, tile)  # one workgroup covers its tile exactly
    return tile, thread, 64 * thread, nt * items


def codes():
    """the BGC_* enum of bg_check.h: name -> value"""
    body = re.search(r"enum \{(.*?)\};", _src("bg_check.h"), re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    out, v = {}, -1
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        name, _, val = item.partition("=")
        v = int(val) if val.strip() else v + 1
        out[name.strip()] = v
    return out


# ------------------------------------------------------------------ rows and placement
def row(chrom, start, end, k=0, extra=b"x"):
    """chr, start, end, id, score, strand, rest: a valid row for 3 to 6 checked fields"""
    return b"%s\t%d\t%d\tid%d\t%d.5\t+\t%s" % (chrom, start, end, k, k % 90, extra)


def rows_upto(chrom, nbytes):
    """strictly sorted, non-nested rows on one chromosome: as many as fit into nbytes"""
    out, used, k = [], 0, 0
    while True:
        r = row(chrom, 100 + 10 * k, 105 + 10 * k, k)
        if used + len(r) + 1 > nbytes:
            return out
        out.append(r)
        used += len(r) + 1
        k += 1


def offset_of(lines, i):
    """the byte offset of lines[i]'s first byte (len(lines): the file size with a final newline)"""
    return sum(len(l) + 1 for l in lines[:i])


def first_line_at(lines, off):
    """the index of the first line that starts at or after byte `off`"""
    p = 0
    for i, l in enumerate(lines):
        if p >= off:
            return i
        p += len(l) + 1
    raise ValueError(off)


def place(lines, i, at):
    """Placement helper: grows the last field (the rest) of the row before lines[i] so that
    lines[i]'s first byte lands on byte offset `at`"""
    need = at - offset_of(lines, i)
    assert i > 0 and need >= 0, (i, at, need)
    out = list(lines)
    out[i - 1] = out[i - 1] + b"x" * need
    return out


def join(lines, newline=True):
    return b"\n".join(lines) + (b"\n" if newline and lines else b"")


def base_lines(total=BASE_BYTES, chroms=(b"chr1", b"chr2", b"chr3")):
    """the clean base file: sorted rows over three chromosomes, about `total` bytes"""
    out = []
    for c in chroms:
        out += rows_upto(c, total // len(chroms))
    return out


def embed(mid, focus, at, total=BASE_BYTES):
    """rows on chr0, then the lines `mid` with mid[focus]'s first byte at offset `at`, then rows
    on chr3 and chr4 up to `total` bytes; returns (lines, index of mid[focus])"""
    head = at - offset_of(mid, focus)
    pre = rows_upto(b"chr0", head)
    lines = place(pre + list(mid), len(pre), head)
    left = max(total - offset_of(lines, len(lines)), 0)
    for c in (b"chr3", b"chr4"):
        lines += rows_upto(c, left // 2)
    assert offset_of(lines, len(pre) + focus) == at
    return lines, len(pre) + focus


def case_lines(data):
    ls = data.split(b"\n")
    if ls[-1] == b"":
        ls.pop()
    return ls


def seam(kind, i):
    """a tile boundary, a wave boundary inside a tile or a thread boundary inside a wave; `i`
    walks through tiles 1-4, waves 1-3 and the lanes"""
    k = 1 + i % 4
    if kind == "tile":
        return k * TILE
    if kind == "wave":
        return k * TILE + (1 + i % 3) * WAVE_BYTES
    assert kind == "thread"
    return k * TILE + (i % 4) * WAVE_BYTES + (1 + (7 * i) % 63) * THREAD_BYTES


SEAM_KINDS = ("tile", "wave", "thread")
CLEAN_ROW = row(b"chr1", 5, 10)

# ------------------------------------------------------------------ A: seam x defect class
STRAND6 = [b"chr1\t5\t10\tid\t1\tx\n", b"chr1\t5\t10\tid\t1\t+-\n", b"chr1\t5\t10\tid\t1\t\t+\n",
           b"chr1\t5\t10\tid\t1\n", b"chr1\t5\t10\tid\t1\t\n", b"chr1\t5\t10\tid\t1\t +\n",
           b"chr1\t5\t10\tid\t1\t-\trest\n"]
# measurement defects neither list of test_check has, and the id defects of 4 checked fields
EXTRA5 = [b"chr1\t5\t10\tid\t\t3\n", b"chr1\t5\t10\tid\t1e-\n", b"chr1\t5\t10\tid\t1e-\t+\n"]
FIELDS4 = [b"chr1\t5\t10\t\n", b"chr1\t5\t10\t\tx\n", b"chr1\t5\t10\ti d\n", b"chr1\t5\t10\n",
           b"chr1\t5\t10\tid\n", b"chr1\t5\t10\tid\t\n"]
A_PARAMS = [(3, 0, test_check.CASES), (3, 1, test_check.CASES),
            (5, 1, test_check.CASES5 + test_check.CASES + EXTRA5),
            (6, 1, test_check.CASES5 + STRAND6 + EXTRA5), (4, 1, FIELDS4)]


def family_a(pi, kind):
    """every file of test_check.CASES/CASES5 (and 6-field strand defects) set into the base
    file, once for each of its lines l with that line's first byte at S-1, S and S+1 of a seam:
    whichever line fails under (nfields, has_rest) sits on the seam in one of them. `expect`
    is left to the oracle; `at` is where line l starts. The clean variants carry a valid row
    at the same offsets."""
    nf, rest, cases = A_PARAMS[pi]
    out = []
    for ci, data in enumerate(cases):
        mid = case_lines(data)
        for j in range(len(mid)):
            for d in (-1, 0, 1):
                at = seam(kind, ci + j) + d
                lines, f = embed(mid, j, at)
                out.append(_case(f"A-{nf}{rest}-{kind}{d:+d}-c{ci}l{j}", join(lines), nf, rest,
                                 at=at, row=f + 1))
    for i in range(4):
        for d in (-1, 0, 1):
            lines, _ = embed([CLEAN_ROW], 0, seam(kind, i) + d)
            out.append(_case(f"A-{nf}{rest}-{kind}{d:+d}-clean{i}", join(lines), nf, rest, expect=None))
    return out


# ------------------------------------------------------------------ B: order checks over a seam
B_PARAMS = [(3, 0), (3, 1), (5, 1)]
_PREV = b"chr2\t500\t600\tidP\t1\t+\tm"
# (tag, the row after _PREV, nest, first failure without has_rest, with has_rest)
_B_ROWS = [
    ("chr", b"chr1\t700\t800\tidP\t1\t+\tm", 0, "BGC_UNSORTED_CHR", "BGC_UNSORTED_CHR"),
    ("start", b"chr2\t499\t600\tidP\t1\t+\tm", 0, "BGC_UNSORTED_START", "BGC_UNSORTED_START"),
    ("end", b"chr2\t500\t599\tidP\t1\t+\tm", 0, "BGC_UNSORTED_END", "BGC_UNSORTED_END"),
    ("rest", b"chr2\t500\t600\tidP\t1\t+\tl", 0, None, "BGC_UNSORTED_REST"),
    ("restprefix", b"chr2\t500\t600\tidP\t1\t+", 0, None, "BGC_UNSORTED_REST"),
    ("restgreater", b"chr2\t500\t600\tidP\t1\t+\tn", 0, None, None),
    ("nested", b"chr2\t510\t590\tidP\t1\t+\tm", 1, "BGC_NESTED", "BGC_NESTED"),
    ("nested-off", b"chr2\t510\t590\tidP\t1\t+\tm", 0, None, None),
    ("nested-equal-ends", b"chr2\t510\t600\tidP\t1\t+\tm", 1, None, None),
    ("nested-le", b"chr2\t510\t505\tidP\t1\t+\tm", 1, "BGC_NESTED", "BGC_NESTED"),
    ("nested-unsorted", b"chr2\t500\t590\tidP\t1\t+\tm", 1, "BGC_UNSORTED_END", "BGC_UNSORTED_END"),
    ("le", b"chr2\t700\t700\tidP\t1\t+\tm", 0, "BGC_END_LE_START", "BGC_END_LE_START"),
    ("lt", b"chr2\t700\t650\tidP\t1\t+\tm", 1, "BGC_END_LE_START", "BGC_END_LE_START"),
]


def family_b(pi, long_prev):
    """the previous row ends in tile k-1, the checked row starts in tile k (its first byte at
    k*TILE, or one later, so that the previous newline opens the tile). long_prev: the previous
    row's rest is 20 KiB, so the backward scan crosses two whole tiles that hold no newline
    and whose newline counts are zero."""
    nf, rest = B_PARAMS[pi]
    prev = _PREV + (b"x" * (20 * 1024) if long_prev else b"")
    out = []
    for i, (tag, cur, nest, e0, e1) in enumerate(_B_ROWS):
        for d in (0, 1):
            k = 4 if long_prev else 1 + i % 4
            at = k * TILE + d
            lines, f = embed([prev, cur], 1, at, total=BASE_BYTES + (TILE if long_prev else 0))
            assert offset_of(lines, f - 1) < (k - 2 if long_prev else k) * TILE
            expect = e1 if rest else e0
            out.append(_case(f"B-{nf}{rest}-{'long' if long_prev else 'short'}-{tag}{d:+d}", join(lines),
                             nf, rest, nest, expect=expect, at=at, row=f + 1))
    return out


# ------------------------------------------------------------------ C: headers
_HDRS = [b"#c", b"@h", b"track name=x", b"browser position", b"TRACK", b"Browser\tx", b"#", b"@",
         b"track\ttype=bed", b"BROWSER"]
LATE_HEADERS = [b"#late", b"@late", b"track x", b"browser\ty", b"track", b"BROWSER", b"TrAcK", b"browser"]


def header_block(nbytes):
    out, i = [], 0
    while offset_of(out, len(out)) < nbytes:
        out.append(_HDRS[i % len(_HDRS)])
        i += 1
    return out


def family_c():
    out = []
    blocks = [("short", header_block(TILE + 1500)), ("long", [b"#" + b"h" * (TILE + 300)]),
              ("long2", [b"#" + b"h" * (2 * TILE - 2)])]  # (long2: row F starts a tile)
    for tag, hdr in blocks:
        assert offset_of(hdr, len(hdr)) >= TILE
        body = base_lines(3 * TILE)
        f = len(hdr)  # index of row F, the first line that is no header
        bad_f = [b"chr1\t50\t50\tid\t1\t+\tx"] + body
        bad_f1 = [body[0], row(b"chr1", 90, 200)] + body[1:]
        for nf, rest in ((3, 0), (5, 1)):
            out.append(_case(f"C-{tag}-clean-{nf}{rest}", join(hdr + body), nf, rest, expect=None))
            out.append(_case(f"C-{tag}-F-{nf}{rest}", join(hdr + bad_f), nf, rest,
                             expect="BGC_END_LE_START", row=f + 1, at=offset_of(hdr, f)))
            out.append(_case(f"C-{tag}-F1-{nf}{rest}", join(hdr + bad_f1), nf, rest,
                             expect="BGC_UNSORTED_START", row=f + 2,
                             at=offset_of(hdr + bad_f1, f + 1)))
    for i, h in enumerate(LATE_HEADERS):
        for d in (-1, 0, 1):
            at = seam("tile", i) + d
            lines, f = embed([h], 0, at)
            out.append(_case(f"C-late{i}{d:+d}", join(lines), 3, 1, expect="BGC_HEADER_LATE",
                             row=f + 1, at=at))
    only = header_block(3 * TILE)
    out.append(_case("C-only", join(only), 3, 1, expect=None))
    out.append(_case("C-only-nonl", join(only, newline=False), 5, 1, expect=None))
    out.append(_case("C-only-oneline", b"#" + b"h" * (2 * TILE + 1000), 3, 0, expect=None))
    return out


# ------------------------------------------------------------------ D: first failure wins
def _fields(line):
    f = line.split(b"\t")
    return f[0], int(f[1]), int(f[2])


def _nested_after(line):
    c, s, e = _fields(line)
    return b"%s\t%d\t%d\tidN\t1\t+\tx" % (c, s + 1, e - 2)


def _start_below(line):
    c, s, e = _fields(line)
    return b"%s\t%d\t%d\tidU\t1\t+\tx" % (c, s - 15, e)


def _edit(lines, edits):
    """edits: (offset, kind, payload, BGC name) in file order. kind "ins": payload goes in as a
    new line before the first base line at or after `offset`; "rep": payload(that line) replaces
    it; "after": payload(the line before) goes in as a new line. -> (lines, [(row, name)])"""
    out, defects, shift = list(lines), [], 0
    for off, kind, payload, name in edits:
        i = first_line_at(lines, off) + shift
        if kind == "rep":
            out[i] = payload(out[i])
        else:
            out.insert(i, payload(out[i - 1]) if kind == "after" else payload)
            shift += 1
        defects.append((i + 1, name))
    return out, defects


def family_d():
    """several defects whose file order is the reverse of their code order, in different tiles
    and in different waves and threads of one tile; each also with its first defect left out,
    so that the later ones are seen to be defects. The last pair: a grammar defect on line j
    and line j+1 out of order against it (no code of its own: line j is reported)."""
    late = ("ins", b"#late", "BGC_HEADER_LATE")
    empty = ("ins", b"", "BGC_EMPTY")
    nested = ("after", _nested_after, "BGC_NESTED")
    below = ("rep", _start_below, "BGC_UNSORTED_START")
    schar = ("ins", b"chr2\t5x\t9", "BGC_S_CHAR")
    t2 = 2 * TILE
    sets = [
        ("late-empty", 0, [(TILE + 100, *late), (3 * TILE + 100, *empty)]),
        ("nested-empty", 1, [(TILE + 100, *nested), (3 * TILE + 100, *empty)]),
        ("nested-start-empty", 1, [(TILE + 100, *nested), (t2 + 100, *below), (3 * TILE + 100, *empty)]),
        ("late-start-schar", 0, [(TILE - 10, *late), (t2 - 10, *below), (4 * TILE - 10, *schar)]),
        ("waves", 0, [(t2 + 10, *late), (t2 + 2 * WAVE_BYTES + 10, *schar)]),
        ("waves-nested", 1, [(t2 + WAVE_BYTES - 5, *nested), (t2 + 3 * WAVE_BYTES + 5, *empty)]),
        ("threads", 0, [(t2 + WAVE_BYTES + 3 * THREAD_BYTES, *late),
                        (t2 + WAVE_BYTES + 40 * THREAD_BYTES, *empty)]),
    ]
    out = []
    for tag, nest, edits in sets:
        for skip in range(len(edits) - 1):
            lines, defects = _edit(base_lines(), edits[skip:])
            out.append(_case(f"D-{tag}" + ("-later%d" % skip if skip else ""), join(lines), 3, 1, nest,
                             expect=defects[0][1], row=defects[0][0], at=offset_of(lines, defects[0][0] - 1),
                             defects=defects))
        lines, defects = _edit(base_lines(), edits[-1:])
        out.append(_case(f"D-{tag}-last", join(lines), 3, 1, nest, expect=defects[0][1],
                         row=defects[0][0], at=offset_of(lines, defects[0][0] - 1), defects=defects))
    for d in (-40, 0):
        lines = base_lines()
        j = first_line_at(lines, t2 + d)
        c, s, e = _fields(lines[j])
        lines[j] = b"%s\t%dx\t%d" % (c, s, e)
        lines[j + 1] = b"%s\t%d\t%d" % (c, s - 50, e)
        out.append(_case(f"D-grammar-then-order{d:+d}", join(lines), 3, 1, expect="BGC_S_CHAR",
                         row=j + 1, at=offset_of(lines, j)))
    return out


# ------------------------------------------------------------------ E: file ends
def _sized(tail, size):
    """rows on chr1, then the lines `tail`, `size` bytes in all with a final newline"""
    tail_bytes = offset_of(tail, len(tail))
    pre = rows_upto(b"chr1", size - tail_bytes)
    return place(pre + list(tail), len(pre), size - tail_bytes)


def family_e():
    tails = [("ok", [b"chr9\t50\t60", b"chr9\t55\t60"], None),
             ("order", [b"chr9\t50\t60", b"chr9\t40\t60"], "BGC_UNSORTED_START"),
             ("gram", [b"chr9\t50\t60", b"chr9\t55\t6y0"], "BGC_E_CHAR")]
    out = []

    def add(name, lines, newline, more, expect, more_expect):
        """`lines`, whose last one carries `expect`; then the bytes `more`, which make one more
        line that fails with `more_expect`"""
        data = join(lines, newline) + more
        if expect:
            meta = dict(expect=expect, row=len(lines), at=offset_of(lines, len(lines) - 1))
        elif more_expect:
            meta = dict(expect=more_expect, row=len(lines) + 1, at=offset_of(lines, len(lines)))
        else:
            meta = dict(expect=None)
        out.append(_case(name, data, 3, 1, **meta))

    for k in (1, 3):
        for tag, tail, expect in tails:
            # no trailing newline: mid-tile, and with the last byte closing / opening a tile
            for sz in (k * TILE + 777, k * TILE + 1, k * TILE + 2):
                add(f"E-nonl-{sz - 1}-{tag}", _sized(tail, sz), False, b"", expect, None)
            add(f"E-exact-{k}-{tag}", _sized(tail, k * TILE), True, b"", expect, None)
            add(f"E-plus1nl-{k}-{tag}", _sized(tail, k * TILE + 1), True, b"", expect, None)
            # a lone unterminated 'c' opens the last tile: a defect itself, unless one comes before
            add(f"E-plus1c-{k}-{tag}", _sized(tail, k * TILE), True, b"c", expect, "BGC_NO_TABS")
            # "\n\n": one empty last line (no second one after the final newline)
            for sz in (k * TILE - 1, k * TILE, k * TILE + 500):
                add(f"E-nlnl-{sz + 1}-{tag}", _sized(tail, sz), True, b"\n", expect, "BGC_EMPTY")
    for i, (data, expect) in enumerate([(b"chr1\t5\t10\n", None), (b"chr1\t5\t10", None),
                                        (b"chr1\t7\t5\n", "BGC_END_LE_START"), (b"chr1\t7\t5", "BGC_END_LE_START"),
                                        (b"c", "BGC_NO_TABS"), (b"\n", "BGC_EMPTY"), (b"#h", None),
                                        (b"#h\n", None), (b"\n\n", "BGC_EMPTY")]):
        out.append(_case(f"E-oneline{i}", data, 3, 1,
                         **(dict(expect=expect, row=1, at=0) if expect else dict(expect=None))))
    return out


# ------------------------------------------------------------------ F: long fields
def rest_line(n, nf):
    """a row with n bytes after the tab that ends field nf (3 or 5)"""
    return (b"chr1\t5\t10\t" if nf == 3 else b"chr1\t5\t10\tid\t1\t") + b"r" * n


def rest_probe(n, nf):
    return _case(f"F-probe-{nf}-{n}", join([row(b"chr0", 1, 2), rest_line(n, nf), row(b"chr3", 1, 2)]), nf, 1)


def family_f(threshold5, threshold3):
    """each long line is row >= 2 and a sorted row follows it. threshold*: the smallest
    n at which the oracle rejects rest_line(n, 5) and rest_line(n, 3) (the test finds them)."""
    out = []
    for n, expect in ((127, None), (128, "BGC_CHR_LONG")):
        for nf in (3, 5):
            lines, f = embed([b"chr2" + b"a" * (n - 4) + b"\t5\t10\tid\t1\t+\tx"], 0, TILE + 37)
            out.append(_case(f"F-chrom{n}-{nf}", join(lines), nf, 1,
                             **(dict(expect=expect, row=f + 1, at=TILE + 37) if expect else dict(expect=None))))
    for n, expect in ((16383, None), (16384, "BGC_ID_LONG")):
        for at in (TILE + 37, 3 * TILE - 16000):  # (the second: the id itself spans two seams)
            lines, f = embed([b"chr1\t5\t10\t" + b"i" * n + b"\t1\t+\tx"], 0, at, total=BASE_BYTES + 2 * TILE)
            out.append(_case(f"F-id{n}-{at}", join(lines), 5, 1,
                             **(dict(expect=expect, row=f + 1, at=at) if expect else dict(expect=None))))
    for nf, thr in ((5, threshold5), (3, threshold3)):
        for n, expect in ((thr - 1, None), (thr, "BGC_REST_LONG")):
            lines, f = embed([rest_line(n, nf)], 0, TILE + 5, total=0)
            lines += rows_upto(b"chr3", 2 * TILE)
            out.append(_case(f"F-rest{nf}-{n}", join(lines), nf, 1,
                             **(dict(expect=expect, row=f + 1, at=TILE + 5) if expect else dict(expect=None))))
    return out


# ------------------------------------------------------------------ G: past the scan's first level
def family_g():
    """one clean file of more than SCAN_TILE tiles (the tile counts need the scan's second
    level), and the same file with one row's start lowered in tile SCAN_TILE-1, in tile
    SCAN_TILE (across the seam of the second level) and in the last tile"""
    rows = 420000
    data = b"".join(b"chr1\t%d\t%d\n" % (1000000 + 7 * i, 1000005 + 7 * i) for i in range(rows))
    ntiles = (len(data) + TILE - 1) // TILE
    assert ntiles > SCAN_TILE + 1 and len(data) % TILE > 100
    out = [_case("G-clean", data, 3, 0, expect=None)]
    line = len(data) // rows  # every row has the same length
    assert len(data) == line * rows
    for tag, off in (("t%d" % (SCAN_TILE - 1), (SCAN_TILE - 1) * TILE + 4000), ("t%d" % SCAN_TILE, SCAN_TILE * TILE),
                     ("t%d+" % SCAN_TILE, SCAN_TILE * TILE + 4000), ("last", (ntiles - 1) * TILE + 40)):
        r = (off + line - 1) // line  # 0-based row that starts at or after `off`
        bad = bytearray(data)
        bad[r * line + 5:r * line + 6] = b"0"  # the start's first digit: below the previous row's
        out.append(_case(f"G-{tag}", bytes(bad), 3, 0, expect="BGC_UNSORTED_START", row=r + 1, at=r * line))
    return out


# ------------------------------------------------------------------ H: dense newlines
def family_h():
    """valid rows, then 40 consecutive newlines: one thread owns 32 one-byte lines; the first
    empty line is reported"""
    out = []
    for i, at in enumerate((3 * THREAD_BYTES, 2 * TILE + 2 * THREAD_BYTES, 2 * TILE + 5, TILE - 20, 3 * TILE)):
        lines, f = embed([b""] * 40, 0, at)
        out.append(_case(f"H-{at}", join(lines), 3, i % 2, expect="BGC_EMPTY", row=f + 1, at=at))
    lines = rows_upto(b"chr1", 3 * THREAD_BYTES)
    out.append(_case("H-tail", join(lines) + b"\n" * 40, 3, 1, expect="BGC_EMPTY", row=len(lines) + 1))
    return out


# ------------------------------------------------------------------ the seam sweep
def sweep():
    """the base file with its first row grown by 0..63 bytes, so that every seam passes through
    every alignment against the lines: each shift once clean and once with one row of tile 2
    starting below the row before it"""
    out = []
    for shift in range(2 * THREAD_BYTES):
        lines = base_lines()
        lines[0] += b"x" * shift
        nf, rest = ((3, 0), (3, 1), (5, 1), (6, 1))[shift % 4]
        out.append(_case(f"S-{shift}-clean", join(lines), nf, rest, shift % 2, expect=None))
        j = first_line_at(lines, 2 * TILE)
        if shift % 2:  # (the row the tile's last newline ends; else the first row inside the tile)
            j += 1
        lines[j] = _start_below(lines[j])
        out.append(_case(f"S-{shift}-order", join(lines), nf, rest, shift % 2, expect="BGC_UNSORTED_START",
                         row=j + 1, at=offset_of(lines, j)))
    return out
