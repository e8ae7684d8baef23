"""Generated bedops inputs that put rows and components where the sweep kernels of
bedops_amd/csrc/bg_setops.hip can go wrong: on the seams of k_components' 64-row items, 512-row
waves and 2048-row tiles and of k_tile_max's 4-tile workgroups, on the diagonals of the
1024-element merge-path tiles (which are also the segments of a segmented result) and on their
4-element thread seams, over whole tiles that hold one input only, around the 256-row blocks
and the 1024-component LDS slice of k_element_flags, and over whole 512-row stretches of kept
and of dropped rows. Pure Python: the CPU test (tests/test_setop_cases.py) proves with
tests/model_setops.py that every input is what this file says it is and that the model gives
the oracle's bytes on it; the GPU test (tests/test_gpu_setop_seams.py) runs the kernels on the
same cases against the oracle.

Every family is a list of Case(name, op, args, texts): `bedops <op> <args> file0 file1 ...` on
the BED texts. META[name] holds what the generator knows about the case by construction:
  n, ncomp   A: rows of the file, components it merges to
  seam, rel  A: row `seam` starts at the running maximum end of the rows before it ("touch"),
             one base after it ("short") or one base before it ("over")
  back       A: that maximum is the end of row seam - back; the rows between are nested in it
  closed     A: rows [a, b) open no component
  chrom_at   A: row chrom_at is the first of its chromosome, the row before ends at 2^40 - 1
  plain      B: every row of every file is a component of its own
  at         B: {d: ("x"|"y", index, (chrom, start, end))}: the element at merged position d
             in the kernel's order (x = file 0, y = file 1)
  total      B: merged elements, nx + ny
  empty, full, only_x, only_y
             B: merge-path tiles that emit nothing, that emit MP_TILE pieces, that hold
             elements of one input only
  cross      C: element counts that some merged list of the fold exceeds
  block, span  D: reference rows [256 * block, 256 * block + 256) reach over `span` components
  kept, dropped  D: reference rows [a, b) that are all kept / all dropped
"""
import os
import re
from typing import NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bedops_amd", "csrc")

# the kernels' geometry, stated here; test_setop_cases.py greps the sources for it
# (source_constants), so a retune fails there instead of quietly moving the seams
CT_ITEMS = 8         # k_components: rows per lane per wave, in items of 64 rows
WAVE_ROWS = 512      # 64 lanes x CT_ITEMS
CT_TILE = 2048       # rows per k_components workgroup
TM_TILES = 4         # k_components tiles per k_tile_max workgroup (8192 rows)
MP_ITEMS = 4         # merged elements per thread of k_mp_tile and k_merge_sorted
MP_TILE = 1024       # merged elements per workgroup
BG_SEG_CAP = 1024    # pieces a segment of a segmented result holds (= MP_TILE)
BG_NT = 256          # threads per workgroup; reference rows per k_element_flags block
EF_SLICE = 1024      # components k_element_flags stages in LDS
CF_TILE = 4096       # flags per k_compact_flags workgroup
FMT_TILE = 512       # output rows per format tile (BG_FMT_TILE)
CONSTANTS = (CT_ITEMS, WAVE_ROWS, CT_TILE, TM_TILES, MP_ITEMS, MP_TILE, BG_SEG_CAP, BG_NT, EF_SLICE,
             CF_TILE, FMT_TILE)

COORD_MAX = (1 << 40) - 1
# where coordinates start: 7 digits make a row of at least 16 bytes, so that a 4 KiB sub-tile of
# the set loader holds fewer than the 256 components it stages (bg_load.hip, SCAP_W) and the
# "set" route stays a set load instead of being redone with row columns
BASE = 1000000
CHROMS = ("chr1", "chr10", "chr2")                    # strcmp order, names of 4, 5 and 4 bytes
WIDE_CHROMS = ("7", "chr1", "chr10", "chr2_random9")  # names of 1 and of 12 bytes
SEAMS = (64, WAVE_ROWS, CT_TILE, TM_TILES * CT_TILE)

# the ways a case is run on the GPU (tests/test_gpu_setop_seams.py): "set" = text, inputs parsed
# straight to their components where the operation allows it (the front-end's route); "rows" =
# text, every input kept as rows (k_tile_max / k_components); "columns" = Engine.load_columns
ROUTES = {"A": ("set", "rows", "columns"), "B": ("set", "rows", "columns"),
          "C": ("set", "rows", "columns"), "D": ("set", "rows", "columns")}


class Case(NamedTuple):
    name: str
    op: str
    args: tuple
    texts: list


META = {}


def _case(name, op, args, files, **meta):
    META[name] = meta
    return Case(name, op, tuple(args), [text(f) for f in files])


def routes(case):
    return META[case.name].get("routes", ROUTES[case.name[0]])


def text(rows):
    return "".join("%s\t%d\t%d%s\n" % (r[0], r[1], r[2], r[3] if len(r) > 3 else "") for r in rows).encode()


def rows_of(data):
    """BED text -> [(chrom, start, end)]"""
    out = []
    for ln in data.decode().splitlines():
        f = ln.split("\t")
        out.append((f[0], int(f[1]), int(f[2])))
    return out


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def source_constants():
    """CONSTANTS as bg_setops.hip and bg_internal.h define them"""
    so, internal = _src("bg_setops.hip"), _src("bg_internal.h")

    def num(src, name):
        return int(re.search(r"#define %s (\d+)\b" % name, src).group(1))

    nt, cap, fmt = num(internal, "BG_NT"), num(internal, "BG_SEG_CAP"), num(internal, "BG_FMT_TILE")
    ct_items, tm, mp_items = num(so, "CT_ITEMS"), num(so, "TM_TILES"), num(so, "MP_ITEMS")
    ef, cf_items = num(so, "EF_SLICE"), num(so, "CF_ITEMS")
    assert re.search(r"#define CT_WROWS \(64 \* CT_ITEMS\)", so)
    assert re.search(r"#define CT_TILE \(BG_NT \* CT_ITEMS\)", so)
    assert re.search(r"#define MP_TILE \(BG_NT \* MP_ITEMS\)", so)
    assert re.search(r"#define CF_TILE \(BG_NT \* CF_ITEMS\)", so)
    assert re.search(r"\(uint64_t\)blockIdx\.x \* BG_NT;", so)  # k_element_flags: one row per thread
    return (ct_items, 64 * ct_items, nt * ct_items, tm, mp_items, nt * mp_items, cap, nt, ef,
            nt * cf_items, fmt)


# ------------------------------------------------------------------ A: components
class Track:
    """one file, built row by row in file order"""

    def __init__(self, chroms=CHROMS, pos=BASE):
        self.rows, self.chroms, self.ci, self.pos = [], chroms, 0, pos

    @property
    def n(self):
        return len(self.rows)

    def next_chrom(self, pos=BASE + 50):
        self.ci += 1
        self.pos = pos

    def row(self, s, e):
        self.rows.append((self.chroms[self.ci], s, e))

    def disjoint(self, k, ln=5, gap=3):
        for _ in range(k):
            self.row(self.pos, self.pos + ln)
            self.pos += ln + gap

    def chained(self, k, ln=5, gap=3):
        """k rows, each ending at the next one's start: one component"""
        for _ in range(k):
            self.row(self.pos, self.pos + ln)
            self.pos += ln
        self.pos += gap

    def disjoint_over(self, k, nchroms):
        """k disjoint rows over `nchroms` more-or-less equal chromosomes (this one first)"""
        for c in range(nchroms):
            self.disjoint(k * (c + 1) // nchroms - k * c // nchroms)
            if c + 1 < nchroms:
                self.next_chrom()


A_COUNTS = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 8191, 8192, 8193, 8192 + 2048 + 1)
A_BACK = (2, 70, 600, 2100)
A_RELS = (("touch", 0), ("short", 1), ("over", -1))
A_TAIL = 300  # disjoint rows after a seam


def family_a_counts():
    """row counts around every seam, each all disjoint (n components) and all chained (one
    component per chromosome); three chromosomes from 3 rows up, changing away from the seams"""
    out = []
    for n in A_COUNTS:
        nc = 3 if n >= 3 else 1
        t = Track()
        t.disjoint_over(n, nc)
        out.append(_case(f"A-n{n}-disjoint", "-m", (), [t.rows], n=n, ncomp=n))
        t = Track()
        for c in range(nc):
            t.chained(n * (c + 1) // nc - n * c // nc)
            if c + 1 < nc:
                t.next_chrom()
        out.append(_case(f"A-n{n}-chained", "-m", (), [t.rows], n=n, ncomp=nc))
    return out


def family_a_seams():
    """row p-1 meets row p (p a seam): touching, one base short, one base over; then the same
    with the covering row `back` rows before p and only nested rows between (every back <= p)"""
    out = []
    for p in SEAMS:
        for back in (1,) + tuple(k for k in A_BACK if k <= p):
            for rel, delta in A_RELS:
                t = Track()
                t.disjoint_over(p - back, 2)  # (rows 0 .. p-back-1; the chromosome changes at half)
                c = t.pos
                end = c + 10 * back + 50
                t.row(c, end)                   # row p-back: its end is the running maximum at p
                for j in range(back - 1):       # rows p-back+1 .. p-1, nested
                    t.row(c + 1 + 3 * j, c + 3 + 3 * j)
                assert t.n == p
                t.row(end + delta, end + delta + 7)
                t.pos = end + delta + 10
                t.disjoint(A_TAIL)
                name = f"A-seam{p}-{rel}" if back == 1 else f"A-seam{p}-back{back}-{rel}"
                out.append(_case(name, "-m", (), [t.rows], n=t.n, seam=p, back=back, rel=rel,
                                 ncomp=p - back + 1 + (rel == "short") + A_TAIL))
    return out


ABSORB_AT, ABSORB_LAST = 100, 3 * CT_TILE + 5


def family_a_other():
    out = []
    # one row near index 100 covers through index 3 * 2048 + 5: tiles 1 and 2 open nothing, and
    # the component's end is written by tile 3, its start by tile 0
    t = Track()
    t.disjoint(ABSORB_AT)
    c = t.pos
    end = c + 3 * (ABSORB_LAST - ABSORB_AT) + 100
    t.row(c, end)
    for j in range(ABSORB_LAST - ABSORB_AT):
        t.row(c + 1 + 3 * j, c + 3 + 3 * j)
    assert t.n == ABSORB_LAST + 1
    t.pos = end + 5
    t.disjoint(200)
    t.next_chrom()
    t.disjoint(A_TAIL)
    out.append(_case("A-absorb", "-m", (), [t.rows], n=t.n, ncomp=ABSORB_AT + 1 + 200 + A_TAIL,
                     closed=(ABSORB_AT + 1, ABSORB_LAST + 1)))
    # a chromosome change exactly at a seam, the outgoing chromosome ending at 2^40 - 1 and the
    # incoming one starting at 0 (keys one apart)
    for p in SEAMS:
        t = Track()
        t.disjoint_over(p - 1, 2)
        assert t.n == p - 1 and t.ci == 1
        t.row(t.pos, COORD_MAX)
        t.next_chrom(pos=0)
        t.disjoint(A_TAIL)
        out.append(_case(f"A-chromseam{p}", "-m", (), [t.rows], n=t.n, ncomp=t.n, chrom_at=p))
    # a component that ends on the file's last row: lane 63 of item 7, and lane 0
    for n in (CT_TILE, CT_TILE + 1):
        t = Track()
        t.disjoint_over(n - 5, 3)
        t.chained(5)
        out.append(_case(f"A-lastrow-n{n}", "-m", (), [t.rows], n=n, ncomp=n - 4, last_chain=5))
    return out


def family_a():
    return family_a_counts() + family_a_seams() + family_a_other()


# ------------------------------------------------------------------ B: merge-path tiles
class Duo:
    """two files of components (x = file 0, y = file 1), built element by element in the
    kernel's merged order for `op`, so that the next element's merged position is d"""

    def __init__(self, op, chroms=CHROMS, pos=BASE):
        self.op, self.f, self.chroms, self.ci, self.pos = op, ([], []), chroms, 0, pos
        self.placed = []  # ("x"|"y", index, row) in merged order

    @property
    def d(self):
        return len(self.placed)

    def next_chrom(self, pos=BASE + 10):
        self.ci += 1
        self.pos = pos

    def put(self, w, s, e):
        row = (self.chroms[self.ci], s, e)
        self.f[w].append(row)
        self.placed.append(("xy"[w], len(self.f[w]) - 1, row))

    def lone(self, w, k=1):
        """k elements of file w that overlap nothing"""
        for _ in range(k):
            self.put(w, self.pos, self.pos + 4)
            self.pos += 10

    def loud(self, k=1):
        """k pairs X = [p, p+10), Y = [p+4, p+7): X comes first under either operation;
        -i gives [p+4, p+7), -d gives [p, p+4) and [p+7, p+10)"""
        for _ in range(k):
            p = self.pos
            self.put(0, p, p + 10)
            self.put(1, p + 4, p + 7)
            self.pos += 16

    def fill(self, n):
        """n elements that emit pieces"""
        self.loud(n // 2)
        self.lone(0, n % 2)

    def fill_to(self, d, spread=True):
        """elements that emit pieces up to merged position d; past 200 of them the chromosome
        changes half way (the last chromosome is left to the caller)"""
        n = d - self.d
        assert n >= 0, (d, self.d)
        if spread and n >= 200 and self.ci + 2 < len(self.chroms):
            self.fill(n // 2)
            self.next_chrom()
            n = d - self.d
        self.fill(n)
        assert self.d == d

    def quiet(self, n):
        """n elements that emit nothing: -i: x and y in turn, apart; -d: y only (outside any x)"""
        if self.op == "-i":
            for k in range(n):
                self.lone(k % 2)
        else:
            self.lone(1, n)

    def at(self, *ds):
        return {d: self.placed[d] for d in ds}

    def case(self, name, **meta):
        return _case(f"B{self.op}-{name}", self.op, (), list(self.f), plain=True, total=self.d, **meta)


B_TOTALS = (1, 4, MP_TILE - 1, MP_TILE, MP_TILE + 1, 2 * MP_TILE, 3 * MP_TILE + 1)
B_TARGETS = (MP_TILE, 2 * MP_TILE, MP_TILE + 4 * 37)  # two diagonals, one thread seam in a tile


def _gadgets(op):
    """(tag, g, build): build(duo) appends a few elements in merged order, of which element g is
    the one to sit on the diagonal (element g-1 is the last of the tile or thread before)"""
    def i_xy(b):   # X starts first; Y (on the diagonal) finds it through the X halo
        p = b.pos; b.put(0, p, p + 10); b.put(1, p + 4, p + 14); b.pos += 20

    def i_yx(b):   # Y starts first; X finds it through the Y halo
        p = b.pos; b.put(1, p, p + 10); b.put(0, p + 4, p + 14); b.pos += 20

    def i_tie(b):  # equal starts: Y first
        p = b.pos; b.put(1, p, p + 6); b.put(0, p, p + 10); b.pos += 16

    def d_xy(b):   # R's first O lies past the tile; O finds R through the X halo
        p = b.pos; b.put(0, p, p + 10); b.put(1, p + 4, p + 7); b.pos += 16

    def d_yy(b):   # two O inside one R: the first one's "next O start" lies one past its tile
        p = b.pos; b.put(0, p, p + 30); b.put(1, p + 4, p + 7); b.put(1, p + 10, p + 13); b.pos += 36

    def d_yx(b):   # O, then the next R: O is the last Y of its tile, the next O two elements on
        p = b.pos
        b.put(0, p, p + 16); b.put(1, p + 8, p + 13); b.put(0, p + 18, p + 30); b.put(1, p + 22, p + 25)
        b.pos += 36

    def d_tie(b):  # X start == Y end (touching): Y first
        p = b.pos; b.put(1, p, p + 5); b.put(0, p + 5, p + 12); b.pos += 18

    def d_oend(b):  # O ends exactly at R's end: no piece after it
        p = b.pos; b.put(0, p, p + 10); b.put(1, p + 6, p + 10); b.pos += 16

    if op == "-i":
        return [("xy", 1, i_xy), ("yx", 1, i_yx), ("tie", 1, i_tie), ("tie-after", 0, i_tie)]
    return [("xy", 1, d_xy), ("yy", 2, d_yy), ("yx", 2, d_yx), ("tie", 1, d_tie), ("tie-after", 0, d_tie),
            ("oend", 1, d_oend)]


def family_b(op):
    out = []
    # element counts
    for total in B_TOTALS:
        b = Duo(op)
        b.fill_to(total)
        out.append(b.case(f"n{total}"))
    for w in (0, 1):  # either input empty
        b = Duo(op)
        b.lone(1 - w, 5)
        out.append(b.case("xempty" if w == 0 else "yempty"))
    # one element against 3000: tiles with no X, tiles with no Y
    for w in (0, 1):
        b = Duo(op)
        b.lone(1 - w, 750); b.next_chrom(); b.lone(1 - w, 750)
        p = b.pos
        wide = (w, p, p + 14)
        small = [(1 - w, p + 2, p + 6), (1 - w, p + 9, p + 12)]
        # (the wide one starts first; under -d a wide O is placed by its end, after the two R)
        for e in ([wide] + small if (op == "-i" or w == 0) else small + [wide]):
            b.put(*e)
        b.pos += 20
        b.lone(1 - w, 748); b.next_chrom(); b.lone(1 - w, 750)
        assert len(b.f[w]) == 1 and len(b.f[1 - w]) == 3000
        out.append(b.case("x1-y3000" if w == 0 else "x3000-y1"))
    # an overlapping pair split by a diagonal, and by a thread seam
    for tag, g, build in _gadgets(op):
        for target in B_TARGETS:
            b = Duo(op)
            b.fill_to(target - g)
            build(b)
            b.next_chrom()
            b.fill(300)
            out.append(b.case(f"{tag}-d{target}", at=b.at(target - 1, target)))
    # one component over more than two whole tiles of the other file
    n_in = 3 * MP_TILE + 200
    b = Duo(op)  # x covers: the tiles after the first hold y only, all served by one X halo
    b.fill_to(100)
    p = b.pos
    b.put(0, p, p + 6 * n_in + 10)
    for k in range(n_in):
        b.put(1, p + 2 + 6 * k, p + 5 + 6 * k)
    b.pos = p + 6 * n_in + 20
    b.next_chrom()
    b.fill(50)
    out.append(b.case("xcovers", only_y=[1, 2], at=b.at(100, MP_TILE, 2 * MP_TILE),
                      **({"full": [1, 2]} if op == "-d" else {})))
    b = Duo(op)  # y covers
    b.fill_to(100)
    p = b.pos
    if op == "-i":
        b.put(1, p, p + 6 * n_in + 10)
        for k in range(n_in):
            b.put(0, p + 2 + 6 * k, p + 5 + 6 * k)
        meta = {}
    else:  # (placed by its end: after every R it covers; the first R sticks out on the left)
        b.put(0, p - 3, p + 4)
        for k in range(1, n_in):
            b.put(0, p + 2 + 6 * k, p + 5 + 6 * k)
        b.put(1, p, p + 6 * n_in + 10)
        meta = {"empty": [1, 2]}
    b.pos = p + 6 * n_in + 20
    b.next_chrom()
    b.fill(50)
    out.append(b.case("ycovers", only_x=[1, 2], at=b.at(100, MP_TILE, 2 * MP_TILE), **meta))
    # empty segments: first, in the middle, last
    b = Duo(op); b.quiet(2 * MP_TILE + 52); b.next_chrom(); b.fill(1000)
    out.append(b.case("quiet-first", empty=[0, 1]))
    b = Duo(op); b.fill_to(MP_TILE - 4, spread=False); b.next_chrom(); b.quiet(2 * MP_TILE + 12)
    b.next_chrom(); b.fill(1000)
    out.append(b.case("quiet-mid", empty=[1, 2]))
    b = Duo(op); b.fill_to(MP_TILE + 6, spread=False); b.next_chrom(); b.quiet(2 * MP_TILE + 76)
    out.append(b.case("quiet-last", empty=[2, 3]))
    # printed widths: neighbouring segments with names of 1 and 12 bytes, coordinates across
    # 10^9 and up to 2^40 - 1
    b = Duo(op, WIDE_CHROMS, pos=3)
    b.fill_to(MP_TILE, spread=False)
    b.next_chrom(pos=10 ** 9 - 16 * 300)
    b.fill_to(2 * MP_TILE, spread=False)
    b.next_chrom(pos=COORD_MAX - 16 * (MP_TILE // 2) + 6)
    b.fill_to(3 * MP_TILE, spread=False)
    assert b.f[0][-1][2] == COORD_MAX
    b.next_chrom(pos=99990)
    b.fill(601)
    out.append(b.case("widths"))
    if op == "-d":
        b = Duo(op)  # O components before the first R of the file
        b.lone(1, 2)
        p = b.pos
        b.put(0, p + 10, p + 30); b.put(1, p, p + 15)  # (R first: its start is below O's end)
        b.pos += 40
        b.fill(200)
        out.append(b.case("ofirst", at=b.at(0, 1, 2, 3)))
        b = Duo(op)  # the first element of tile 1 is an O, and tile 1 holds no X at all
        b.fill_to(MP_TILE - 1)
        p = b.pos
        b.put(0, p, p + 6 * 1100 + 10)
        for k in range(1100):
            b.put(1, p + 2 + 6 * k, p + 5 + 6 * k)
        b.pos = p + 6 * 1100 + 20
        b.next_chrom()
        b.fill(100)
        out.append(b.case(f"ohead-d{MP_TILE}", only_y=[1], full=[1], at=b.at(MP_TILE - 1, MP_TILE)))
        for total in (MP_TILE, MP_TILE + 6):  # the file's last Y: its "next O start" is the sentinel
            b = Duo(op)
            b.fill_to(total - 2)
            p = b.pos
            b.put(0, p, p + 30); b.put(1, p + 4, p + 7)
            out.append(b.case(f"sentinel-n{total}", at=b.at(total - 1)))
    return out


# ------------------------------------------------------------------ C: folds over 3 and 4 files
def _comb(n, period, off, ln, chroms=CHROMS, extra=()):
    """n rows [period*i + off, + ln) over the chromosomes in thirds (coordinates restart with
    each chromosome), every 7th followed by a row nested in it; extra: {i: (off, ln)} overrides"""
    out = []
    for c in range(len(chroms)):
        lo, hi = n * c // len(chroms), n * (c + 1) // len(chroms)
        for i in range(hi - lo):
            o, l = extra.get(lo + i, (off, ln)) if extra else (off, ln)
            s = BASE + period * i + o
            out.append((chroms[c], s, s + l))
            if (lo + i) % 7 == 0 and l > 2:
                out.append((chroms[c], s + 1, s + l - 1))
    return out


def family_c():
    """-m: union folds through k_merge_sorted (ties X first; lists of 1401 and about 2100
    elements, neither a multiple of 4); -i: the folds before the last one are k_mp_tile's count
    and write pair; -d: the other files are united first"""
    out = []
    ties = {i: (0, 5) for i in range(0, 700, 50)}   # f1 rows that start where f0's do
    bridge = {i: (11, 4) for i in range(0, 702, 9)}  # f2 rows that join f0's row to f1's
    m = [_comb(701, 20, 0, 12), _comb(700, 20, 14, 4, extra=ties), _comb(702, 20, 3, 5, extra=bridge),
         _comb(500, 28, 1, 20)]
    i_ = [_comb(1300, 20, 0, 12), _comb(1300, 20, 5, 11), _comb(900, 30, 2, 23), _comb(600, 50, 0, 45)]
    d = [_comb(1500, 20, 0, 15), _comb(800, 37, 3, 6), _comb(800, 41, 1, 5), _comb(700, 43, 7, 9)]
    for op, files in (("-m", m), ("-i", i_), ("-d", d)):
        for nf in (3, 4):
            out.append(_case(f"C{op}-{nf}files", op, (), files[:nf], cross=[MP_TILE, 2 * MP_TILE]))
    return out


# ------------------------------------------------------------------ D: element-of
D_SHAPES = ((1, 4), (1, 9), (3, 8), (5, 10), (4, 11), (0, 5))
# a reference row of shape (a, b) at component j = [10j, 10j+5) is [10j+a, 10j+b): covered to
# 3/3, 4/8 (exactly half), 2/5, 0/5, 2/7 (one base of component j, one of j+1) and 5/5
D_COUNTS = (BG_NT - 1, BG_NT, BG_NT + 1, CF_TILE - 1, CF_TILE, CF_TILE + 1)
D_SPECS = ("1", "50%", "100%")


def _rest(i):
    return "\tid%d" % i + ("\t" + "x" * (i % 23) + "\t+" if i % 3 else "")


def _d_files(n, shape_of, wide=None, ncomps=None):
    """n reference rows (row i at component i, with a remainder of varying length) and the
    other file's components; two thirds on chr1, the rest on chr10. wide = (row, components):
    that row reaches from its component to the first base of the last of `components`"""
    ncomps = ncomps or n + 5
    cut = max(2 * n // 3, (wide[0] + wide[1] + 8) if wide else 0)
    where = lambda j: (CHROMS[0], BASE + 10 * j) if j < cut else (CHROMS[1], BASE + 10 * (j - cut))
    ref = []
    for i in range(n):
        c, base = where(i)
        a, b = D_SHAPES[shape_of(i)]
        if wide and i == wide[0]:
            a, b = 1, 10 * (wide[1] - 1) + 1
        ref.append((c, base + a, base + b, _rest(i)))
    other = []
    for j in range(ncomps):
        c, base = where(j)
        other.append((c, base, base + 5))
    return [ref, other]


def family_d():
    out = []
    cyc = lambda i: i % len(D_SHAPES)
    for n in D_COUNTS:
        for op in ("-e", "-n"):
            for spec in D_SPECS:
                out.append(_case(f"D{op}-n{n}-{spec}", op, (spec,), _d_files(n, cyc), n=n))
    # block 1 (rows 256..511) reaches over exactly 1024 components (staged in LDS) and over
    # 1025 (searched in global memory); the wide row is covered to exactly half; the last
    # block (rows 512..600) is partly filled
    for span in (EF_SLICE, EF_SLICE + 1):
        for op in ("-e", "-n"):
            for spec in ("1", "50%"):
                files = _d_files(601, cyc, wide=(BG_NT, span), ncomps=BG_NT + span + 400)
                out.append(_case(f"D{op}-span{span}-{spec}", op, (spec,), files, n=601, block=1, span=span))
    # 512 consecutive rows all kept, then 512 none kept (-e; the reverse under -n), then a mix
    def blocks(i):
        return 0 if i < FMT_TILE else 3 if i < 2 * FMT_TILE else cyc(i)
    for op in ("-e", "-n"):
        files = _d_files(2300, blocks)
        a, b = (0, FMT_TILE), (FMT_TILE, 2 * FMT_TILE)
        out.append(_case(f"D{op}-tiles", op, ("1",), files, n=2300, kept=a if op == "-e" else b,
                         dropped=b if op == "-e" else a))
    return out


FAMILIES = [("A-counts", family_a_counts), ("A-seams", family_a_seams), ("A-other", family_a_other),
            ("B-i", lambda: family_b("-i")), ("B-d", lambda: family_b("-d")), ("C", family_c),
            ("D", family_d)]
