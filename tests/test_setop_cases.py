"""The generated inputs of tests/setop_cases.py on the CPU: the geometry the generator places
its seams by is the sources'; every case is what its META says it is, proved with the model of
the kernels' formulation (tests/model_setops.py: which row opens a component, the merged order
with positions, the pieces of each merge-path tile, the component range of an element-of
block); and on every case the model gives the oracle's bytes (oracle/bedops_oracle.c). The
oracle is the reference; the model is only what locates the seams.
tests/test_gpu_setop_seams.py runs the kernels on the same cases."""
import os
import subprocess

import pytest

import model_setops as M
import setop_cases as S

MODE = {"-i": "i", "-d": "d"}
SPEC = {"1": (1.0, 0), "50%": (0.5, 1), "100%": (1.0, 1)}


def keyed(case):
    """-> ([keyed rows of each file], names in strcmp order, [rows of each file])"""
    rows = [S.rows_of(t) for t in case.texts]
    names = sorted({r[0] for f in rows for r in f}, key=lambda s: s.encode())
    rank = {n: i for i, n in enumerate(names)}
    return [[((rank[c] << M.SHIFT) | s, (rank[c] << M.SHIFT) | e) for c, s, e in f] for f in rows], names, rows


def render(pieces, names):
    mask = (1 << M.SHIFT) - 1
    return "".join(f"{names[s >> M.SHIFT]}\t{s & mask}\t{e & mask}\n" for s, e in pieces).encode()


def model_output(case, k, names):
    if case.op == "-m":
        return render(M.union_components(k), names)
    if case.op == "-i":
        acc = M.components(k[0])
        for f in k[1:]:
            acc = M.intersect2(acc, M.components(f))
        return render(acc, names)
    if case.op == "-d":
        return render(M.difference2(M.components(k[0]), M.union_components(k[1:])), names)
    thres, pct = SPEC[case.args[0]]
    keep = M.element_of(k[0], M.union_components(k[1:]), thres, pct, case.op == "-n")
    lines = case.texts[0].splitlines(keepends=True)
    return b"".join(lines[i] for i in keep)


def oracle_output(oracle_bin, case, tmpdir):
    paths = []
    for i, t in enumerate(case.texts):
        paths.append(os.path.join(str(tmpdir), f"in{i}.bed"))
        with open(paths[-1], "wb") as f:
            f.write(t)
    return subprocess.run([oracle_bin["bedops"], case.op, *case.args, *paths], stdout=subprocess.PIPE,
                          check=True).stdout


# ------------------------------------------------------------------ the claims, family by family
def claims_a(case, m, k, rows):
    iv, f = k[0], rows[0]
    ks, ke = [s for s, _ in iv], [e for _, e in iv]
    opens = M.openings(iv)
    assert len(f) == m["n"] <= 20000, case.name
    assert sum(opens) == len(M.components(iv)) == m["ncomp"], case.name
    if "seam" in m:
        p, back = m["seam"], m["back"]
        cover = ke[p - back]
        assert cover == max(ke[:p]) and all(e < cover for e in ke[p - back + 1:p]), case.name
        assert ks[p] - cover == dict(S.A_RELS)[m["rel"]], case.name  # the bridged rows straddle p
        assert opens[p - back] and not any(opens[p - back + 1:p]), case.name
        assert opens[p] == (m["rel"] == "short") and opens[p + 1], case.name
        # whose lane, item, wave or tile the maximum comes from
        assert (p - back) // 64 != p // 64, case.name
        if back > 64:
            assert (p - back) // 64 != (p - 1) // 64, case.name
        if back > S.WAVE_ROWS:
            assert (p - back) // S.WAVE_ROWS != (p - 1) // S.WAVE_ROWS, case.name
        if back > S.CT_TILE:
            assert (p - back) // S.CT_TILE != (p - 1) // S.CT_TILE, case.name
    if "closed" in m:
        a, b = m["closed"]
        assert opens[a - 1] and opens[b] and not any(opens[a:b]), case.name
        assert (a - 1) // S.CT_TILE == 0 and (b - 1) // S.CT_TILE == 3, case.name
        assert not any(opens[S.CT_TILE:3 * S.CT_TILE]), case.name  # tiles 1 and 2: zero openings
    if "chrom_at" in m:
        p = m["chrom_at"]
        assert f[p - 1][0] != f[p][0] and f[p - 1][2] == S.COORD_MAX, case.name
        assert ks[p] - ke[p - 1] == 1 and opens[p], case.name
    if "last_chain" in m:
        n, c = m["n"], m["last_chain"]
        assert opens[n - c] and not any(opens[n - c + 1:]), case.name
        lane, item = (n - 1) % 64, (n - 1) % S.WAVE_ROWS // 64
        assert (lane, item) == ((63, S.CT_ITEMS - 1) if n % S.CT_TILE == 0 else (0, 0)), case.name


def claims_b(case, m, k, rows):
    mode = MODE[case.op]
    x, y = k
    assert m["plain"] and M.components(x) == x and M.components(y) == y, case.name
    assert max(len(x), len(y)) <= 20000
    order = M.merge_order(x, y, mode)
    assert len(order) == m["total"], case.name
    for d, (w, idx, row) in m.get("at", {}).items():  # the element named is at the stated d
        assert order[d] == (w, idx) and rows["xy".index(w)][idx] == row, (case.name, d, order[d])
    pieces = M.pieces_by_position(x, y, mode)
    assert [p for _, p in pieces] == (M.intersect2 if mode == "i" else M.difference2)(x, y), case.name
    counts = M.segment_counts(x, y, mode, S.MP_TILE)
    for t in m.get("empty", []):
        assert counts[t] == 0, (case.name, t)
    for t in m.get("full", []):
        assert counts[t] == S.BG_SEG_CAP, (case.name, t, counts[t])  # filled to capacity
    assert max(counts, default=0) <= S.BG_SEG_CAP
    for key, w in (("only_x", "x"), ("only_y", "y")):
        for t in m.get(key, []):
            tile = order[t * S.MP_TILE:(t + 1) * S.MP_TILE]
            assert len(tile) == S.MP_TILE and {e[0] for e in tile} == {w}, (case.name, t)
    if m.get("empty") and case.name.split("-")[-1] in ("first", "mid", "last"):
        assert sum(counts) > 0, case.name


def claims_c(case, m, k, rows):
    comps = [M.components(f) for f in k]
    sizes, acc, ties = [], comps[0], False
    if case.op == "-i":
        for c in comps[1:]:
            sizes.append(len(acc) + len(c))
            acc = M.intersect2(acc, c)
    else:
        acc = comps[0] if case.op == "-m" else comps[1]
        for c in comps[1:] if case.op == "-m" else comps[2:]:
            sizes.append(len(acc) + len(c))
            ties = ties or bool({s for s, _ in acc} & {s for s, _ in c})
            acc = M.components(sorted(acc + c, key=lambda t: t[0]))
        if case.op == "-m":
            assert ties, case.name                                    # equal starts: k_merge_sorted's ties
            assert any(n % S.MP_ITEMS for n in sizes), case.name      # a last partial thread
        else:
            sizes.append(len(comps[0]) + len(acc))
    for c in m["cross"]:
        assert any(n > c for n in sizes), (case.name, sizes)


def claims_d(case, m, k, rows):
    assert len(k[0]) == m["n"], case.name
    comps = M.union_components(k[1:])
    thres, pct = SPEC[case.args[0]]
    keep = set(M.element_of(k[0], comps, thres, pct, case.op == "-n"))
    assert 0 < len(keep) < m["n"], case.name
    if pct and thres == 0.5:  # rows covered to exactly half decide differently a hair above it
        assert keep != set(M.element_of(k[0], comps, 0.5 + 1e-9, 1, case.op == "-n")), case.name
    if "span" in m:
        b = m["block"]
        blo, bhi = M.element_range(k[0][b * S.BG_NT:(b + 1) * S.BG_NT], comps)
        assert bhi - blo == m["span"], (case.name, blo, bhi)
        assert (bhi - blo <= S.EF_SLICE) == (m["span"] == S.EF_SLICE), case.name  # staged / unstaged
        assert m["n"] % S.BG_NT, case.name  # the last block is partly filled
    if "kept" in m:
        assert set(range(*m["kept"])) <= keep and not set(range(*m["dropped"])) & keep, case.name
        assert len(keep) > S.FMT_TILE, case.name  # more than one output format tile
    rests = {len(ln.split(b"\t", 3)[3]) for ln in case.texts[0].splitlines()}
    assert len(rests) > 10, case.name  # remainders of varying length


CLAIMS = {"A": claims_a, "B": claims_b, "C": claims_c, "D": claims_d}


# ------------------------------------------------------------------ tests
def test_constants_match_sources():
    """the geometry the generator places its seams by is the kernels'"""
    assert S.source_constants() == S.CONSTANTS == (8, 512, 2048, 4, 4, 1024, 1024, 256, 1024, 4096, 512)
    assert S.SEAMS == (64, 512, 2048, 8192)


def test_case_names_and_routes():
    names = [c.name for _, fam in S.FAMILIES for c in fam()]
    assert len(set(names)) == len(names) > 150
    for _, fam in S.FAMILIES:
        for c in fam():
            assert c.name[0] in S.ROUTES and len(S.routes(c)) >= 2, c.name
            assert set(S.routes(c)) <= {"set", "rows", "columns"}, c.name
            chroms = []
            for t in c.texts:
                for r in S.rows_of(t):
                    if not chroms or chroms[-1] != r[0]:
                        chroms.append(r[0])
            uniq = sorted(set(chroms), key=lambda s: s.encode())
            assert 1 <= len(uniq) <= 4, c.name
            assert len(uniq) >= 2 or c.name.startswith(("A-n1-", "B")), c.name


@pytest.mark.parametrize("fam", [f for _, f in S.FAMILIES], ids=[n for n, _ in S.FAMILIES])
def test_family_is_as_stated_and_model_matches_oracle(oracle_bin, tmp_path, fam):
    cases = fam()
    assert cases
    for c in cases:
        k, names, rows = keyed(c)
        CLAIMS[c.name[0]](c, S.META[c.name], k, rows)
        want = oracle_output(oracle_bin, c, tmp_path)
        assert model_output(c, k, names) == want, c.name


def test_every_seam_has_its_cases():
    """what the issue lists is there: every count, every seam in every relation, every diagonal"""
    names = {c.name for _, fam in S.FAMILIES for c in fam()}
    for n in S.A_COUNTS:
        assert {f"A-n{n}-disjoint", f"A-n{n}-chained"} <= names
    for p in S.SEAMS:
        for rel, _ in S.A_RELS:
            assert f"A-seam{p}-{rel}" in names and f"A-seam{p}-back2-{rel}" in names
        assert f"A-chromseam{p}" in names
    assert {f"A-seam8192-back{k}-touch" for k in S.A_BACK} <= names
    for op in ("-i", "-d"):
        for n in S.B_TOTALS:
            assert f"B{op}-n{n}" in names
        for d in S.B_TARGETS:
            assert {f"B{op}-xy-d{d}", f"B{op}-yx-d{d}", f"B{op}-tie-d{d}"} <= names
    assert S.B_TARGETS[0] % S.MP_TILE == 0 and S.B_TARGETS[2] % S.MP_TILE and S.B_TARGETS[2] % S.MP_ITEMS == 0
