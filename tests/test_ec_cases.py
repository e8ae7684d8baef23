"""The generated --ec inputs of tests/ec_cases.py on the CPU: on every case the oracle
(oracle/ec_oracle.c) and the GPU grammar compiled for the host (tests/cpu/check_main.cpp +
bg_check_message) give the same text, and the inputs are what the generator says they are: the
stated first failure on the stated line at the stated offset, clean variants that pass, defects
of every code on lines that start past the first tile, and in family D an earlier line with the
larger code. tests/test_gpu_check_tiles.py runs bg_check itself on the same cases."""
import os

import pytest

import ec_cases
import test_check
from test_check import check_bin, lib  # noqa: F401  (fixtures)

CODES = ec_cases.codes()
NAMES = {v: k for k, v in CODES.items()}
MIB = 1 << 20


class Runner:
    """writes a case to a file and asks both CPU references about it"""

    def __init__(self, tmpdir, check_bin, lib):
        self.dir, self.check_bin, self.lib = str(tmpdir), check_bin, lib

    def __call__(self, case):
        """-> (path, the oracle's text, check_main's (row, code, offset, length) or None);
        asserts that the two agree and that the case is what the generator's META says"""
        path = os.path.join(self.dir, case.name + ".bed")
        with open(path, "wb") as f:
            f.write(case.data)
        want = test_check.oracle_text(path, case.nfields, case.has_rest, case.nest)
        raw = test_check.gpu_grammar_raw(self.check_bin, path, case.nfields, case.has_rest, case.nest)
        got = test_check.raw_text(self.lib, path, case.data, raw, case.nfields, case.has_rest)
        os.unlink(path)
        assert got == want, case.name
        m = ec_cases.META[case.name]
        if "expect" in m:
            if m["expect"] is None:
                assert want == b"" and raw is None, (case.name, want)
            else:
                assert raw is not None and NAMES[raw[1]] == m["expect"], (case.name, raw)
                assert "row" not in m or raw[0] == m["row"], (case.name, raw, m)
                assert "at" not in m or raw[2] == m["at"], (case.name, raw, m)
        return path, want, raw


@pytest.fixture(scope="module")
def runner(tmp_path_factory, check_bin, lib):  # noqa: F811
    return Runner(tmp_path_factory.mktemp("ec"), check_bin, lib)


def rest_thresholds(run):
    """the smallest n at which the oracle rejects ec_cases.rest_line(n, nf), for nf = 5 and 3:
    within 2 bytes of 1 MiB (with 5 fields the reference's marker has stepped one byte past the
    tab after the score, BedCheckIterator.hpp:568-573, so it is not MAXRESTSIZE + 1)"""
    out = []
    for nf in (5, 3):
        says = {n: run(ec_cases.rest_probe(n, nf))[1] for n in range(MIB - 3, MIB + 5)}
        bad = sorted(n for n, text in says.items() if text)
        assert bad and bad == list(range(bad[0], MIB + 5)), bad  # one threshold inside the window
        assert all(b"cannot fit into MAXRESTSIZE chars" in says[n] for n in bad)
        assert abs(bad[0] - MIB) <= 2, bad[0]
        out.append(bad[0])
    return out


def test_constants_match_sources():
    """the geometry the generator places its seams by is the kernels'"""
    assert ec_cases.source_constants() == (ec_cases.TILE, ec_cases.THREAD_BYTES, ec_cases.WAVE_BYTES,
                                           ec_cases.SCAN_TILE) == (8192, 32, 2048, 1024)
    assert CODES["BGC_EMPTY"] == 10 and CODES["BGC_NESTED"] == max(CODES.values()) < 256


def test_placement_helper():
    lines = ec_cases.base_lines()
    assert abs(ec_cases.offset_of(lines, len(lines)) - ec_cases.BASE_BYTES) < 100
    assert len({l.split(b"\t")[0] for l in lines}) == 3
    for at in (8191, 8192, 8193, 30000):
        i = ec_cases.first_line_at(lines, at)
        placed = ec_cases.place(lines, i, at + 40)
        data = ec_cases.join(placed)
        assert data[at + 40 - 1:at + 40] == b"\n" and data[at + 40:].startswith(lines[i] + b"\n")


# (family A: the population test below runs it, and asserts the same per case)
FAMILIES = ([(f"B{pi}{lp}", lambda pi=pi, lp=lp: ec_cases.family_b(pi, lp))
             for pi in range(len(ec_cases.B_PARAMS)) for lp in (0, 1)] +
            [("C", ec_cases.family_c), ("D", ec_cases.family_d), ("E", ec_cases.family_e),
             ("H", ec_cases.family_h), ("sweep", ec_cases.sweep)])


@pytest.mark.parametrize("fam", [f for _, f in FAMILIES], ids=[n for n, _ in FAMILIES])
def test_family_matches_oracle(runner, fam):
    cases = fam()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        runner(c)


def test_family_f_long_fields(runner):
    t5, t3 = rest_thresholds(runner)
    assert (t5, t3) == (MIB + 2, MIB + 1)
    for c in ec_cases.family_f(t5, t3):
        runner(c)


def test_family_g_past_first_scan_level(runner):
    for c in ec_cases.family_g():
        runner(c)


def _codes_of_test_check(runner):
    """every code check_main emits on the inputs of tests/test_check.py"""
    seen = set()

    def note(data, nf, rest, nest=0):
        raw = runner(ec_cases.Case("tc", data, nf, rest, nest))[2]
        if raw:
            seen.add(NAMES[raw[1]])

    ec_cases.META["tc"] = {}
    for nf, rest, cases in test_check.GRAMMAR_PARAMS:
        for data in cases:
            note(data, nf, rest)
    for data, _, _ in test_check.NEST_CASES:
        for rest in (0, 1):
            note(data, 3, rest, 1)
    for _, data in test_check.mutation_files():
        for nf, rest in test_check.MUTATION_PARAMS:
            note(data, nf, rest)
    return seen


def test_population_every_code_past_the_first_tile(runner):
    """Population condition: every BGC_* code that check_main emits anywhere in
    tests/test_check.py also fails a family-A or family-B case on a line that starts at byte
    >= 8192, placed there by the generator (META "at"). No code had to be left out. (Of the
    codes test_check.py never emits, BGC_ID_LONG and BGC_REST_LONG start past the first tile in
    family F; BGC_S_MAX and BGC_E_MAX cannot be emitted at all: a number of at most
    MAX_DEC_INTEGERS = 12 digits never exceeds MAX_COORD_VALUE.)"""
    placed = set()
    for pi in range(len(ec_cases.A_PARAMS)):
        for kind in ec_cases.SEAM_KINDS:
            cases = ec_cases.family_a(pi, kind)
            assert len({c.name for c in cases}) == len(cases)
            hits = {}  # inserted file at one offset -> how often its failing line sat on the seam
            for c in cases:
                raw = runner(c)[2]
                m = ec_cases.META[c.name]
                if raw is None:
                    continue
                assert "at" in m and abs(raw[2] - m["at"]) < 200, (c.name, raw)  # never a base row
                group = c.name.rsplit("l", 1)[0]
                hits.setdefault(group, 0)
                if raw[2] == m["at"]:
                    hits[group] += 1
                    if raw[2] >= ec_cases.TILE:  # (S-1 of the first seam is the last byte of tile 0)
                        placed.add(NAMES[raw[1]])
            # (one variant per line of the inserted file: the failing line is on the seam in one)
            assert hits and set(hits.values()) == {1}, [g for g, n in hits.items() if n != 1]
    for pi in range(len(ec_cases.B_PARAMS)):
        for lp in (0, 1):
            for c in ec_cases.family_b(pi, lp):
                raw = runner(c)[2]
                if raw and raw[2] == ec_cases.META[c.name]["at"] and raw[2] >= ec_cases.TILE:
                    placed.add(NAMES[raw[1]])
    want = _codes_of_test_check(runner)
    assert {"BGC_EMPTY", "BGC_M_CHAR", "BGC_UNSORTED_REST", "BGC_HEADER_LATE", "BGC_NESTED"} <= want
    print("codes on seams:", len(placed), "of", len(CODES) - 2, "; never placed:",
          sorted(set(CODES) - placed - {"BGC_OK", "BGC_HEADER"}))
    assert want - placed == set(), sorted(want - placed)


def test_family_d_earlier_line_larger_code(runner):
    """in each case with several defects the reported line is the smallest one and its code is
    larger than a later defect's; each later defect is reported once the earlier are left out"""
    many = 0
    for c in ec_cases.family_d():
        raw = runner(c)[2]
        d = ec_cases.META[c.name].get("defects")
        if not d:
            continue
        assert (raw[0], NAMES[raw[1]]) == d[0], (c.name, raw)
        if len(d) > 1:
            many += 1
            assert all(d[0][0] < row for row, _ in d[1:])
            assert CODES[d[0][1]] > min(CODES[name] for _, name in d[1:]), c.name
            assert CODES[d[0][1]] > CODES[d[-1][1]], c.name
    assert many >= 7
