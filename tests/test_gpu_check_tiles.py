"""bg_check's parallel form (bedops_amd/csrc/bg_check.hip) on the generated inputs of
tests/ec_cases.py: defects on tile, wave and thread seams, order checks whose previous row
lies in another tile, header blocks longer than a tile, several defects whose file order is
not their code order, every kind of file end, very long fields, more tiles than one level of
the scan holds, runs of newlines, and the base file shifted through every alignment.
Engine.check must give the oracle's bytes (oracle/ec_oracle.c), or None where the oracle
prints nothing; bg_check_result must hold check_main's row and code, the failing line's span
and the span of the line before it. tests/test_ec_cases.py checks the inputs on the CPU."""
import subprocess

import pytest

import ec_cases
import test_check
from test_check import check_bin  # noqa: F401  (fixture)
from test_ec_cases import FAMILIES, Runner, rest_thresholds

pytestmark = pytest.mark.gpu

PASSES = dict(row=0, code=0, line_off=0, line_len=0, prev_off=0, prev_len=0)


@pytest.fixture(scope="module")
def eng():
    from bedops_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def runner(tmp_path_factory, check_bin, oracle_bin, eng):  # noqa: F811
    """the CPU references, with the messages worded by the library the engine has loaded"""
    return Runner(tmp_path_factory.mktemp("ec"), check_bin, eng.L)


def line_span(data, row):
    """(offset, length) of getline's 1-based line `row`, found from the bytes alone"""
    pos = 0
    for _ in range(row - 1):
        pos = data.index(b"\n", pos) + 1
    end = data.find(b"\n", pos)
    return pos, (len(data) if end < 0 else end) - pos


def check_case(eng, runner, c):
    path, want, raw = runner(c)
    got = eng.check(c.data, c.nfields, bool(c.has_rest), name=path, nest=bool(c.nest))
    assert got == (want or None), (c.name, got, want)
    r = eng.check(c.data, c.nfields, bool(c.has_rest), nest=bool(c.nest), raw=True)
    if raw is None:
        assert r == PASSES, (c.name, r)
        return
    assert (r["row"], r["code"]) == raw[:2], (c.name, r, raw)
    assert (r["line_off"], r["line_len"]) == line_span(c.data, r["row"]) == raw[2:], (c.name, r, raw)
    if r["row"] > 1:  # the line before, without its newline
        assert (r["prev_off"], r["prev_len"]) == line_span(c.data, r["row"] - 1), (c.name, r)
    else:
        assert (r["prev_off"], r["prev_len"]) == (0, 0), (c.name, r)


@pytest.mark.parametrize("kind", ec_cases.SEAM_KINDS)
@pytest.mark.parametrize("pi", range(len(ec_cases.A_PARAMS)))
def test_family_a_seam_by_defect_class(eng, runner, pi, kind):
    for c in ec_cases.family_a(pi, kind):
        check_case(eng, runner, c)


@pytest.mark.parametrize("fam", [f for _, f in FAMILIES], ids=[n for n, _ in FAMILIES])
def test_family(eng, runner, fam):
    for c in fam():
        check_case(eng, runner, c)


def test_family_f_long_fields(eng, runner):
    for c in ec_cases.family_f(*rest_thresholds(runner)):
        check_case(eng, runner, c)


def test_family_g_past_first_scan_level(eng, runner):
    for c in ec_cases.family_g():
        check_case(eng, runner, c)


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def test_cli_reports_defects_past_the_first_tile(gpu_bin, oracle_bin, tmp_path):
    """the front-ends word a late tile's defect as the reference does: usage hint, "Error: ",
    the oracle's text, a non-zero exit"""
    ok = _write(tmp_path / "ok.bed", b"chr0\t1\t3\nchr0\t4\t8\n")
    lines = ec_cases.base_lines()
    j = ec_cases.first_line_at(lines, 3 * ec_cases.TILE + 100)
    lines[j] = ec_cases._start_below(lines[j])
    bad = _write(tmp_path / "bad.bed", ec_cases.join(lines))
    nested = {c.name: c for c in ec_cases.family_b(1, 0)}["B-31-short-nested+0"]
    late = {c.name: c for c in ec_cases.family_c()}["C-late1+0"]
    assert ec_cases.META[late.name]["at"] == 2 * ec_cases.TILE
    runs = [("bedops", ["--ec", "-m", ok, bad], bad, (3, 0, 0), j + 1),
            ("bedmap", ["--faster", "--ec", "--count", ok, _write(tmp_path / "map.bed", nested.data)],
             str(tmp_path / "map.bed"), (3, 1, 1), ec_cases.META[nested.name]["row"]),
            ("closest", ["--ec", ok, _write(tmp_path / "late.bed", late.data)],
             str(tmp_path / "late.bed"), (3, 1, 0), ec_cases.META[late.name]["row"])]
    for tool, args, path, (nf, rest, nest), row in runs:
        want = test_check.oracle_text(path, nf, rest, nest)
        assert want.endswith(b"\nSee row: %d" % row), (tool, want)
        r = subprocess.run([gpu_bin[tool]] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        prog = "closest-features" if tool == "closest" else tool
        assert r.returncode != 0, (tool, r.stderr)
        assert r.stderr == f"May use {prog} --help for more help.\n\nError: ".encode() + want + b"\n", tool
