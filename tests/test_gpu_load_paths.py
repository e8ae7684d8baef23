"""bg_load's recovery ladder (bedops_amd/csrc/bg_load.hip), path by path: a BG_BED3_SET input
whose staging overflows is loaded again as rows, short lines send a row load to the wide
parser, blank lines are stripped and the load redone with the inputs' own kinds. Each case
asserts the oracle's bytes AND the kernels the load launched, counted by the library's
profiling (tests/kernel_paths.py) under the names of the BG_LAUNCH sites:
  k_parse_set   k_parse_set_v, the set parse
  k_parse       k_parse_rv, the row parse
  k_parse_wide  k_parse, the row parse of a load redone for short lines
  k_blank_marks / k_blank_pack   strip_blank_lines
The clean case is the control: a set load that needs no recovery launches no row parser."""
import random
import tempfile

import pytest

import kernel_paths
import randbed
from test_gpu_parity import run_oracle

pytestmark = pytest.mark.gpu

ROW_PARSERS = ("k_parse", "k_parse_wide")
BG_E_ARG = -6


@pytest.fixture(scope="module")
def eng():
    from bedops_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _set_texts(seed=5):
    """two sorted one-chromosome inputs of 3000 rows (six 8 KiB tiles each): between the first
    and the last tile no tile holds a chromosome change, so the loader's scan for chromosome
    runs (k_tile_runs, boundary tiles only) reads none of their lines"""
    rng = random.Random(seed)
    return [randbed.text(randbed.rows(rng, 3000, chroms=["chr1"], span=400_000, maxlen=60)).encode()
            for _ in range(2)]


def _intersect(eng, oracle_bin, texts):
    """bedops -i through the set loader: (launches, output == oracle's)"""
    with tempfile.TemporaryDirectory() as td:
        want = run_oracle(oracle_bin["bedops"], ["-i"], texts, td)
    got, k = kernel_paths.launches(eng, lambda: eng.bedops("-i", texts))
    print(k)
    return k, got == want


def _order(k, first, then):
    names = list(k)  # first-launch order
    return names.index(first) < names.index(then)


def test_clean_set_inputs_launch_no_row_parser(eng, oracle_bin):
    k, same = _intersect(eng, oracle_bin, _set_texts())
    assert same
    assert k.get("k_parse_set", 0) == 2
    assert not any(n in k for n in ROW_PARSERS)
    assert "k_blank_marks" not in k and "k_blank_pack" not in k


def test_staging_overflow_reloads_as_rows(eng, oracle_bin):
    """the inputs of test_gpu_setload.py::test_set_load_staging_overflow_falls_back"""
    a = "".join(f"c\t{3 * i}\t{3 * i + 1}\n" for i in range(30000)).encode()
    b = "".join(f"c\t{5 * i}\t{5 * i + 3}\n" for i in range(18000)).encode()
    k, same = _intersect(eng, oracle_bin, [a, b])
    assert same
    assert k.get("k_parse_set", 0) == 2  # the first attempt, both inputs
    rows = [n for n in ROW_PARSERS if n in k]
    assert rows and sum(k[n] for n in rows) >= 2  # the redo parses both inputs as rows
    assert all(_order(k, "k_parse_set", n) for n in rows)


def test_short_lines_reach_the_wide_parser(eng, oracle_bin):
    """the inputs of test_gpu_rowload.py::test_short_lines_redo_with_the_wide_parser: 8-9 byte
    lines stay under the 512 lines a 4 KiB sub-tile of k_parse_rv holds (the control), 6-byte
    lines pass it and the whole load is redone with the wide parser"""
    rows = "".join(f"c\t{i}\t{i + 1}\n" for i in range(3000)).encode()
    tiny = "".join(f"c\t{i % 10}\t{i % 10 + 1}\n" for i in range(3000))
    tiny = "".join(sorted(tiny.splitlines(keepends=True),
                          key=lambda s: (int(s.split()[1]), int(s.split()[2])))).encode()
    with tempfile.TemporaryDirectory() as td:
        for ref, redo in ((rows, False), (tiny, True)):
            want = run_oracle(oracle_bin["bedmap"], ["--echo", "--count"], [ref, rows], td)
            got, k = kernel_paths.launches(eng, lambda: eng.bedmap(["echo", "count"], ref, rows))
            print(k)
            assert got == want
            assert k.get("k_parse", 0) == 2  # the first attempt: k_parse_rv on both inputs
            assert k.get("k_parse_wide", 0) == (2 if redo else 0)  # the redo, both inputs
            if redo:
                assert _order(k, "k_parse", "k_parse_wide")


TT = 8192  # bg_load.hip: the loader's tile


def _with_blank(text, where):
    lines = text.splitlines(keepends=True)
    if where == "trailing":
        return text + b"\n"
    pos = sum(len(ln) for ln in lines[:1500])
    # inside a tile that is neither the first nor the last, and not at its start: only the
    # parse itself meets this line
    assert pos % TT != 0 and 0 < pos // TT < (len(text) - 1) // TT
    return b"".join(lines[:1500]) + (b"\n" if where == "mid_tile" else b" \t\n") + b"".join(lines[1500:])


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("where", ["mid_tile", "mid_tile_spaces", "trailing"])
def test_blank_line_in_a_set_input_keeps_the_set_load(eng, oracle_bin, where, which):
    """a blank line is stripped and the input loaded again as a set: it must not demote the
    call's set inputs to rows (that moved the headline path off k_parse_set_v)"""
    from bedops_amd import BedgpuError
    from bedops_amd.engine import BED3_SET
    texts = _set_texts()
    texts[which] = _with_blank(texts[which], where)
    k, same = _intersect(eng, oracle_bin, texts)
    assert same
    assert not any(n in k for n in ROW_PARSERS), k
    # the last parse of both inputs is the set parse. A blank line inside a middle tile is met
    # by the first load's parse (both inputs parsed twice); a trailing one by the scan for
    # chromosome runs in the last tile, before any parse
    assert k.get("k_parse_set", 0) == (2 if where == "trailing" else 4), k
    s = eng.load([(t, BED3_SET) for t in texts])
    try:
        assert s.rows(0) == 3000 and s.rows(1) == 3000
        with pytest.raises(BedgpuError) as ei:  # (how test_set_tables_refuse_row_operations
            eng.op("-p", s, [0, 1])             # recognises a set table)
        assert ei.value.code == BG_E_ARG
    finally:
        s.free()
    assert k.get("k_blank_marks", 0) >= 1 and k.get("k_blank_pack", 0) >= 1, k


def _outcome(eng, text, set_load):
    from bedops_amd import BedgpuError
    try:
        return ("ok", eng.bedops("-m", [text], set_load=set_load))
    except BedgpuError as e:
        return ("err", e.code, e.msg)


@pytest.mark.parametrize("order", ["blank_first", "error_first"])
def test_blank_line_and_a_real_error_report_the_row_loaders_error(eng, order):
    rs = randbed.rows(random.Random(12), 3000, chroms=["chr1"], span=10**6, maxlen=40)
    lines = randbed.text(rs).encode().splitlines(keepends=True)
    first, second = (b"\n", b"chr1\t10\t5\n") if order == "blank_first" else (b"chr1\t10\t5\n", b"\n")
    text = b"".join(lines[:1000]) + first + b"".join(lines[1000:2000]) + second + b"".join(lines[2000:])
    got = _outcome(eng, text, True)
    assert got[0] == "err" and "data line" in got[2], got
    assert got == _outcome(eng, text, False)
