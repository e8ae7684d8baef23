"""The sweep kernels of bedops_amd/csrc/bg_setops.hip on the generated inputs of
tests/setop_cases.py: rows and components on the seams of k_components' items, waves and tiles
and of k_tile_max's workgroups, overlapping pairs split by the diagonals and thread seams of the
merge-path tiles, tiles that hold one input only, full and empty segments, printed widths that
change between segments, folds over three and four files, and element-of blocks around the LDS
slice and the format tiles. On every case the GPU must give the oracle's bytes
(oracle/bedops_oracle.c), on every route the case's family lists (setop_cases.ROUTES): text
parsed straight to sets, text kept as rows, and numeric columns, the last compared both as
exported columns and as the formatted text of the same result. tests/test_setop_cases.py
proves on the CPU that the inputs are where this says."""
import os
import subprocess

import numpy as np
import pytest
import torch

import setop_cases as S
from kernel_paths import launches

pytestmark = pytest.mark.gpu

# torch's HIP runtime has to start before libbedgpu opens the device; in a
# whole-suite run other modules open engines before this module's tests run, so it is started
# when the module is collected, as tests/test_gpu_columns.py does
if torch.cuda.is_available():
    torch.cuda.init()

BED3 = 0
ARG = -6


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


def oracle(oracle_bin, case, tmpdir):
    paths = []
    for i, t in enumerate(case.texts):
        paths.append(os.path.join(str(tmpdir), f"in{i}.bed"))
        with open(paths[-1], "wb") as f:
            f.write(t)
    return subprocess.run([oracle_bin["bedops"], case.op, *case.args, *paths], stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, check=True).stdout


def col_input(data, device):
    """BED text -> (names, chrom, start, end, BED3); names in an order that is not strcmp's"""
    rows = S.rows_of(data)
    names = sorted({r[0] for r in rows}, key=lambda s: s.encode())[::-1]
    idx = {nm: k for k, nm in enumerate(names)}
    cols = [torch.as_tensor(np.array([idx[r[0]] for r in rows], dtype=np.int32)),
            torch.as_tensor(np.array([r[1] for r in rows], dtype=np.int64)),
            torch.as_tensor(np.array([r[2] for r in rows], dtype=np.int64))]
    if device:
        cols = [c.to("cuda:0") for c in cols]
    return (names, *cols, BED3)


def ivl_text(names, cols):
    c, s, e = (cols[k].cpu().numpy() for k in ("chrom", "start", "end"))
    return "".join(f"{names[c[i]]}\t{s[i]}\t{e[i]}\n" for i in range(len(c))).encode()


def spec_of(case):
    return case.args[0] if case.args else None


def run_text(eng, case, route):
    return eng.bedops(case.op, case.texts, spec=spec_of(case), set_load=(route == "set"))


def run_columns(eng, case, want, export_first):
    """the case through Engine.load_columns: the exported columns and the formatted text of one
    result, in either order; element-of: the exported rows select the oracle's lines"""
    from bedops_amd import BedgpuError
    s = eng.load_columns([col_input(t, device=(i != 1)) for i, t in enumerate(case.texts)])
    try:
        r = eng.op(case.op, s, list(range(len(case.texts))), spec_of(case))
        try:
            if case.op in ("-e", "-n"):
                rows = r.columns()["rows"].cpu().tolist()
                lines = case.texts[0].splitlines(keepends=True)
                assert b"".join(lines[i] for i in rows) == want, (case.name, "columns: rows")
                with pytest.raises(BedgpuError) as ei:  # (a column table has no text to print)
                    r.text()
                assert ei.value.code == ARG
                return
            if export_first:
                cols, text = r.columns(), r.text()
            else:
                text, cols = r.text(), r.columns()
            assert text == want, (case.name, "columns: text", export_first)
            assert ivl_text(s.chroms(), cols) == want, (case.name, "columns: columns", export_first)
        finally:
            r.free()
    finally:
        s.free()


def check_case(eng, oracle_bin, tmpdir, case, k):
    want = oracle(oracle_bin, case, tmpdir)
    ran = []
    for route in S.routes(case):
        if route == "columns":
            run_columns(eng, case, want, export_first=(k % 2 == 0))
        else:
            assert run_text(eng, case, route) == want, (case.name, route)
        ran.append(route)
    assert len(ran) >= 2, case.name
    return want


@pytest.mark.parametrize("fam", [f for _, f in S.FAMILIES], ids=[n for n, _ in S.FAMILIES])
def test_family_vs_oracle(eng, oracle_bin, tmp_path, fam):
    base = eng.live()
    cases = fam()
    produced = 0
    for k, c in enumerate(cases):
        produced += len(check_case(eng, oracle_bin, tmp_path, c, k))
    assert cases and produced > 0
    assert eng.live() == base


def _named(fam, name):
    return {c.name: c for c in fam()}[name]


def test_the_kernels_meant_are_launched(eng):
    """once per family: the route that is meant to reach a kernel does reach it"""
    a = _named(S.family_a_seams, "A-seam8192-back2100-touch")
    _, ks = launches(eng, lambda: run_text(eng, a, "rows"))
    assert ks.get("k_tile_max") == 1 and ks.get("k_components_count") == 1, ks
    assert ks.get("k_components_write") == 1, ks
    _, ks = launches(eng, lambda: run_text(eng, a, "set"))
    assert "k_components_write" not in ks, ks  # (parsed straight to its components)

    folds = {c.name: c for c in S.family_c()}
    _, ks = launches(eng, lambda: run_text(eng, folds["C-i-4files"], "set"))
    assert ks.get("k_intersect_count") == 2 and ks.get("k_intersect_write") == 3, ks
    _, ks = launches(eng, lambda: run_text(eng, folds["C-m-4files"], "set"))
    assert ks.get("k_merge_sorted") == 3, ks
    # (bg_difference leaves its result segmented, which has no count pass: k_difference_count
    # is never launched; the union of the other files goes through k_merge_sorted)
    _, ks = launches(eng, lambda: run_text(eng, folds["C-d-4files"], "set"))
    assert ks.get("k_difference_write") == 1 and ks.get("k_merge_sorted") == 2, ks
    assert "k_difference_count" not in ks, ks

    for op in ("-i", "-d"):  # an export of a segmented result
        b = _named(lambda: S.family_b(op), f"B{op}-widths")
        s = eng.load_columns([col_input(t, True) for t in b.texts])
        try:
            r = eng.op(op, s, [0, 1])
            try:
                _, ks = launches(eng, r.columns)
                assert ks.get("k_seg_compact") == 1, (op, ks)
            finally:
                r.free()
        finally:
            s.free()

    d = _named(S.family_d, "D-e-span1025-50%")
    for route in ("set", "rows"):
        _, ks = launches(eng, lambda: run_text(eng, d, route))
        assert ks.get("k_element_lo") == 1 and ks.get("k_element_flags") == 1, ks
        assert ks.get("k_compact_rows_bytes") == 1, ks
        assert ("k_components_write" in ks) == (route == "rows"), ks
