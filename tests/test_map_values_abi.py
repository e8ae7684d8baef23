"""CPU checks of bg_result_export_map_values' boundary: the header declares it, the library
exports it, the Python mirror binds it; and the numpy model the GPU tests use as one of their two
oracles (map_values_model.model) reproduces what the reference printed, so that it is not only
checked against the code it is there to check."""
import ctypes
import os
import re

from conftest import ROOT

import map_values_model as M

NAME = "bg_result_export_map_values"


def test_header_declares_the_call():
    src = open(os.path.join(ROOT, "include", "bedgpu.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*bg_ctx\s*\*\s*\w+,\s*bg_result\s*\*\s*\w+,\s*int\s+\w+,\s*double\s*\*\s*\w+\s*\)\s*;"
                     % NAME, src)


def test_library_exports_the_call(gpu_bin):
    from bedops_amd.engine import lib_path
    assert hasattr(ctypes.CDLL(lib_path()), NAME)


def test_engine_binds_the_call():
    import bedops_amd.engine as E
    assert NAME in E.SYMBOLS
    assert set(E.EXPORT_MAP_OPS) < set(E.EXPORT_MAP_VALUE_OPS)
    new = {E.MAP_OPS[op] for op in M.NEW_OPS}
    assert set(E.EXPORT_MAP_VALUE_OPS) == set(E.EXPORT_MAP_OPS) | new and len(new) == 10
    assert callable(getattr(E.Result, "values"))
    src = open(os.path.join(ROOT, "bedops_amd", "engine.py")).read()
    assert re.search(r"L\.%s\.argtypes\s*=" % NAME, src)


def test_the_fixtures_hold_what_the_gpu_test_counts_on():
    cases = M.fixture_cases()
    assert len(cases) >= 170
    for op in M.NEW_OPS:
        assert sum(any(o[0] == op for o in p["ops"]) for _, _, p, _, _ in cases) >= 10, op


def test_model_agrees_with_the_reference():
    """the model's domain: --bp-ovr without --faster, two files, no zero-length rows (its
    brute-force members are the sweep's only then)"""
    ran, per_op = 0, {op: 0 for op in M.NEW_OPS + M.OLD_OPS}
    for suite, k, p, texts, cols in M.fixture_cases():
        ref = M.parse_bed(texts[0])
        mp, sc = M.parse_bed(texts[-1], score=True)
        inside = (p["crit"] == "bp-ovr" and not p["faster"] and len(texts) == 2
                  and not any(s == e for _, s, e in ref + mp))
        # (outside it, what does not depend on the members is still the model's to say)
        members = M.brute_bp(ref, mp, p["val"]) if inside else [[]] * len(ref)
        got = M.model(p["ops"], ref, mp, sc, members)
        for q, op in enumerate(p["ops"]):
            if got[q] is None or not (inside or op[0] == "echo-ref-size"):
                continue
            assert M.fmt(op[0], p["prec"], got[q]) == cols[q], (suite, k, op)
            per_op[op[0]] += 1
        ran += inside
    print("model vs reference: %d cases; per operation %s" % (ran, per_op))
    assert ran >= 20, ran
    assert all(per_op[op] >= 3 for op in M.NEW_OPS), sorted(per_op.items())
