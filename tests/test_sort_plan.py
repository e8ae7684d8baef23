"""The sort plan for unsorted columnar input (bedops_amd/csrc/bg_sortplan.h) on
the CPU: tools/build/sort_plan_check includes the header and prints the plan for given row and
name counts and the largest start and length."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CHECK = os.path.join(ROOT, "tools", "build", "sort_plan_check")


@pytest.fixture(scope="module")
def plan():
    subprocess.run(["make", "-s", "tools/build/sort_plan_check"], cwd=ROOT, check=True)

    def run(n, names, max_start, max_len):
        out = subprocess.run([CHECK, str(n), str(names), str(max_start), str(max_len)], stdout=subprocess.PIPE,
                             check=True).stdout.decode()
        m = re.fullmatch(r"packed=(\d) br=(\d+) bs=(\d+) bl=(\d+) bits=(\d+),(\d+) passes=(\d+),(\d+)\n", out)
        assert m, out
        v = [int(x) for x in m.groups()]
        return {"packed": bool(v[0]), "br": v[1], "bs": v[2], "bl": v[3], "bits": (v[4], v[5]), "passes": (v[6], v[7])}
    return run


def test_header_has_no_hip_in_it():
    src = open(os.path.join(ROOT, "bedops_amd", "csrc", "bg_sortplan.h")).read()
    assert re.findall(r"#include\s+(\S+)", src) == ["<stdint.h>"]
    assert "__global__" not in src and "__device__" not in src


def test_widths(plan):
    p = plan(1000, 70, (1 << 28) - 1, (1 << 16) - 1)
    assert (p["br"], p["bs"], p["bl"]) == (7, 28, 16)
    assert p["packed"] and p["bits"] == (51, 0) and p["passes"] == (7, 0)
    assert plan(1000, 2, 1 << 28, 1 << 16)["bits"] == (1 + 29 + 17, 0)
    assert plan(1000, 3, 0, 0)["br"] == 2 and plan(1000, 4, 0, 0)["br"] == 2 and plan(1000, 5, 0, 0)["br"] == 3


def test_boundary_between_the_packed_key_and_two_rounds(plan):
    top = (1 << 40) - 1
    p = plan(1000, 16, top, (1 << 20) - 1)  # 4 + 40 + 20 = 64
    assert p["packed"] and p["bits"] == (64, 0) and p["passes"] == (8, 0)
    p = plan(1000, 17, top, (1 << 20) - 1)  # 5 + 40 + 20 = 65
    assert not p["packed"] and p["bits"] == (20, 45) and p["passes"] == (3, 6)
    p = plan(1000, 16, top, 1 << 20)  # 4 + 40 + 21 = 65
    assert not p["packed"] and p["bits"] == (21, 44) and p["passes"] == (3, 6)
    # the widest input there is: 2^22 - 1 names, every coordinate bit
    p = plan(1000, (1 << 22) - 1, top - 1, top)
    assert not p["packed"] and p["bits"] == (40, 62) and p["passes"] == (5, 8)


@pytest.mark.parametrize("bits,passes", [(1, 1), (8, 1), (9, 2), (16, 2), (17, 3), (64, 8)])
def test_pass_counts(plan, bits, passes):
    # one name: the key is start << bl | len
    bs = min(bits, 40)
    bl = bits - bs
    p = plan(1000, 1, (1 << bs) - 1, (1 << bl) - 1 if bl else 0)
    assert p["packed"] and p["br"] == 0 and p["bits"] == (bits, 0) and p["passes"] == (passes, 0)


def test_one_name(plan):
    top = (1 << 40) - 1
    p = plan(5, 1, top, (1 << 24) - 1)  # br = 0: 40 + 24 bits still pack
    assert p["packed"] and p["br"] == 0 and p["bits"] == (64, 0)
    p = plan(5, 1, top, top)  # 80 bits do not
    assert not p["packed"] and p["bits"] == (40, 40) and p["passes"] == (5, 5)
    p = plan(5, 1, 0, 0)  # nothing to tell rows apart by: no pass
    assert p["packed"] and p["bits"] == (0, 0) and p["passes"] == (0, 0)


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_rows_need_no_pass(plan, n):
    for names, ms, ml in ((0, 0, 0), (70, (1 << 28) - 1, 99), (3000, (1 << 40) - 2, 1 << 39)):
        assert plan(n, names, ms, ml)["passes"] == (0, 0)
    assert plan(2, 70, (1 << 28) - 1, 99)["passes"] == (6, 0)
