"""Inputs designed to drive bg_closest (bedops_amd/csrc/bg_closest.hip) down each of its recovery
paths, checked on the CPU: every design goes through the model of the speculation
(tests/model_closest_chunks.py, with the constants bg_closest.hip defines) and must take the
path it is named for; the model's scan must print what the control-flow oracle prints.
tests/test_gpu_closest_paths.py runs the same designs on the GPU and compares the kernels it
launched with what the model says here. A design that stops reaching its path after a retuning
fails here first: re-derive it from the model (its sizes scale with CAP0, CBACK and
CQ_DEF x FIX_ROUNDS), do not weaken the assertion."""
import random
import subprocess
import zlib
from collections import namedtuple

import pytest

import model_closest_chunks as MC
import model_closest_seq as M
import randbed

Design = namedtuple("Design", "name q c Q C")  # texts (bytes) and (chrom id, start, end) rows
NAMES = ["chr1", "chr2"]


def _text(rows, tag):
    return "".join(f"{NAMES[g]}\t{s}\t{e}\t{tag}{i}\n" for i, (g, s, e) in enumerate(rows)).encode()


def _design(name, Q, C):
    assert Q == sorted(Q) and C == sorted(C)
    return Design(name, _text(Q, "q"), _text(C, "c"), Q, C)


def stair(n, nref=100):
    """n nested candidates (i, 100000 - i), every one of them still open at each of the ref rows
    to their right: the reader cache holds all n"""
    C = [(0, i, 100000 - i) for i in range(n)]
    Q = [(0, n + 10 + 3 * j, n + 12 + 3 * j) for j in range(nref)]
    return Q, C


def stair_two_chroms():
    """the deep cache of stair300 met by ref rows of the next chromosome: every cached row is
    popped and dropped as an earlier chromosome's"""
    Q, C = stair(300)
    Q = Q + [(1, 100 + 50 * j, 120 + 50 * j) for j in range(30)]
    C = C + [(1, 90, 95), (1, 130, 400), (1, 700, 710), (1, 1500, 1600)]
    return Q, C


def clamp():
    """one candidate over everything (so lmax reaches back to the file's start) and 9000 short
    ones; 440 ref rows past the first CBACK candidates: every chunk but the first starts with
    its look-back clamped and has not read the long candidate"""
    C = [(0, 0, 90050)] + [(0, 10 * i + 1, 10 * i + 4) for i in range(9000)]
    Q = [(0, 10 * i + 6, 10 * i + 8) for i in (4300 + (j * 4700) // 440 for j in range(440))]
    return Q, C


def grow(gap, nshort, ref_from, nref=440):
    """clamp's short candidates with a nested one (10 i, 1000000 - 10 i) before every gap-th:
    the true cache grows by one row per gap shorts passed, while a clamped start has read only
    the CBACK / gap nested rows of its look-back. So the first attempt at CAP0 overflows nowhere
    in k_closest_chunks (chunk 0 is still shallow, the others start too shallow), every clamped
    start is wrong, and the overflow is met by whatever repairs the chunk in which the true
    cache passes CAP0: a fix round when that is one of the first FIX_ROUNDS chunks, else the
    in-order pass"""
    C = []
    for i in range(nshort):
        if i % gap == 0:
            C.append((0, 10 * i, 1000000 - 10 * i))
        C.append((0, 10 * i + 1, 10 * i + 4))
    Q = [(0, 10 * i + 6, 10 * i + 8)
         for i in (ref_from + (j * (nshort - ref_from - 1)) // nref for j in range(nref))]
    return Q, C


def random_case(shape, args):
    """the inputs of tests/test_gpu_parity.py::test_random_closest_vs_oracle for (shape, args)"""
    rng = random.Random(zlib.crc32(repr((shape, args)).encode()))
    nq, nc, span, ml, zf = {"sparse": (3000, 400, 200000, 100, 0.0),
                            "dense": (2000, 20000, 50000, 60, 0.0),
                            "nested": (3000, 3000, 100000, 3000, 0.0),
                            "zero": (2500, 2500, 10000, 80, 0.1)}[shape]
    qr = randbed.rows(rng, nq, span=span, maxlen=ml, zero_frac=zf)
    q = randbed.text(qr, rest="cols", rng=rng)
    cr = randbed.rows(rng, nc, span=span, maxlen=ml, zero_frac=zf)
    c = randbed.text(cr, rest="cols", rng=rng)
    gid = {nm: g for g, nm in enumerate(sorted(randbed.CHROMS, key=lambda s: s.encode()))}
    ids = lambda rs: [(gid[ch], s, e) for ch, s, e in rs]
    return Design(shape, q.encode(), c.encode(), ids(qr), ids(cr))


_BUILDERS = {"stair300": lambda: _design("stair300", *stair(300)),
             "stair1200": lambda: _design("stair1200", *stair(1200)),
             "stair_two_chroms": lambda: _design("stair_two_chroms", *stair_two_chroms()),
             "clamp": lambda: _design("clamp", *clamp()),
             "grow_fix": lambda: _design("grow_fix", *grow(20, 9000, 4300)),
             "grow_serial": lambda: _design("grow_serial", *grow(40, 13000, 7400)),
             "nested": lambda: random_case("nested", []),
             "sparse": lambda: random_case("sparse", [])}
_designs, _paths = {}, {}


def design(name):
    if name not in _designs:
        _designs[name] = _BUILDERS[name]()
    return _designs[name]


def paths(name, overlaps):
    """the model's result for a design, computed once and shared by the tests"""
    if (name, overlaps) not in _paths:
        d = design(name)
        _paths[name, overlaps] = MC.simulate(d.Q, d.C, overlaps)
    return _paths[name, overlaps]


# (design, overlaps) whose path is asserted below
CASES = [("stair300", True), ("stair300", False), ("stair1200", False), ("stair_two_chroms", True),
         ("stair_two_chroms", False), ("clamp", True), ("clamp", False), ("grow_fix", True),
         ("grow_serial", True), ("nested", True), ("sparse", True)]


# (design, closest-features options) of tests/test_gpu_closest_paths.py. The random shapes are
# pinned for the inputs of their [] case only: test_random_closest_vs_oracle seeds per option set
GPU_OPTS = [[], ["--closest", "--dist"], ["--no-overlaps"]]
GPU_CASES = [(name, args) for name in _BUILDERS for args in GPU_OPTS
             if not (name in ("nested", "sparse") and "--no-overlaps" in args)]


def _passes_for(depth):
    n, cap = 1, MC.K["CAP0"]
    while depth > cap:
        n, cap = n + 1, cap * 4
    return n


def test_constants_are_read_from_the_kernel_source():
    assert set(MC.K) == {"CQ_DEF", "CW_DEF", "CBACK", "CAP0", "FIX_ROUNDS"}
    assert all(v > 0 for v in MC.K.values())


@pytest.mark.parametrize("name,overlaps", CASES)
def test_chunk_model_ends_at_the_sequential_answer(name, overlaps):
    """whatever the speculation did, the check / fix / serial ladder of the model leaves the
    in-order scan's (left, right)"""
    d = design(name)
    want, _ = M.run_seq(d.Q, d.C, overlaps)
    assert paths(name, overlaps).out == want


@pytest.mark.parametrize("name,overlaps", CASES + [("zero", True), ("zero", False)])
def test_model_scan_matches_oracle(oracle_bin, tmp_path, name, overlaps):
    d = design(name) if name in _BUILDERS else random_case(name, [])
    q, c = tmp_path / "q.bed", tmp_path / "c.bed"
    q.write_bytes(d.q)
    c.write_bytes(d.c)
    args = [] if overlaps else ["--no-overlaps"]
    out = subprocess.run([oracle_bin["closest"], "--no-ref", *args, str(q), str(c)],
                         stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    lines = d.c.decode().splitlines()
    res, _ = M.run_seq(d.Q, d.C, overlaps)
    want = ["|".join(lines[x] if x >= 0 else "NA" for x in lr) for lr in res]
    assert out == want


@pytest.mark.parametrize("overlaps", [True, False])
def test_stair300_needs_a_second_capacity_pass(overlaps):
    p = paths("stair300", overlaps)
    assert MC.K["CAP0"] < p.cache_depth <= 4 * MC.K["CAP0"]
    assert p.cache_depth == 300
    assert p.passes == 2


def test_stair1200_needs_three_capacity_passes():
    p = paths("stair1200", False)
    assert 4 * MC.K["CAP0"] < p.cache_depth <= 16 * MC.K["CAP0"]
    assert p.cache_depth == 1200
    assert p.passes == 3


@pytest.mark.parametrize("overlaps", [True, False])
def test_stair_two_chroms_drops_a_deep_cache_at_the_chromosome_change(overlaps):
    d = design("stair_two_chroms")
    p = paths("stair_two_chroms", overlaps)
    assert p.cache_depth > MC.K["CAP0"]
    assert p.passes == _passes_for(p.cache_depth) == 2
    # the cache is deep at the last row of the first chromosome and holds none of its rows
    # after the first row of the second
    _, states = M.run_seq(d.Q, d.C, overlaps)
    last1 = max(i for i, b in enumerate(d.Q) if b[0] == 0)
    assert len(states[last1][1]) > MC.K["CAP0"]
    assert all(d.C[x][0] == 1 for x in states[last1 + 1][1])


def test_clamp_serial_every_clamped_start_is_wrong():
    d = design("clamp")
    p = paths("clamp", True)
    nchunks = -(-len(d.Q) // MC.K["CQ_DEF"])
    assert p.clamped == nchunks - 1 >= MC.K["FIX_ROUNDS"] + 2
    assert p.passes == 1
    # one chunk is repaired per round (its predecessor must be exact first), so the rounds run
    # out and the in-order pass takes over
    assert p.fix_rounds == [MC.K["FIX_ROUNDS"]]
    assert p.serial == [True]


def test_clamp_benign_clamped_starts_are_the_true_state():
    d = design("clamp")
    p = paths("clamp", False)
    assert p.clamped == -(-len(d.Q) // MC.K["CQ_DEF"]) - 1
    assert p.passes == 1
    assert p.fix_rounds == [0]
    assert p.serial == [False]


def test_grow_fix_overflows_in_a_fix_round():
    p = paths("grow_fix", True)
    assert p.clamped == -(-440 // MC.K["CQ_DEF"]) - 1
    assert MC.K["CAP0"] < p.cache_depth <= 4 * MC.K["CAP0"]
    assert p.passes == 2
    # the first attempt is abandoned in a fix round, the second goes all the way
    assert 1 <= p.fix_rounds[0] < MC.K["FIX_ROUNDS"] and p.serial[0] is False
    assert p.fix_rounds[1] == MC.K["FIX_ROUNDS"] and p.serial[1] is True


def test_grow_serial_overflows_in_the_serial_pass():
    p = paths("grow_serial", True)
    assert p.clamped == -(-440 // MC.K["CQ_DEF"]) - 1
    assert MC.K["CAP0"] < p.cache_depth <= 4 * MC.K["CAP0"]
    assert p.passes == 2
    # no overflow in k_closest_chunks or in the fix rounds of the first attempt: its in-order
    # pass meets it
    assert p.fix_rounds == [MC.K["FIX_ROUNDS"]] * 2
    assert p.serial == [True, True]


def test_random_nested_ends_in_the_serial_pass():
    p = paths("nested", True)
    assert p.passes == 1 and p.clamped == 0
    assert p.serial == [True]
    assert p.fix_rounds == [MC.K["FIX_ROUNDS"]]


def test_random_sparse_converges_in_the_fix_rounds():
    p = paths("sparse", True)
    assert p.passes == 1 and p.clamped == 0
    assert 1 <= p.fix_rounds[0] <= MC.K["FIX_ROUNDS"]
    assert p.serial == [False]


def test_half_of_a_zero_length_candidate_is_what_c_doubles_give():
    """prop = (cen + 1 - cs) / 0.0 = +inf in C, not below 0.5; cen < cs gives prop = 0"""
    assert M._half((0, 50, 50), (0, 10, 100)) is False   # cen = 54.5 >= 50
    assert M._half((0, 60, 60), (0, 10, 100)) is True    # cen < 60
    # the kernel's integer form (cl_run) agrees on zero-length candidates inside the ref row
    for bs, be in ((10, 100), (10, 101), (0, 3)):
        for cs in range(bs + 1, be):
            integer = 2 * cs > bs + be - 1 or bs + be + 1 - 2 * cs < 0
            assert M._half((0, cs, cs), (0, bs, be)) == integer, (bs, be, cs)


def test_the_gpu_cases_cover_every_path():
    """taken together, the cases the GPU test runs reach each rung of the ladder"""
    seen = [paths(name, "--no-overlaps" not in args) for name, args in GPU_CASES]
    assert {p.passes for p in seen} >= {1, 2, 3}
    assert any(any(p.serial) for p in seen)
    assert any(sum(p.fix_rounds) and not any(p.serial) for p in seen)
    assert any(p.clamped and not sum(p.fix_rounds) for p in seen)
    assert any(p.clamped and any(p.serial) for p in seen)
