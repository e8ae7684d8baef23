"""Block accounting of the context's allocator (bg_live): after every operation, on success,
on the refusals the suite provokes elsewhere, and with a device allocation made to fail at
every position of the call sequence (bg_fail_alloc_after), the context holds exactly the
blocks it held before, and the next run on good input prints what the first run printed.

Shapes: 1,500 rows over 3 chromosomes (several 8 KiB parse tiles, more than one 1,024-element
merge-path segment), an empty input, an input with zero-length rows (the symmdiff stream
replay and bedmap's zin / zout windows), and a 300-row reference for bedmap and
closest-features."""
import ctypes
import random

import pytest

import randbed

pytestmark = pytest.mark.gpu

CHROMS = ["chr1", "chr2", "chrX"]
NOMEM, UNSORTED, ARG, UNSUPPORTED = -7, -3, -6, -8
MAX_N = 400


@pytest.fixture(scope="module")
def eng():
    from bedops_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _texts():
    rng = random.Random(20261020)
    t = {}
    a = randbed.rows(rng, 1500, chroms=CHROMS, span=200000, maxlen=300)
    b = randbed.rows(rng, 1500, chroms=CHROMS, span=200000, maxlen=300)
    z = randbed.rows(rng, 1500, chroms=CHROMS, span=200000, maxlen=300, zero_frac=0.1)
    r = randbed.rows(rng, 300, chroms=CHROMS, span=200000, maxlen=300)
    t["a"] = randbed.text(a).encode()
    t["b"] = randbed.text(b).encode()
    t["z"] = randbed.text(z).encode()
    t["empty"] = b""
    t["a_rest"] = randbed.text(a, rest="cols", rng=rng).encode()
    t["b_rest"] = randbed.text(b, rest="cols", rng=rng).encode()
    t["b5"] = randbed.text(b, rest="bed5", rng=rng).encode()
    t["z5"] = randbed.text(z, rest="bed5", rng=rng).encode()
    t["r"] = randbed.text(r).encode()
    t["r_rest"] = randbed.text(r, rest="cols", rng=rng).encode()
    lines = t["a_rest"].splitlines(keepends=True)
    rng.shuffle(lines)
    t["shuffled"] = b"".join(lines)
    k = next(k for k in range(700, 1400) if a[k][0] == a[k + 1][0] and a[k][1] < a[k + 1][1])
    t["unsorted"] = randbed.text(a[:k] + [a[k + 1], a[k]] + a[k + 2:]).encode()
    # past the key range once padded: refused on the GPU path (ERR_RANGE)
    t["far"] = t["a"] + b"chrX\t1099511627000\t1099511627500\n"
    # an unmapped reference row under --max-element: the text stops there (BedgpuStop)
    t["stop_ref"] = t["r"] + b"chrY\t1\t2\n"
    return t


T = _texts()


def _sortbed(eng, texts):
    """bg_sortbed through the C ABI (the engine has no wrapper: the CLI drives it)"""
    from bedops_amd.engine import BedgpuError, Result, _Input

    class _Err(ctypes.Structure):
        _fields_ = [("input", ctypes.c_int), ("line", ctypes.c_uint64), ("code", ctypes.c_int)]

    arr = (_Input * len(texts))()
    keep = [ctypes.create_string_buffer(t, len(t) + 1) for t in texts]
    for i, t in enumerate(texts):
        arr[i].data = ctypes.cast(keep[i], ctypes.c_void_p)
        arr[i].nbytes, arr[i].on_device, arr[i].kind = len(t), 0, 0
    h, err = ctypes.c_void_p(), _Err()
    fn = eng.L.bg_sortbed
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(_Input), ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(_Err)]
    rc = fn(eng.ctx, len(texts), arr, ctypes.byref(h), ctypes.byref(err))
    if rc:
        raise BedgpuError(rc, eng.L.bg_last_error(eng.ctx).decode(errors="replace"))
    r = Result(eng, h)
    try:
        return r.text()
    finally:
        r.free()


def _load(kind):
    def run(eng):
        s = eng.load([(T["b5"], kind), (T["z5"], kind), (T["empty"], kind)])
        try:
            return b"%d %d %d" % (s.rows(0) if kind != 3 else 0, s.rows(1) if kind != 3 else 0, len(s.chroms()))
        finally:
            s.free()
    return run


def _pad(eng, texts=None, pad=(-150, 40)):
    return eng.bedops("-m", texts or [T["a"], T["z"]], pad=pad)


# every cycle loads its inputs, runs the operation, formats and frees the result and the set
# (the engine's one-call wrappers do exactly that, with the frees in `finally` blocks)
OPS = {
    "merge": lambda e: e.bedops("-m", [T["a"], T["b"], T["empty"]]),
    "intersect": lambda e: e.bedops("-i", [T["a"], T["b"]]),
    "intersect-zero": lambda e: e.bedops("-i", [T["a"], T["z"]]),
    "difference": lambda e: e.bedops("-d", [T["a"], T["b"], T["z"]]),
    "element-of": lambda e: e.bedops("-e", [T["a_rest"], T["b"]], spec="1"),
    "not-element-of": lambda e: e.bedops("-n", [T["a_rest"], T["b"], T["empty"]], spec="50%"),
    "complement": lambda e: e.bedops("-c", [T["a"], T["b"]], full_left=True),
    "chop": lambda e: e.bedops("-w", [T["a"], T["b"]], chop=(100, 30, True)),
    "partition": lambda e: e.bedops("-p", [T["a"], T["z"]]),
    "symmdiff": lambda e: e.bedops("-s", [T["a"], T["b"]]),
    "symmdiff-replay": lambda e: e.bedops("-s", [T["a"], T["z"], T["empty"]]),
    "everything": lambda e: e.bedops("-u", [T["a_rest"], T["b_rest"], T["empty"]]),
    "pad": _pad,
    "check": lambda e: repr((e.check(T["a_rest"], 6, True), e.check(T["unsorted"]))).encode(),
    "bedmap-count": lambda e: e.bedmap(["echo", "count", "echo-ref-row-id"], T["r_rest"], T["b"], skip_unmapped=True),
    "bedmap-mean": lambda e: e.bedmap(["mean", "sum", "stdev"], T["r"], T["b5"]),
    "bedmap-tmean": lambda e: e.bedmap([("tmean", 0.1, 0.2)], T["r"], T["b5"]),
    "bedmap-echo-map": lambda e: e.bedmap(["echo-map"], T["r"], T["b_rest"]),
    "bedmap-bases-uniq": lambda e: e.bedmap(["bases-uniq", "bases"], T["r"], T["z"]),
    "bedmap-zero-single": lambda e: e.bedmap(["count", "echo-map-id"], T["z5"]),
    "bedmap-faster": lambda e: e.bedmap(["count", "mean"], T["r"], T["b5"], faster=True),
    "closest": lambda e: e.closest(T["r_rest"], T["b_rest"], dist=True),
    "sort-bed": lambda e: _sortbed(e, [T["shuffled"], T["empty"], T["b"]]),
    "load-bed3": _load(0),
    "load-bed3-set": _load(3),
    "load-bed3-rest": _load(1),
    "load-bed5": _load(2),
}


@pytest.fixture(scope="module")
def warm(eng):
    """each operation's text from a first run (which also fills the pool), computed once"""
    return {name: fn(eng) for name, fn in OPS.items()}


@pytest.mark.parametrize("name", list(OPS))
def test_balance_on_success(eng, warm, name):
    base = eng.live()
    got = OPS[name](eng)
    assert eng.live() == base
    assert got == warm[name]
    assert len(got) > 0


def _stop(eng):
    from bedops_amd.engine import BedgpuStop
    with pytest.raises(BedgpuStop):
        eng.bedmap(["echo", "max-element"], T["stop_ref"], T["b5"])


def _raises(code, fn):
    def run(eng):
        from bedops_amd import BedgpuError
        with pytest.raises(BedgpuError) as ei:
            fn(eng)
        assert ei.value.code == code, str(ei.value)
    return run


def _partition_on_set(eng):
    s = eng.load([(T["a"], 3), (T["b"], 3)])
    try:
        eng.op("-p", s, [0, 1]).free()
    finally:
        s.free()


# (the symmdiff push-back overflow needs more than three pending pieces per file head, which
# no input of this size reaches: the stack depth is bounded by 2, see k_sd_replay)
FAILURES = {
    "pad-range": (_raises(UNSUPPORTED, lambda e: _pad(e, [T["far"], T["z"]], (0, 1000))), "pad"),
    "bedmap-stop": (_stop, "bedmap-mean"),
    "unsorted-rows": (_raises(UNSORTED, lambda e: e.bedmap(["count"], T["unsorted"], T["b"])), "bedmap-count"),
    "partition-on-set": (_raises(ARG, _partition_on_set), "partition"),
}


@pytest.mark.parametrize("name", list(FAILURES))
def test_balance_on_refusal(eng, warm, name):
    fail, good = FAILURES[name]
    base = eng.live()
    fail(eng)
    assert eng.live() == base
    assert OPS[good](eng) == warm[good]
    assert eng.live() == base


@pytest.mark.parametrize("name", list(OPS))
def test_balance_on_injected_allocation_failure(eng, warm, name):
    """the n-th allocation of the cycle fails, for every n the cycle reaches"""
    from bedops_amd import BedgpuError
    base = eng.live()
    failed = 0
    for n in range(1, MAX_N + 1):
        eng.fail_alloc_after(n)
        try:
            got = OPS[name](eng)
        except BedgpuError as e:
            assert e.code == NOMEM, (n, str(e))
            assert "injected" in str(e), (n, str(e))
            assert eng.live() == base, n
            failed += 1
            continue
        finally:
            eng.fail_alloc_after(0)
        assert got == warm[name], n
        assert eng.live() == base, n
        break
    else:
        pytest.fail(f"{name}: no success within {MAX_N} allocations")
    print(f"{name}: {failed} allocations failed in turn")
    assert failed >= 1, "the cycle made no device allocation"
