"""What bg_result_export_map_values has to return, from two sources that are not the code under
test (shared by tests/test_map_values_abi.py and tests/test_gpu_map_values.py):

  fixture_cases()  the cases of the reference fixtures (tests/golden/ref_*.json.gz) whose
                   operations are all numeric, with what each prints per reference row;
  model()          an independent numpy model: the members of every reference row by an all-pairs
                   brute force for --bp-ovr, then the reference's rules in float64.

Sums of non-integer scores are outside the model: the reference keeps them as running doubles
across the whole sweep (added when a row enters a window, subtracted when it leaves), so their
last bits depend on every row before; the model returns None for --sum / --mean / --variance /
--stdev / --cv there. Integer sums are exact in any order (below 2^53), and the order statistics
never depend on an order of addition."""
import math

import numpy as np

import ref_fixtures

SUITES = ["bedmap", "f2", "faster", "decimal", "r6"]
OLD_OPS = ("count", "indicator", "sum", "mean", "min", "max")
NEW_OPS = ("bases", "bases-uniq", "bases-uniq-f", "echo-ref-size", "variance", "stdev", "cv", "median", "kth", "mad")
INT_OPS = ("count", "indicator", "bases", "bases-uniq", "echo-ref-size")
SUM_OPS = ("sum", "mean", "variance", "stdev", "cv")
CRIT_ARGS = {"--bp-ovr": "bp-ovr", "--range": "range", "--fraction-ref": "fraction-ref",
             "--fraction-map": "fraction-map", "--fraction-either": "fraction-either",
             "--fraction-both": "fraction-both"}


def _is_number(tok):
    try:
        float(tok)
        return True
    except ValueError:
        return False


def parse_args(args):
    """bedmap's arguments -> {"ops", "prec", "delim", "crit", "val", "faster"}, or None when
    anything but numeric operations, --prec, --delim, a criterion and --faster is among them"""
    out = {"ops": [], "prec": 6, "delim": "|", "crit": "bp-ovr", "val": 1, "faster": False}
    i = 0
    while i < len(args):
        a = args[i]
        i += 1
        if a == "--faster":
            out["faster"] = True
        elif a == "--prec":
            out["prec"] = int(args[i])
            i += 1
        elif a == "--delim":
            out["delim"] = args[i]
            i += 1
        elif a == "--exact":
            out["crit"], out["val"] = "exact", None
        elif a in CRIT_ARGS:
            out["crit"] = CRIT_ARGS[a]
            out["val"] = float(args[i]) if "fraction" in a else int(args[i])
            i += 1
        elif a == "--kth":
            out["ops"].append(("kth", float(args[i])))
            i += 1
        elif a == "--mad":
            if i < len(args) and _is_number(args[i]):
                out["ops"].append(("mad", float(args[i])))
                i += 1
            else:
                out["ops"].append(("mad",))
        elif a.startswith("--") and a[2:] in OLD_OPS + NEW_OPS:
            out["ops"].append((a[2:],))
        else:
            return None
    return out if out["ops"] else None


def fixture_cases():
    """[(suite, index, parsed arguments, input texts, columns)]: every qualifying case (numeric
    operations only, rc 0, output, one of the ten new operations, inputs from files), `columns`
    the tokens the reference printed, one list per operation"""
    out = []
    for suite in SUITES:
        fx = ref_fixtures.load(suite)
        for k, case in enumerate(fx["cases"]):
            if case.get("tool", "bedmap") != "bedmap" or case["rc"] != 0 or not case["stdout"]:
                continue
            p = parse_args(case["args"])
            if p is None or not any(op[0] in NEW_OPS for op in p["ops"]):
                continue
            if case.get("stdin") is not None or any(f < 0 for f in case["files"]):
                continue  # (input from stdin: not a load the test can express)
            texts = [fx["groups"][case["group"]][f] for f in case["files"]]
            lines = case["stdout"].split("\n")[:-1]
            toks = [ln.split(p["delim"]) for ln in lines]
            if any(len(t) != len(p["ops"]) for t in toks):
                continue  # (a delimiter that also occurs inside a number)
            out.append((suite, k, p, texts, [[t[q] for t in toks] for q in range(len(p["ops"]))]))
    return out


def fmt(op, prec, values):
    """the values of one operation as the reference prints them: NAN where there is no value
    (a NaN with the sign bit clear), -nan for a value that is a NaN (sign bit set: glibc's print
    of the x86-64 default NaN an invalid operation gives)"""
    f = "%d" if op in INT_OPS else "%%.%df" % prec
    return [("-nan" if np.signbit(v) else "NAN") if math.isnan(v) else
            "-inf" if v == -math.inf else "inf" if v == math.inf else f % v for v in values]


def parse_bed(text, score=False):
    rows, sc = [], []
    for ln in text.split("\n"):
        if not ln:
            continue
        t = ln.split("\t")
        rows.append((t[0], int(t[1]), int(t[2])))
        if score:
            sc.append(float(t[4]))
    return (rows, np.array(sc, dtype=np.float64)) if score else rows


def brute_bp(ref, mp, ovr):
    """--bp-ovr by all pairs: per reference row the map rows that overlap it by >= ovr bases
    (inputs without zero-length rows: the sweep window is then every overlapping row)"""
    chroms = {c: k for k, c in enumerate(sorted({r[0] for r in ref + mp}))}
    rc, rs, re = (np.array([f(r) for r in ref], dtype=np.int64) for f in
                  (lambda r: chroms[r[0]], lambda r: r[1], lambda r: r[2]))
    mc, ms, me = (np.array([f(r) for r in mp], dtype=np.int64) for f in
                  (lambda r: chroms[r[0]], lambda r: r[1], lambda r: r[2]))
    out = []
    for i in range(len(ref)):
        ov = np.minimum(re[i], me) - np.maximum(rs[i], ms)
        out.append(np.nonzero((mc == rc[i]) & (ov >= ovr))[0])
    return out


def _kth(x, kth):
    """RollingKthAverage::DoneReference on the sorted scores x"""
    n = len(x)
    if n == 1:
        return x[0]
    up, down = int(math.ceil(kth * n)), int(math.floor(kth * n))
    up -= up > 0
    down -= down > 0
    if up == down:
        return (x[up] + (x[up + 1] if up + 1 < n else 0.0)) / 2.0
    return x[up]


def _row(op, arg, r, mp, sc, mem, integral):
    _, s, e = r
    c = len(mem)
    nan = float("nan")
    if op == "count":
        return float(c)
    if op == "indicator":
        return 1.0 if c else 0.0
    if op == "echo-ref-size":
        return float(e - s)
    if op in ("bases", "bases-uniq", "bases-uniq-f"):
        cl = sorted((max(s, mp[m][1]), min(e, mp[m][2])) for m in mem)
        if op == "bases":
            return float(sum(b - a for a, b in cl))
        uniq, end = 0, s
        for a, b in cl:
            if b > max(a, end):
                uniq += b - max(a, end)
                end = b
        uniq &= 0xFFFFFFFF  # (OvrUnique counts in an unsigned int)
        return float(uniq) if op == "bases-uniq" else np.float64(uniq) / np.float64(e - s)
    if c == 0:
        return nan
    x = np.sort(sc[mem])
    if op == "min":
        return x[0]
    if op == "max":
        return x[-1]
    if op in SUM_OPS:
        if not integral:
            return None
        isum = sum(int(v) for v in x)
        isq = sum(int(v) * int(v) for v in x)
        if op == "sum":
            return float(isum)
        if op == "mean":
            return float(isum) / float(c)
        if c <= 1:
            return nan
        cnt, sm, sq = float(c), float(isum), float(isq)
        v = ((cnt * sq) - (sm * sm)) / (cnt * (cnt - 1))
        if op != "variance":
            v = math.sqrt(v) if v >= 0 else nan
        if op == "cv":
            mean = sm / cnt
            v = nan if mean == 0 else v / mean
        return v
    if op == "median":
        return _kth(x, 0.5)
    if op == "kth":
        return _kth(x, arg)
    if op == "mad":
        if c <= 1:
            return nan
        d = np.sort(np.abs(x - _kth(x, 0.5)))
        mad = (d[c // 2 - 1] + d[c // 2]) / 2.0 if c % 2 == 0 else d[c // 2]
        return mad * (arg if arg and arg > 0 else 1.0)
    raise ValueError(op)


def model(ops, ref, mp, scores, members):
    """per operation of `ops` (tuples as Engine.map_op takes them) a float64 array with one
    value per reference row, or None where the model does not apply (module docstring)"""
    sc = np.asarray(scores, dtype=np.float64)
    integral = bool(len(sc) == 0 or (np.all(sc == np.round(sc)) and np.all(np.abs(sc) < 2.0 ** 26)))
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for op in ops:
            op = op if isinstance(op, tuple) else (op,)
            name, arg = op[0], (op[1] if len(op) > 1 else 0.0)
            if name in SUM_OPS and not integral:
                out.append(None)
                continue
            out.append(np.array([_row(name, arg, ref[i], mp, sc, members[i], integral) for i in range(len(ref))],
                                dtype=np.float64))
    return out
