"""A CPU model of how bg_closest (bedops_amd/csrc/bg_closest.hip) gets from speculative chunks
to the exact answer: which of its recovery paths a given input takes.

  - k_closest_chunks: chunk k > 0 of CQ ref rows starts CW rows early with an empty cache at
    fp = max(lower_bound(cs, qs[qw] - lmax - 1), lower_bound(cs, qs[qw]) - CBACK) on
    chrom << 40 | coord keys, replays the CW rows, records its start state, runs its rows;
  - k_closest_check: chunk k is flagged when its start state differs from chunk k-1's final one;
  - k_closest_fix: up to FIX_ROUNDS rounds, each re-running the flagged chunks whose
    predecessor is not flagged from that predecessor's final state;
  - k_closest_serial: one in-order pass over what is left after FIX_ROUNDS rounds;
  - closest_pass is repeated with four times the capacity when a kept list, or the cache plus
    the kept list, outgrew `cap` entries in a chunk's own rows (an overflow in the speculative
    rows only leaves that chunk to the fix-up).

The constants come from the #define lines of bg_closest.hip, so retuning them retunes the
model. Rows are (chrom id, start, end) as in model_closest_seq, whose run_seq is the scan.
"""
import bisect
import os
import re
from collections import namedtuple

import model_closest_seq as M

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bedops_amd", "csrc",
                    "bg_closest.hip")


def constants(path=_SRC):
    """CQ_DEF, CW_DEF, CBACK, CAP0, FIX_ROUNDS as bg_closest.hip defines them"""
    with open(path) as f:
        src = f.read()
    out = {}
    for name in ("CQ_DEF", "CW_DEF", "CBACK", "CAP0", "FIX_ROUNDS"):
        m = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)\b" % name, src, re.M)
        assert len(m) == 1, (name, m)
        out[name] = int(m[0])
    return out


K = constants()

Paths = namedtuple("Paths", "passes fix_rounds serial clamped cache_depth kept_depth out")
# passes: closest_pass calls (= k_closest_chunks launches); fix_rounds: k_closest_fix launches
# of each pass; serial: whether k_closest_serial runs in each pass; clamped: chunk starts whose
# look-back was cut to CBACK candidates; cache_depth / kept_depth: the deepest cache (with the
# kept list about to be pushed) and the longest kept list of the in-order scan; out: the
# [(left, right)] the last pass leaves

_NO_START = ("no predecessor ends here",)  # k_closest_chunks: st_fp = ~0 after a speculative overflow
_NO_FINAL = ("no successor starts here",)  # cl_own: st_fp = ~0 - 1 after an overflow


def _key(chrom, coord):
    return (chrom << 40) | coord


def _run(Q, C, overlaps, state, rows, cap):
    """(outputs, final state) of cl_run over Q[rows] from state; final state None on overflow"""
    depth = [0, 0]
    out, states = M.run_seq(Q, C, overlaps, state, rows, depth)
    if depth[0] > cap:  # (a kept list longer than cap is deeper than cap with the cache too)
        return out, None
    return out, (states[-1] if states else (state[0], tuple(state[1])))


def _pass(Q, C, overlaps, cap, k):
    cq, cw = k["CQ_DEF"], k["CW_DEF"]
    nq = len(Q)
    cs = [_key(c[0], c[1]) for c in C]
    lmax = max((c[2] - c[1] for c in C), default=0)
    nchunks = (nq + cq - 1) // cq
    start, final = [None] * nchunks, [None] * nchunks
    out = [None] * nq
    overflow = False
    clamped = 0

    def own(j):
        nonlocal overflow
        q0, q1 = j * cq, min((j + 1) * cq, nq)
        res, fin = _run(Q, C, overlaps, start[j], (q0, q1), cap)
        if fin is None:
            overflow = True
            fin = _NO_FINAL
            # (cl_run stops at the overflowing row; what it wrote before does not matter: the
            # pass is thrown away)
        out[q0:q1] = res
        final[j] = fin

    for j in range(nchunks):
        if j == 0:
            start[0] = (0, ())
        else:
            qw = j * cq - cw
            kq = _key(Q[qw][0], Q[qw][1])
            p = bisect.bisect_left(cs, kq)
            f = bisect.bisect_left(cs, kq - lmax - 1)
            fp = f
            if p - f > k["CBACK"]:
                fp = p - k["CBACK"]
                clamped += 1
            _, st = _run(Q, C, overlaps, (fp, ()), (qw, j * cq), cap)
            if st is None:  # speculation overflowed: left to the fix-up, no overflow recorded
                start[j], final[j] = _NO_START, _NO_FINAL
                continue
            start[j] = st
        own(j)

    fix_rounds, serial = 0, False
    rnd = 0
    while True:
        flag = [j > 0 and start[j] != final[j - 1] for j in range(nchunks)]
        if not any(flag) or overflow:
            break
        if rnd == k["FIX_ROUNDS"]:
            serial = True
            for j in range(1, nchunks):
                if start[j] == final[j - 1]:
                    continue
                start[j] = final[j - 1]
                own(j)
                if overflow:  # (the kernel goes on from states that no longer matter: the
                    break     # pass is thrown away)
            break
        for j in [j for j in range(1, nchunks) if flag[j] and not flag[j - 1]]:
            start[j] = final[j - 1]
            own(j)
        fix_rounds += 1
        rnd += 1
    return overflow, fix_rounds, serial, clamped, out


def simulate(Q, C, overlaps=True, k=None):
    """the path bg_closest takes on ref rows Q and candidates C: a Paths"""
    k = k or K
    depth = [0, 0]
    M.run_seq(Q, C, overlaps, depth=depth)
    fix_rounds, serial = [], []
    cap = k["CAP0"]
    clamped, out = 0, []
    while Q:
        ovf, fr, se, clamped, out = _pass(Q, C, overlaps, cap, k)
        fix_rounds.append(fr)
        serial.append(se)
        if not ovf:
            break
        cap *= 4
        assert cap <= 1 << 30, "the model's capacity does not converge"
    return Paths(len(fix_rounds), fix_rounds, serial, clamped, depth[0], depth[1], out)
