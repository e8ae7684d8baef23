"""Which kernels a call launched, from the library's own profiling (bg_prof_enable /
bg_prof_read): every BG_LAUNCH site records its launch under its name while a filter is set.
Profiling adds HIP events around the launches and nothing else (BG_LAUNCH, bg_internal.h), so
the kernels launched and their order are those of an unprofiled call; only timing changes."""
import ctypes


def parse(text):
    """the "<kernel> <launches> <total_ms>" lines of bg_prof_read -> {kernel: launches}, in
    first-launch order"""
    out = {}
    for ln in text.splitlines():
        if not ln.strip():
            continue
        name, calls, _ms = ln.split()
        out[name] = int(calls)
    return out


def launches(eng, call):
    """run call() with every kernel profiled: (its result, {kernel: launches})"""
    eng.prof_enable("*")
    try:
        res = call()
        buf = ctypes.create_string_buffer(1 << 16)
        eng._check(eng.L.bg_prof_read(eng.ctx, buf, 1 << 16))
        return res, parse(buf.value.decode())
    finally:
        eng.prof_enable("")
