"""--ec validation: the GPU grammar (bedops_amd/csrc/bg_check.h, compiled
here with g++) and the library's message wording against the oracle's restatement of
Bed::bed_check_iterator (oracle/ec_oracle.c) on every error class; the GPU run of the same
cases goes through the CLIs (tests/test_gpu_check.py)."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import ROOT

# one or more lines per error class of BedCheckIterator.hpp:326-624 (3-field BED unless noted)
CASES = [
    b"chr1\t5\t10\n\nchr1\t6\t7\n", b"chr1 \t5\t10\n", b"\tchr1\t5\t10\n", b"chr1\n",
    b"c" * 130 + b"\t1\t2\n", b"chr1\t\t5\n", b"chr1\t-5\t10\n", b"chr1\t5 \t10\n",
    b"chr1\t5x\t10\n", b"chr1\t+5\t10\n", b"chr1\t5\n", b"chr1\t1234567890123\t2\n",
    b"chr1\t5\t\t\n", b"chr1\t5\t-10\n", b"chr1\t5\t10 x\n", b"chr1\t5\t1y0\n",
    b"chr1\t5\t10\r\n", b"chr1\t5\t1234567890123\n", b"chr1\t5\t10\nchr1\t4\t10\n",
    b"chr2\t5\t10\nchr1\t4\t10\n", b"chr1\t5\t10\nchr1\t5\t9\n", b"chr1\t5\t5\n",
    b"chr1\t7\t5\n", b"track name=x\nbrowser position\n#c\n@h\nchr1\t5\t10\n",
    b"chr1\t5\t10\ntrack x\n", b"chr1\t5\t10\n#late\n", b"chr1\t5\t10", b"chr1\t5\t",
    b"TRACK\nchr1\t1\t2\nchr1\t1\t2\n", b"chr1\t5\t10\tb\nchr1\t5\t10\ta\n",
    b"chr1\t5\t10\t0b\nchr1\t5\t010\ta\n", b"chr10\t1\t2\nchr1\t3\t4\n", b"",
]
CASES5 = [  # map files under score operations: 5 fields
    b"chr1\t5\t10\tid\t1\n", b"chr1\t5\t10\n", b"chr1\t5\t10\tid\n", b"chr1\t5\t10\t\t3\n",
    b"chr1\t5\t10\ti d\t3\n", b"chr1\t5\t10\tid\t\n", b"chr1\t5\t10\tid\t1.2.3\n",
    b"chr1\t5\t10\tid\t1e5.0\n", b"chr1\t5\t10\tid\t1e5e3\n", b"chr1\t5\t10\tid\t1 2\n",
    b"chr1\t5\t10\tid\t1-2\n", b"chr1\t5\t10\tid\t1e+-2\n", b"chr1\t5\t10\tid\t1e2-\n",
    b"chr1\t5\t10\tid\t-15\trest\n", b"chr1\t5\t10\tid\t3x\n", b"chr1\t5\t10\tid\t1e5-\n",
]
# bedmap --faster --ec's nested-row check (BedCheckIterator.hpp:612-615, maxEnd_ = the previous
# row's end, :632): (file, the expected message or None, the row it is reported on)
NESTED = b"Fully nested component found."
NEST_CASES = [
    (b"chr1\t5\t100\nchr1\t10\t20\n", NESTED, 2),                   # nested after a longer row
    (b"chr1\t5\t100\nchr1\t10\t100\n", None, 0),                    # equal ends
    (b"chr1\t5\t100\nchr1\t10\t101\n", None, 0),
    (b"chr1\t5\t100\nchr2\t10\t20\n", None, 0),                     # the next chromosome
    (b"chr1\t5\t100\nchr1\t4\t20\n", b"Bed file not properly sorted by start coordinates.", 2),
    (b"chr1\t5\t100\nchr1\t5\t20\n", b"Bed file not properly sorted by end coordinates when start "
     b"coordinates are identical.", 2),                                # nested and unsorted: sort wins
    (b"chr2\t5\t100\nchr1\t10\t20\n", b"Bed file not properly sorted by first column.", 2),
    (b"chr1\t5\t100\nchr1\t30\t20\n", NESTED, 2),                   # nested and end <= start
    (b"chr1\t5\t100\nchr1\t30\t30\n", NESTED, 2),
    (b"chr1\t5\t100\nchr1\t10\t200\nchr1\t20\t150\n", NESTED, 3),  # against the previous row,
    (b"chr1\t5\t100\nchr1\t10\t20\nchr1\t30\t40\n", NESTED, 2),    # not a running maximum
    (b"chr1\t5\t200\nchr1\t10\t300\nchr1\t20\t250\tx\nchr1\t30\t40\n", NESTED, 3),
    (b"#h\nchr1\t5\t100\nchr1\t10\t20\n", NESTED, 3),
]


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ck") / "ck")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe,
                    os.path.join(ROOT, "tests", "cpu", "check_main.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-s", "-j8", "lib", "oracle"], cwd=ROOT, check=True,
                   stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(os.path.join(ROOT, "bedops_amd", "lib", "libbedgpu.so"))
    L.bg_check_message.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64]
    return L


def gpu_grammar_raw(check_bin, path, nf, rest, nest=0):
    """check_main's (row, code, line offset, line length) of the first failing line, or None"""
    r = subprocess.run([check_bin, str(nf), str(rest), path, str(int(nest))], stdout=subprocess.PIPE)
    assert r.returncode in (0, 1), r.returncode
    return tuple(map(int, r.stdout.split())) if r.returncode else None


def raw_text(lib, path, data, raw, nf, rest):
    """the exception text for check_main's result `raw`, worded by the library"""
    if raw is None:
        return b""
    row, code, off, ln = raw
    buf = ctypes.create_string_buffer(4096)
    assert lib.bg_check_message(data[off:off + ln], ln, code, nf, rest, buf, 4096) == 0
    return f"in {path}\n".encode() + buf.value + f"\nSee row: {row}".encode()


def gpu_grammar_text(check_bin, lib, path, data, nf, rest, nest=0):
    return raw_text(lib, path, data, gpu_grammar_raw(check_bin, path, nf, rest, nest), nf, rest)


def oracle_text(path, nf, rest, nest=0):
    r = subprocess.run([os.path.join(ROOT, "oracle", "build", "ec_oracle"), str(nf), str(rest), path,
                        str(int(nest))], stdout=subprocess.PIPE)
    assert r.returncode in (0, 1), r.returncode
    return r.stdout


GRAMMAR_PARAMS = [(3, 0, CASES), (3, 1, CASES), (5, 1, CASES5 + CASES)]


@pytest.mark.parametrize("nf,rest,cases", GRAMMAR_PARAMS)
def test_check_grammar_matches_oracle(check_bin, lib, tmp_path, nf, rest, cases):
    for i, data in enumerate(cases):
        p = str(tmp_path / f"c{i}.bed")
        with open(p, "wb") as f:
            f.write(data)
        assert gpu_grammar_text(check_bin, lib, p, data, nf, rest) == oracle_text(p, nf, rest), data


@pytest.mark.parametrize("nf,rest", [(3, 0), (3, 1)])
def test_check_nest_matches_oracle(check_bin, lib, tmp_path, nf, rest):
    """BGC_NESTED: the oracle gives the message and row stated with each case, the GPU grammar
    gives the oracle's text, and without nest the same files raise no nest message"""
    for i, (data, msg, row) in enumerate(NEST_CASES):
        p = str(tmp_path / f"n{i}.bed")
        with open(p, "wb") as f:
            f.write(data)
        want = oracle_text(p, nf, rest, 1)
        assert want == (f"in {p}\n".encode() + msg + f"\nSee row: {row}".encode() if msg else b""), data
        assert gpu_grammar_text(check_bin, lib, p, data, nf, rest, 1) == want, data
        plain = oracle_text(p, nf, rest)
        assert NESTED not in plain and gpu_grammar_text(check_bin, lib, p, data, nf, rest) == plain, data


def mutation_files():
    """400 small sorted files with up to three bytes overwritten (a fixed seed)"""
    rng = random.Random(9)
    alphabet = b"\t \n0123456789-+.eExchr#@\r"
    for trial in range(400):
        rows = sorted((rng.choice(["chr1", "chr2", "chr10"]), s, s + rng.randint(1, 30))
                      for s in rng.sample(range(1000), 12))
        data = bytearray("".join(f"{c}\t{s}\t{e}\tid{k}\t{k}\n" for k, (c, s, e) in enumerate(rows)).encode())
        for _ in range(rng.randint(0, 3)):
            data[rng.randrange(len(data))] = rng.choice(alphabet)
        yield trial, bytes(data)


MUTATION_PARAMS = ((3, 0), (3, 1), (5, 1))


def test_check_random_mutations(check_bin, lib, tmp_path):
    for trial, data in mutation_files():
        p = str(tmp_path / "m.bed")
        with open(p, "wb") as f:
            f.write(data)
        for nf, rest in MUTATION_PARAMS:
            assert gpu_grammar_text(check_bin, lib, p, data, nf, rest) == oracle_text(p, nf, rest), (trial, data)
