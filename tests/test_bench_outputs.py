"""bench.py's plain run and --dump-outputs.

dump_outputs() is checked on the CPU with made-up text at every size at which it takes another
path (empty, below one block, whole text kept, sampled windows). On the GPU one small plain run
with --dump-outputs is compared with the oracle on the same generated inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ["counts", "text_block_sums", "text_sample", "text_sample_offsets"]


def _load(d, suffix=""):
    assert sorted(os.listdir(d)) == sorted(f"{n}{suffix}.npy" for n in NAMES)
    return {n: np.load(os.path.join(d, f"{n}{suffix}.npy")) for n in NAMES}


@pytest.mark.parametrize("n", [0, 1, (1 << 16) - 1, (1 << 16) + 1, 1 << 23, (1 << 23) + 1, 20_000_003])
def test_dump_outputs_arrays(tmp_path, n):
    import bench
    text = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    bench.dump_outputs(str(tmp_path / "a"), 12345, text)
    bench.dump_outputs(str(tmp_path / "b"), 12345, text, suffix="_rank1")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b", "_rank1")
    raw = np.frombuffer(text, dtype=np.uint8)
    assert all(a[k].dtype == (np.float32 if k == "text_sample" else np.float64) for k in NAMES)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)  # the same text samples the same
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["counts"].tolist() == [12345, n]
    # every byte is in exactly one block sum
    blk = bench.DUMP_BLOCK
    assert len(a["text_block_sums"]) == -(-n // blk)
    assert a["text_block_sums"].sum() == raw.sum(dtype=np.uint64)
    if n:
        assert a["text_block_sums"][-1] == raw[(n - 1) // blk * blk:].sum(dtype=np.uint64)
    offs = a["text_sample_offsets"].astype(np.int64)
    if n <= bench.DUMP_WINDOWS * blk:  # the whole text
        assert offs.tolist() == [0] and np.array_equal(a["text_sample"], raw.astype(np.float32))
    else:  # windows in offset order, the first and the last among them
        assert len(offs) == bench.DUMP_WINDOWS and offs[0] == 0 and offs[-1] == n - blk
        assert np.all(np.diff(offs) >= 0)
        want = np.concatenate([raw[o:o + blk] for o in offs]).astype(np.float32)
        assert np.array_equal(a["text_sample"], want)
    # one changed byte anywhere changes the dump
    if n:
        changed = bytearray(text)
        changed[n // 2] ^= 1
        bench.dump_outputs(str(tmp_path / "c"), 12345, bytes(changed))
        assert not np.array_equal(_load(tmp_path / "c")["text_block_sums"], a["text_block_sums"])


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT)
    assert r.returncode == 2 and b"--steps" in r.stderr


SCALE = 0.0005  # 50,000 rows per input


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--scale", str(SCALE), "--dump-outputs", str(d)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().strip().splitlines()
    assert len(lines) == 1  # one JSON result line
    return json.loads(lines[0]), _load(d)


@pytest.mark.gpu
def test_plain_run_result_line(plain_run):
    line, dump = plain_run
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["unit"] == "intervals/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int64" and line["metric"].startswith("intervals/sec")
    rows = sum(line["config"]["rows_per_input"])
    # value = rows per second of one timed step (ms_per_step is printed to 0.001 ms, value to 0.1)
    ms = line["ms_per_step"]
    assert rows / ((ms + 0.00051) / 1e3) - 0.1 <= line["value"] <= rows / ((ms - 0.00051) / 1e3) + 0.1
    # nothing beside the headline figure was measured
    assert line["full"] is False
    for k in ("roofline", "cpu_baseline", "e2e", "parity", "multi_gpu", "kernels_warm_step_ms"):
        assert line[k] is None, k
    assert dump["counts"][0] == line["config"]["output_rows"]


@pytest.mark.gpu
def test_dumped_output_is_the_oracles(plain_run, oracle_bin, tmp_path):
    """the dumped text (kept whole at this size) is `bedops -i` of the same generated inputs"""
    import bench
    line, dump = plain_run
    W = bench.WORKLOADS["intersect"]
    L = bench.bedgen_lib()
    paths = []
    for i, ((seed, mode), n) in enumerate(zip(W["gen"], W["rows"])):
        p, nb, _ = bench.gen(L, int(n * SCALE), seed, (1 << 64) - 1, mode)
        paths.append(str(tmp_path / f"in{i}.bed"))
        with open(paths[-1], "wb") as f:
            f.write(bench.host_bytes(p, nb))
        L.bedgen_free(p)
    want = subprocess.run([oracle_bin["bedops"], "-i", *paths], stdout=subprocess.PIPE, check=True).stdout
    got = dump["text_sample"].astype(np.uint8).tobytes()
    assert len(want) > 0 and got == want
    assert dump["counts"].tolist() == [want.count(b"\n"), len(want)]
