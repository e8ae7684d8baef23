"""The input preparation of tools/bench_sort_columns.py on the CPU: it is sized by the tensors it
is given, never by the row count that was asked of the generator. tools/bedgen.c rounds each
contig's share of the rows, so it may return fewer rows than asked (4,096 asked: 4,095 made); a
permutation of the asked count would then index past the end of the columns."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import bench
from conftest import ROOT

ASKED, MADE = 4096, 4095


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("bench_sort_columns",
                                                  os.path.join(ROOT, "tools", "bench_sort_columns.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def generated(bedgen):
    """(names, chrom, start, end) of ASKED rows asked of the generator (seed 1, every contig),
    parsed on the host; names in strcmp order"""
    L = bench.bedgen_lib()
    mask = (1 << len(bench.contigs(L))) - 1
    p, nb, made = bench.gen(L, ASKED, 1, mask, 3)
    text = bytes(bench.host_bytes(p, nb))
    L.bedgen_free(p)
    rows = [ln.split(b"\t") for ln in text.splitlines()]
    assert made == len(rows)
    names = sorted({r[0] for r in rows})
    idx = {nm: k for k, nm in enumerate(names)}
    return ([nm.decode() for nm in names], np.array([idx[r[0]] for r in rows], dtype=np.int32),
            np.array([int(r[1]) for r in rows], dtype=np.int64), np.array([int(r[2]) for r in rows], dtype=np.int64))


def test_the_generator_returns_a_row_fewer_than_asked(generated):
    # (the point of this file: were this ASKED, the tests below would not show the sizing rule)
    assert len(generated[1]) == MADE != ASKED


def test_shuffle_is_sized_by_the_columns(tool, generated):
    names, chrom, start, end = generated
    cols = [torch.as_tensor(c) for c in (chrom, start, end)]
    names2, out, perm = tool.shuffled(names, cols, seed=5)
    assert perm.numel() == MADE and all(c.numel() == MADE for c in out)
    assert np.array_equal(np.sort(perm.numpy()), np.arange(MADE))
    assert not np.array_equal(perm.numpy(), np.arange(MADE))
    # the name list: the same names, no longer in strcmp order
    assert sorted(names2) == names and names2 != names
    c2, s2, e2 = (c.numpy() for c in out)
    assert out[0].dtype == torch.int32 and out[1].dtype == torch.int64
    # a reordering of the originals, row by row
    assert [names2[k] for k in c2] == [names[k] for k in chrom[perm.numpy()]]
    assert np.array_equal(s2, start[perm.numpy()]) and np.array_equal(e2, end[perm.numpy()])
    # sorted back with numpy (names by byte order, then start, then end): the generator's rows
    rank = np.argsort(np.argsort(np.array([nm.encode() for nm in names2])))
    back = np.lexsort((e2, s2, rank[c2]))
    assert [names2[k] for k in c2[back]] == [names[k] for k in chrom]
    assert np.array_equal(s2[back], start) and np.array_equal(e2[back], end)
    # the same seed gives the same shuffle; the inputs are left as they were
    _, again, perm2 = tool.shuffled(names, cols, seed=5)
    assert torch.equal(perm, perm2) and all(torch.equal(a, b) for a, b in zip(out, again))
    assert np.array_equal(cols[1].numpy(), start)


def test_unequal_columns_are_refused_before_any_indexing(tool, generated):
    names, chrom, start, end = generated
    cols = [torch.as_tensor(chrom), torch.as_tensor(start), torch.as_tensor(end)]
    for k in range(3):
        bad = list(cols)
        bad[k] = torch.cat([bad[k], bad[k][:1]])  # ASKED rows where the others have MADE
        with pytest.raises(ValueError, match="rows"):
            tool.shuffled(names, bad, seed=5)
    with pytest.raises(ValueError, match="rows"):
        tool.shuffled(names, [cols[0], cols[1].reshape(-1, 1)[:, 0:1], cols[2]], seed=5)
    with pytest.raises(ValueError, match="chrom index"):
        tool.shuffled(names[:-1], cols, seed=5)
    assert tool.shuffled([], [c[:0] for c in cols], seed=5)[2].numel() == 0
