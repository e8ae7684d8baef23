"""bg_closest's recovery ladder on the GPU, path by path: each design of
tests/test_closest_paths_model.py (a reader cache deeper than CAP0 and than 4 x CAP0, a deep
cache dropped at a chromosome change, look-backs clamped to CBACK with and without a wrong
start state, the random shapes that need the fix rounds and the in-order pass) must give the
oracle's bytes AND launch the kernels the CPU model (tests/model_closest_chunks.py) says it
takes: k_closest_chunks once per capacity pass, k_closest_fix iff the model has fix rounds,
k_closest_serial iff the model hands over to the in-order pass. The launches are counted by the
library's own profiling (tests/kernel_paths.py)."""
import tempfile

import pytest

import kernel_paths
import test_closest_paths_model as D
from test_gpu_parity import _closest_kwargs, run_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from bedops_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def _cases():
    return [pytest.param(name, args, id=name + "-" + ("_".join(args) or "default"))
            for name, args in D.GPU_CASES]


@pytest.mark.parametrize("name,args", _cases())
def test_closest_design_takes_its_path(eng, oracle_bin, name, args):
    d = D.design(name)
    want_path = D.paths(name, "--no-overlaps" not in args)
    with tempfile.TemporaryDirectory() as td:
        want = run_oracle(oracle_bin["closest"], args, [d.q, d.c], td)
    got, k = kernel_paths.launches(eng, lambda: eng.closest(d.q, d.c, **_closest_kwargs(args)))
    print(name, args, "model:", want_path[:6], "launched:",
          {n: c for n, c in k.items() if n.startswith("k_closest")})
    assert got == want
    assert k.get("k_closest_chunks", 0) == want_path.passes
    assert (k.get("k_closest_serial", 0) >= 1) == any(want_path.serial)
    if not any(want_path.serial):
        assert k.get("k_closest_serial", 0) == 0
    assert (k.get("k_closest_fix", 0) >= 1) == (sum(want_path.fix_rounds) > 0)
    if sum(want_path.fix_rounds) == 0:
        assert k.get("k_closest_fix", 0) == 0
