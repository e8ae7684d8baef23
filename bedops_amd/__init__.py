"""bedops_amd — MI355X-native engine for the BEDOPS sorted-interval sweep path.

The product is the C-ABI library ``bedops_amd/lib/libbedgpu.so`` (HIP kernels for
gfx950, declared in ``include/bedgpu.h``) and the drop-in C front-ends
``bedops_amd/bin/{bedops,bedmap}``. This package is the Python host mirror of that
path: it binds the C ABI with ctypes and exposes the reference's operations with the
reference's argument meaning (``bedops -m/-i/-d/-e/-n``, ``bedmap --count/--mean``).
Intervals that are already numbers go in and out as ``torch`` tensors
(``Engine.load_columns``, ``Engine.sort_columns`` for rows in any order,
``InputSet.columns``, ``Result.columns``; closest-features on such tables:
``Engine.closest_rows``, ``Result.closest``).
There is no CPU fallback: if the library cannot be loaded, importing the engine
raises.
"""
from .engine import (BedgpuError, Engine, MAP_COUNT, MAP_MEAN, BED3, BED3_REST,  # noqa: F401
                     BED5, BED3_SET, RESKIND_INTERVALS, RESKIND_ROWS, RESKIND_MAP, RESKIND_OTHER,
                     RESKIND_CLOSEST, DIST_NA, lib_path)

__all__ = ["Engine", "BedgpuError", "MAP_COUNT", "MAP_MEAN", "BED3", "BED3_REST", "BED5", "BED3_SET",
           "RESKIND_INTERVALS", "RESKIND_ROWS", "RESKIND_MAP", "RESKIND_OTHER", "RESKIND_CLOSEST",
           "DIST_NA", "lib_path"]
