"""Seeded cost matrices for the minimum-cost assignment (include/rmpc_assign_opt.h): four kinds and a "holes" variant of
each, shared by tests/test_assign_optimal_cpu.py, tests/test_gpu_assign_optimal.py and scripts/bench_assign_optimal.py."""
import math
import zlib

import numpy as np

KINDS = ("unif", "ties", "const", "grid")


def octile(a, b, W=41):
    """octile distances (len(a), len(b)) between the cells a and b (row * W + col) of a map W cells wide"""
    dr = np.abs(a[:, None] // W - b[None, :] // W).astype(np.float64)
    dc = np.abs(a[:, None] % W - b[None, :] % W).astype(np.float64)
    return np.maximum(dr, dc) + (math.sqrt(2.0) - 1.0) * np.minimum(dr, dc)


def make_costs(kind, B, T, holes=False, seed=0):
    """(B, T) fp64.  "unif": uniform in [0, 100); "ties": integers 0 .. 3; "const": all 7.5; "grid": octile distances of
    random cells of a 41 x 41 map.  With holes: +inf in a tenth of the entries, a sprinkle of NaN, negative and
    above-limit entries (at the default scale 1024 the limit is 1024.0, which itself is takeable), one row and one
    column wholly untakeable."""
    rng = np.random.default_rng([zlib.crc32(kind.encode()), B, T, int(holes), seed])
    if kind == "unif":
        c = rng.uniform(0.0, 100.0, size=(B, T))
    elif kind == "ties":
        c = rng.integers(0, 4, size=(B, T)).astype(np.float64)
    elif kind == "const":
        c = np.full((B, T), 7.5)
    elif kind == "grid":
        c = octile(rng.integers(0, 41 * 41, B), rng.integers(0, 41 * 41, T))
    else:
        raise ValueError(kind)
    if holes:
        c[rng.uniform(size=(B, T)) < 0.1] = math.inf
        for value in (math.nan, -1.0, -math.inf, 1024.0, 1024.001, 5000.0, 1e300):
            c[rng.uniform(size=(B, T)) < 0.02] = value
        c[int(rng.integers(0, B)), :] = rng.choice([math.inf, math.nan, -2.0, 1e9], T)
        c[:, int(rng.integers(0, T))] = rng.choice([math.inf, math.nan, -2.0, 1e9], B)
    return c
