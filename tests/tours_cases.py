"""Seeded problems for the tours (include/rmpc_tours.h), shared by tests/test_tours_cpu.py, tests/test_gpu_tours.py and
scripts/bench_tours.py: start costs (B, T) and task costs (T, T) of three kinds and a "holes" variant of each, the store
draw of examples/fleet_store_tours.py, and scripted walks for the follower."""
import math
import zlib

import numpy as np

from assign_optimal_cases import octile

KINDS = ("grid", "unif", "ties")


def make_problem(kind, B, T, holes=False, seed=0):
    """(start_cost (B, T), task_cost (T, T)) fp64.  "grid": octile distances between random cells of a 41 x 41 map
    (symmetric, metric); "unif": uniform in [0, 100), asymmetric and no metric, so that insertions with a negative delta
    occur; "ties": integers 0 .. 3.  With holes: +inf in a tenth of the entries and a sprinkle of NaN, negative and
    above-limit entries (at the default scale 1024 the limit is 1024.0, which itself is takeable), and one task that no
    edge leads to."""
    rng = np.random.default_rng([zlib.crc32(kind.encode()), B, T, int(holes), seed])
    if kind == "grid":
        cells = rng.integers(0, 41 * 41, B + T)
        s, d = octile(cells[:B], cells[B:]), octile(cells[B:], cells[B:])
    elif kind == "unif":
        s, d = rng.uniform(0.0, 100.0, size=(B, T)), rng.uniform(0.0, 100.0, size=(T, T))
    elif kind == "ties":
        s, d = rng.integers(0, 4, size=(B, T)).astype(np.float64), rng.integers(0, 4, size=(T, T)).astype(np.float64)
    else:
        raise ValueError(kind)
    if holes:
        for m in (s, d):
            m[rng.uniform(size=m.shape) < 0.1] = math.inf
            for value in (math.nan, -1.0, -math.inf, 1024.0, 1024.001, 1e300):
                m[rng.uniform(size=m.shape) < 0.01] = value
        lost = int(rng.integers(0, T))
        s[:, lost], d[:, lost] = math.inf, math.nan
    return s, d


def small_integer_problem(rng, B, T, holes):
    """quantised costs (qs (B, T), qt (T, T)) in 0 .. 9 with -1 on a fifth of the edges when holes"""
    qs, qt = rng.integers(0, 10, size=(B, T)), rng.integers(0, 10, size=(T, T))
    if holes:
        qs[rng.uniform(size=qs.shape) < 0.2] = -1
        qt[rng.uniform(size=qt.shape) < 0.2] = -1
    return qs.astype(np.int64), qt.astype(np.int64)


def store_draw(B, T, seed=0):
    """(data (H, W) the store's enlarged map, starts (B,), picks (T,) int32): distinct cells clear of the shelves, drawn
    as examples/fleet_store_dispatch.py draws them (inflate_ref stands for rmpc_grid_inflate_device)"""
    from global_planner_reference import inflate_ref
    from robot_mpcs_amd.global_planner import png_values
    from robot_mpcs_amd.store import STORE as S, clear_cells, store_map
    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    data = inflate_ref(png_values(raw), S.cell, S.size_robot, 0.29)[0]
    ok = np.flatnonzero((clear_cells(raw, S.clear_cells) & (data < 0.8)).ravel())
    cells = rng.choice(ok, B + T, replace=False).astype(np.int32)
    return data, cells[:B].copy(), cells[B:].copy()
