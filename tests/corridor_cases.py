"""The cases the corridor tests share (tests/test_corridor_cpu.py, tests/test_gpu_corridor.py): the hand map of the
issue's table, the small maps of the any-angle tests, the store's raw maps, a sparse seeded 300 x 300 map on which a
reach of 64 and 256 has room, a map of special values, and seeded point sets with points exactly on cell boundaries, in
occupied cells, outside the map, NaN and +inf."""
import numpy as np

from any_angle_cases import small_maps, store_raw      # noqa: F401  (shared with the corridor tests)

OCC = 0.8
FRAME = (-1.3, 0.7, 0.45)            # (x0, y0, cell) of the small maps: nothing special about it
EXACT = (-75.0, -75.0, 0.5)          # of the 300 x 300 map: (c + 0.5) cell is exact, so boundary points round half to even


def store_frame():
    from robot_mpcs_amd.store import STORE as S
    return (S.x0, S.y0, S.cell)


def hand_map():
    """5 x 7, free but for (1, 4) and (3, 1)"""
    g = np.zeros((5, 7))
    g[1, 4] = g[3, 1] = 1.0
    return g


# seed, reach -> rectangle (r0, r1, c0, c1) on hand_map(), from the prototype of the rule
HAND = [((2, 2), 8, (0, 4, 2, 3)), ((2, 2), 1, (1, 3, 2, 3)), ((0, 0), 8, (0, 2, 0, 3)), ((4, 6), 8, (2, 4, 2, 6))]


def sparse_map(H=300, W=300, share=0.003, seed=33):
    return (np.random.default_rng(seed).uniform(size=(H, W)) < share).astype(np.float64)


def special_map():
    """7 x 9 with a NaN cell (occupied), a cell equal to the threshold (occupied), a negative cell and one just below
    the threshold (free), an infinite cell (occupied)"""
    g = np.full((7, 9), 0.25)
    g[1, 2], g[3, 4], g[5, 6], g[2, 7], g[4, 1] = np.nan, OCC, -3.0, np.nextafter(OCC, 0.0), np.inf
    return g


def sums_maps():
    """name -> map for the summed-area table: the edge shapes, the widths at the wavefront's 64-cell steps, the store,
    a random 300 x 300 and the special values"""
    rng = np.random.default_rng(34)
    rand = lambda H, W, share=0.3: (rng.uniform(size=(H, W)) < share).astype(np.float64)
    maps = {"1x1_free": np.zeros((1, 1)), "1x1_occ": np.ones((1, 1)), "1x70": rand(1, 70), "70x1": rand(70, 1), "7x9": rand(7, 9)}
    for W in (63, 64, 65, 129):
        maps["5x%d" % W] = rand(5, W, 0.5)
    maps["store"] = store_raw(0)
    maps["300x300"] = rand(300, 300)
    maps["special"] = special_map()
    return maps


def free_centres(grid, frame, thr=OCC):
    """(n, 1, 3) points: the centre of every free cell, z = 0.05"""
    x0, y0, cell = frame
    r, c = np.nonzero(grid < thr)
    return np.stack([x0 + c * cell, y0 + r * cell, np.full(len(r), 0.05)], 1)[:, None, :]


def random_points(grid, frame, B, N, seed):
    """(B, N, 3) seeded points: most inside the map, every fifth exactly on a cell boundary in x, y or both
    (x0 + (c + 0.5) cell), every eleventh at the centre of an occupied cell (where there is one), every thirteenth
    outside the map, then one NaN in x, one NaN in y, one +inf, one -inf and one far beyond the int range"""
    x0, y0, cell = frame
    H, W = grid.shape
    rng = np.random.default_rng(seed)
    n = B * N
    p = np.stack([x0 + rng.uniform(-0.5, W - 0.5, n) * cell, y0 + rng.uniform(-0.5, H - 0.5, n) * cell, rng.uniform(0.0, 0.1, n)], 1)
    i = np.arange(n)
    cb, rb = rng.integers(-1, W, n), rng.integers(-1, H, n)
    on_x, on_y = (i % 5 == 0) & (i % 10 != 5), (i % 5 == 0) & (i % 15 != 10)
    p[on_x, 0] = (x0 + (cb + 0.5) * cell)[on_x]
    p[on_y, 1] = (y0 + (rb + 0.5) * cell)[on_y]
    occ_r, occ_c = np.nonzero(~(grid < OCC))
    if len(occ_r):
        j = rng.integers(0, len(occ_r), n)
        m = i % 11 == 3
        p[m, 0], p[m, 1] = (x0 + occ_c[j] * cell)[m], (y0 + occ_r[j] * cell)[m]
    m = i % 13 == 7
    p[m, :2] += (rng.choice([-1.0, 1.0], (n, 2)) * np.array([W, H]) * cell)[m]
    for k, (col, v) in enumerate(((0, np.nan), (1, np.nan), (0, np.inf), (1, -np.inf), (0, 1e300))):
        if n > 2 * k + 1:
            p[2 * k + 1, col] = v
    return p.reshape(B, N, 3)
