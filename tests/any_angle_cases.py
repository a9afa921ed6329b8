"""The cases the any-angle tests share (tests/test_any_angle_cpu.py, tests/test_gpu_any_angle.py): the small maps on
which every ordered pair of cells is asked, the larger seeded ones, the store maps enlarged as ``store_routes`` does it
with dense routes from the CPU restatement of the planner, and a seeded walk along and off a fleet's routes."""
import numpy as np

OCC = 0.8


def small_maps():
    """name -> (H, W) map between 7 x 7 and 9 x 9, 1 occupied, 0 free"""
    empty = np.zeros((7, 7))
    wall = np.zeros((8, 7))
    wall[3, :] = 1.0
    wall[3, 4] = 0.0
    r, c = np.indices((9, 9))
    checker = ((r + c) % 2 == 1).astype(np.float64)
    rand = (np.random.default_rng(28).uniform(size=(7, 9)) < 0.15).astype(np.float64)
    return {"empty": empty, "wall": wall, "checker": checker, "random": rand}


def all_pairs(H, W):
    a, b = np.divmod(np.arange(H * W * H * W), H * W)
    return a.astype(np.int32), b.astype(np.int32)


def random_map(H=70, W=70, share=0.15, seed=29):
    return (np.random.default_rng(seed).uniform(size=(H, W)) < share).astype(np.float64)


def serpentine_map(H=70, W=70, pitch=10, gap=3):
    """walls every ``pitch`` rows, open for ``gap`` cells at alternating ends: a route from the first corridor to the
    last one winds through all of them"""
    g = np.zeros((H, W))
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 1.0
    for n, r in enumerate(range(pitch, H - 1, pitch)):
        g[r, :] = 1.0
        if n % 2:
            g[r, 1:1 + gap] = 0.0
        else:
            g[r, W - 1 - gap:W - 1] = 0.0
    return g


def store_data(seed):
    """shelf_map(41, 41, seed) enlarged as ``store_routes`` does it (inflate_ref stands for rmpc_grid_inflate_device)"""
    from global_planner_reference import inflate_ref
    from robot_mpcs_amd.global_planner import png_values, shelf_map
    from robot_mpcs_amd.store import STORE as S
    return inflate_ref(png_values(shelf_map(41, 41, seed)), S.cell, S.size_robot, 0.29)[0]


def store_raw(seed):
    """the same store before the enlargement, in the values the enlargement reads (free 68/256, occupied 253/256)"""
    from robot_mpcs_amd.global_planner import png_values, shelf_map
    return png_values(shelf_map(41, 41, seed))


def store_ends(data, B, seed, goals=16):
    """B (start, goal) pairs of distinct free cells, the goals drawn from ``goals`` cells"""
    rng = np.random.default_rng(1000 + seed)
    free = np.flatnonzero((data < OCC).ravel())
    g = rng.choice(free, goals, replace=False)
    gi = rng.integers(0, goals, B)
    goal, start = g[gi], rng.choice(free, B)
    start = np.where(start == goal, g[(gi + 1) % goals], start)
    return start.astype(np.int32), goal.astype(np.int32)


def dense_routes(data, starts, goals, max_len=None):
    """(paths (B, max_len) int32 padded with 0, lens (B,) int32): the planner's restatement, one field per goal"""
    from global_planner_reference import descend_ref, field_ref
    H, W = data.shape
    max_len = max_len or min(H * W, 4 * (H + W))
    fields = {int(g): field_ref(data, int(g)) for g in np.unique(goals)}
    paths, lens = np.zeros((len(starts), max_len), dtype=np.int32), np.zeros(len(starts), dtype=np.int32)
    for b, (s, g) in enumerate(zip(starts.tolist(), goals.tolist())):
        D = fields[g]
        if np.isfinite(D[s // W, s % W]):
            p = descend_ref(data, D, s, g)
            paths[b, :len(p)], lens[b] = p, len(p)
    return paths, lens


_STORE = {}


def store_case(seed, B=64):
    """(data, paths, lens) of the store map ``seed`` with B dense routes; computed once and shared, not to be changed"""
    if (seed, B) not in _STORE:
        data = store_data(seed)
        _STORE[(seed, B)] = (data,) + dense_routes(data, *store_ends(data, B, seed))
    return _STORE[(seed, B)]


def keep_flags(paths, lens, seed=30, share=0.08):
    """flags on a share of every path's cells, 0 past its end"""
    rng = np.random.default_rng(seed)
    k = (rng.uniform(size=paths.shape) < share).astype(np.int32) * rng.integers(1, 4, size=paths.shape).astype(np.int32)
    return k * (np.arange(paths.shape[1])[None, :] < lens[:, None])


def scripted_positions(paths, lens, W, x0, y0, cell, calls, seed=31):
    """(calls, B, 3) positions: every robot moves along its route by a seeded stride per call, displaced by a seeded
    offset of up to two cells; every seventh robot leaves the map for a few calls, one holds a NaN once"""
    rng = np.random.default_rng(seed)
    B = paths.shape[0]
    at = np.zeros(B)
    pos = np.zeros((calls, B, 3))
    for t in range(calls):
        at = np.minimum(at + rng.uniform(0.0, 3.0, B), np.maximum(lens, 1) - 1)
        c = paths[np.arange(B), at.astype(int)]
        off = rng.choice([0.0, 0.2, 0.9, 2.0], size=(B, 1)) * rng.uniform(-1.0, 1.0, size=(B, 2)) * cell
        pos[t, :, 0], pos[t, :, 1] = x0 + (c % W) * cell + off[:, 0], y0 + (c // W) * cell + off[:, 1]
        if t % 9 in (3, 4):
            pos[t, ::7, 0] += 100.0 * (1 if t % 2 else -1)
    pos[5, 1, 1] = np.nan
    return pos
