"""The cases the traffic tests share (tests/test_traffic_cpu.py, tests/test_gpu_traffic.py): the maps at the sizes where
the field kernel changes its layout, seeded flow tables of four kinds, the goal lists, the fleet of 24 robots on the
21 x 21 store of the rule's prototype, and the hand case of the swap."""
import numpy as np

from robot_mpcs_amd.global_planner import shelf_map
from traffic_reference import free_cells, make_costs

OCC = 0.8
# the sizes of the field kernel: one cell, one row, one column, runs of one cell (1024 cells), just above 1024 cells
# (runs of 3, the last threads without a cell), the store's 41 x 41, an odd size below the limit and the limit (runs of 17)
SIZES = [(1, 1), (1, 37), (37, 1), (32, 32), (25, 41), (41, 41), (127, 129), (128, 128)]
FLOWS = ["empty", "below", "above", "negative"]
COSTS = make_costs()                                                    # the defaults: caps 32 and 15
UNIT = make_costs(1, 1, 0, 0, 0, 0)                                     # what rmpc_grid_fields_device prices at factor 0


def field_map(H, W):
    """a map of the size with a region no route leads out of (where the size has room for one)"""
    if H >= 21 and W >= 21:
        g = shelf_map(H, W, seed=H + W)
        g[2:7, 2] = g[2:7, 6] = g[2, 2:7] = g[6, 2:7] = 1.0              # a walled box: its inside is free and unreachable
        g[3:6, 3:6] = 0.0
        g[10, 1:4] = np.nan                                              # a NaN is occupied
        return g
    g = np.zeros((H, W))
    if H * W >= 37:
        g.flat[5] = 1.0                                                  # cuts the row or column: cells 0 .. 4 are apart
        g.flat[20] = np.nan
    return g


def serpentine_map(H, W):
    """every other row a wall with one gap, at alternating ends: one lane through the whole map, so a field needs about
    as many sweeps as the lane has cells divided by a thread's run"""
    g = np.zeros((H, W))
    for i, r in enumerate(range(1, H, 2)):
        g[r, :] = 1.0
        g[r, W - 1 if i % 2 == 0 else 0] = 0.0
    return g


def flow_table(kind, H, W, seed=0, costs=COSTS):
    """a seeded flow table [9][H][W] int32: empty, below the caps, far above them, or with negative entries"""
    rng = np.random.default_rng([seed, H, W, FLOWS.index(kind)])
    f = np.zeros((9, H, W), np.int32)
    if kind == "below":
        f[:8] = rng.integers(0, costs["cap_contra"] + 1, (8, H, W)) * (rng.random((8, H, W)) < 0.3)
        f[8] = rng.integers(0, costs["cap_visit"] + 1, (H, W)) * (rng.random((H, W)) < 0.5)
    elif kind == "above":
        f[:8] = rng.integers(0, 4 * costs["cap_contra"] + 5, (8, H, W))
        f[8] = rng.integers(0, 20 * costs["cap_visit"] + 50, (H, W))
    elif kind == "negative":
        f[:] = rng.integers(-4, 6, (9, H, W))
    return f


def goal_list(grid, G, seed=0):
    """G goal cells: free ones, and for G >= 4 an occupied one, one below 0 and one past the map among them"""
    H, W = grid.shape
    rng = np.random.default_rng([seed, H, W, G])
    free = np.flatnonzero(free_cells(grid, OCC).ravel())
    goals = rng.choice(free, G, replace=len(free) < G).astype(np.int32)
    if G >= 4:
        occ = np.flatnonzero(~free_cells(grid, OCC).ravel())
        goals[1], goals[G // 2], goals[G - 1] = occ[len(occ) // 2], -1, H * W
    return goals


def fleet_case(B=24, H=21, W=21, seed=0):
    """(grid, starts, goals): B robots on the H x W store, distinct free start cells and distinct free goal cells, every
    goal reachable (the store's free cells are connected)"""
    grid = shelf_map(H, W, seed=seed, aisle=3, shelf=2, gap=2)
    rng = np.random.default_rng(seed + 1)
    free = np.flatnonzero(free_cells(grid, OCC).ravel())
    cells = rng.choice(free, 2 * B, replace=False).astype(np.int32)
    return grid, cells[:B], cells[B:]


def swap_case():
    """the hand case: a 3 x 7 open map, two robots swap the ends of the middle row; movement 4, bases 1, w_visit 0,
    w_contra 5"""
    return np.zeros((3, 7)), np.array([7, 13], np.int32), np.array([13, 7], np.int32), make_costs(1, 1, 0, 0, 5, 15)
