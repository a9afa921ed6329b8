"""The cases the CBS test modules share (tests/test_cbs_cpu.py asserts the outcome of every one, tests/test_gpu_cbs.py
holds the device to ``cbs_ref`` on them): name -> dict(grid, starts, goals, T, sep2, lag, movement, nodes, expand, rounds)
and ``want``, the outcome the restatement must reach.  Only the budget cases (``BUDGET``) may end unsolved."""
import numpy as np

from cbs_reference import INFEASIBLE, POOL, ROUNDS, SOLVED


def bay():
    """3 x 7: the middle row is a corridor, the only bay lies above its middle column"""
    g = np.ones((3, 7))
    g[1, :] = 0.0
    g[0, 3] = 0.0
    return g


def _case(grid, starts, goals, T, sep2, lag=1, movement=4, nodes=4096, expand=1, rounds=4096, want=SOLVED):
    return dict(grid=np.asarray(grid, dtype=float), starts=np.asarray(starts), goals=np.asarray(goals), T=T, sep2=sep2,
                lag=lag, movement=movement, nodes=nodes, expand=expand, rounds=rounds, want=want)


def random_case(seed, H, W, B, T, sep2, lag, movement, density=0.15, spacing=None, **kw):
    """B robots on a random H x W map: starts pairwise at least ``spacing`` (squared cells, sep2 by default) apart, goals
    too, all on free cells"""
    rng = np.random.default_rng(seed)
    spacing = sep2 if spacing is None else spacing
    g = (rng.uniform(size=(H, W)) < density).astype(float)
    free = rng.permutation(np.flatnonzero(g.ravel() < 0.5))
    d2 = lambda a, b: (a // W - b // W) ** 2 + (a % W - b % W) ** 2
    starts, goals = [], []
    for c in free:
        if len(starts) < B and all(d2(c, q) >= spacing for q in starts):
            starts.append(int(c))
    for c in free[::-1]:
        if len(goals) < B and all(d2(c, q) >= spacing for q in goals):
            goals.append(int(c))
    assert len(starts) == B and len(goals) == B, "the map has no room for the robots"
    return _case(g, starts, goals, T, sep2, lag, movement, **kw)


def shelves(H, W):
    """free aisles every third row and at both ends of the rows"""
    g = np.zeros((H, W))
    for r in range(1, H - 1):
        if r % 3:
            g[r, 2:W - 2] = 1.0
    return g


HAND = {
    # two robots swapping the corridor's ends: both priority orders fail, the joint optimum is 18
    "bay": _case(bay(), [7, 13], [13, 7], 12, 1),
    # 1 x 7 swap at a small window: there is no bay, nobody can arrive, and the optimum is two late robots kept apart
    "swap_1x7": _case(np.zeros((1, 7)), [0, 6], [6, 0], 4, 1),
    # 1 x 2 with sep2 2: wherever robot 1 stands at layer 1 it conflicts with robot 0 on its start at layer 0
    "infeasible": _case(np.zeros((1, 2)), [0, 1], [1, 0], 3, 2, want=INFEASIBLE),
    # two robots whose starts conflict: (0, 0) is exempt, the layers (0, 1) and (1, 0) are not
    "close_starts": _case(np.zeros((3, 4)), [4, 5], [7, 1], 6, 2),
    # a robot outside the map between two that meet head on in a 2 x 5
    "skipped": _case(np.zeros((2, 5)), [0, -1, 4], [4, 7, 0], 7, 1),
}

# the device cases beside the hand cases
DEVICE = {
    "7x5_B3": random_case(3, 7, 5, 3, 10, 2, 1, 4),
    "12x12_B4": random_case(5, 12, 12, 4, 26, 4, 2, 8),
    "65x70_T40": _case(shelves(65, 70), [0, 24 * 70 + 1, 12 * 70 + 20], [24 * 70, 1, 12 * 70], 40, 2, expand=2, nodes=1024),
    "65x70_T70": _case(shelves(65, 70), [0, 69, 32 * 70], [30 * 70 + 35, 30 * 70 + 33, 30 * 70 + 37], 70, 2),
    "4x130": _case(np.zeros((4, 130)), [130 + 60, 130 + 69, 64], [130 + 69, 130 + 60, 3 * 130 + 64], 14, 2, movement=8),
    "T1": _case(np.zeros((3, 3)), [0, 2], [1, 1], 1, 1),
    "B1": _case(bay(), [7], [13], 12, 1),
    "nan_cell": None,       # filled below: the bay case with a NaN on the corridor (a NaN is free)
    "pool": _case(bay(), [7, 13], [13, 7], 12, 1, nodes=20, want=POOL),
    "rounds": _case(bay(), [7, 13], [13, 7], 12, 1, rounds=7, want=ROUNDS),
}
_g = bay()
_g[1, 2] = np.nan
DEVICE["nan_cell"] = _case(_g, [7, 13], [13, 7], 12, 1)

BUDGET = ("pool", "rounds")
CASES = dict(HAND, **DEVICE)


def problem(case):
    """(goal_cells, goal_index) of a case: the distinct goals and every robot's index into them; a goal outside the map
    keeps an index outside [0, Gf) so that its robot is skipped"""
    goals = np.asarray(case["goals"])
    HW = case["grid"].size
    inside = (goals >= 0) & (goals < HW)
    goal_cells = np.unique(goals[inside]).astype(np.int32)
    gi = np.where(inside, np.searchsorted(goal_cells, np.where(inside, goals, goal_cells[0])), -1).astype(np.int32)
    return goal_cells, gi
