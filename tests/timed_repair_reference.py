"""The repair of failing priority orders (include/rmpc_timed_repair.h) restated on the CPU on top of
``plan_ref`` of tests/timed_reference.py: every round is one call of ``plan_ref`` on one order, and what happens between
two rounds is list work.  tests/test_timed_repair_cpu.py holds it to hand-worked cases and to the properties that follow
from the rule, tests/test_gpu_timed_repair.py holds the device to it bit for bit."""
import numpy as np

from timed_reference import BAD_ORDER, INT64_MAX, _is_permutation, plan_ref


def bad_robots(status, arrive, T):
    """rule 3: failed, or planned and not at its goal by T; a skipped robot (status < 0) is never bad"""
    status, arrive = np.asarray(status), np.asarray(arrive)
    return (status > 0) | ((status == 0) & (arrive > T))


def next_order(order, bad):
    """rule 4: the bad robots in their rank order, then the others in theirs"""
    return [b for b in order if bad[b]] + [b for b in order if not bad[b]]


def repair_ref(grid, start, goal_index, fields, goal_cells, orders, T, sep2, lag=1, movement=4, occ=0.8, rounds=0):
    """The rule of rmpc_timed_plan_repair_device: ``plan_ref``'s dict with order_out (G, B), rounds_run, round_best (G,)
    int32 and, beyond what the device reports, ``keys``: per row the list of every round's key, ``tried``: per row the
    list of every round's order, and ``nbad``: per row the list of every round's number of bad robots."""
    orders = np.atleast_2d(np.asarray(orders))
    G, B = orders.shape
    out = dict(paths=np.full((G, B, T + 1), -1, dtype=np.int32), status=np.full((G, B), BAD_ORDER, dtype=np.int32),
               arrive=np.full((G, B), T + 1, dtype=np.int32), key=np.full(G, INT64_MAX, dtype=np.int64),
               order_out=np.full((G, B), -1, dtype=np.int32), rounds_run=np.zeros(G, dtype=np.int32),
               round_best=np.full(G, -1, dtype=np.int32), keys=[[] for _ in range(G)], tried=[[] for _ in range(G)],
               nbad=[[] for _ in range(G)])
    best = -1
    for g in range(G):
        if not _is_permutation(orders[g], B):
            continue
        order, r = [int(b) for b in orders[g]], 0
        while True:
            one = plan_ref(grid, start, goal_index, fields, goal_cells, [order], T, sep2, lag, movement, occ)
            out["keys"][g].append(int(one["key"][0]))
            out["tried"][g].append(list(order))
            if r == 0 or one["key"][0] < out["key"][g]:            # the least (key, round)
                for k in ("paths", "status", "arrive", "key"):
                    out[k][g] = one[k][0]
                out["order_out"][g], out["round_best"][g] = order, r
            bad = bad_robots(one["status"][0], one["arrive"][0], T)
            out["nbad"][g].append(int(bad.sum()))
            nxt = next_order(order, bad)
            if not bad.any() or r == rounds or nxt == order:
                break
            order, r = nxt, r + 1
        out["rounds_run"][g] = r + 1
        if best < 0 or out["key"][g] < out["key"][best]:
            best = g
    out["best"] = np.array([best], dtype=np.int32)
    return out


# ---- hand-worked maps (tests/test_timed_repair_cpu.py works them out) ----------------------------------------------------
def bay_corridor():
    """3 x 7: a corridor (row 1, cells 7 .. 13) with a one-cell bay above its column 1 (cell 1)"""
    g = np.ones((3, 7))
    g[1, :] = 0.0
    g[0, 1] = 0.0
    return g


def two_by_three():
    """2 x 3 with cell 0 occupied: cells 1 2 over 3 4 5"""
    g = np.zeros((2, 3))
    g[0, 0] = 1.0
    return g
