"""Conflict-based search over the timed routes, restated on the CPU from include/rmpc_cbs.h: ``cbs_ref`` is the rule as
written (boolean layers, the batch of ``expand`` nodes per round, ids, slices); ``joint_optimum``, written apart from it,
is an exhaustive search over the robots' joint cells.  tests/test_cbs_cpu.py holds the two against each other and against
hand-worked cases, tests/test_gpu_cbs.py holds the device against ``cbs_ref`` bit for bit.  Grids, cells and moves are
those of tests/timed_reference.py."""
import itertools

import numpy as np

from global_planner_reference import MOVES
from timed_reference import OUTSIDE, _arrive, _d2, _end_cell, _skipped

SOLVED, INFEASIBLE, POOL, ROUNDS, BAD_STATE = 1, 2, 3, 4, 5
INF = 2 ** 31 - 1
INFO = ("outcome", "node", "conflict_free", "cost", "bound", "created", "expanded", "rounds_run")
OPEN, SOLUTION, EXPANDED = 1, 2, 3


class CbsSearch:
    """The state of one search: ``run(rounds)`` is one call (the first one makes the root), ``result`` its outputs."""

    def __init__(self, grid, start, goal_index, fields, goal_cells, T, sep2, lag=1, movement=4, occ=0.8, nodes=4096,
                 expand=1):
        self.grid = np.asarray(grid, dtype=float)
        self.H, self.W = self.grid.shape
        self.start, self.gi = [int(s) for s in start], [int(g) for g in goal_index]
        self.fields, self.goal_cells = fields, goal_cells
        self.B, self.T, self.sep2, self.lag, self.M, self.E = len(self.start), T, sep2, lag, nodes, expand
        self.free = ~(self.grid >= occ)
        self.moves = [(dc, dr) for dc, dr, _ in MOVES[movement]]
        self.skipped = [_skipped(s, g, self.H * self.W, len(fields)) for s, g in zip(self.start, self.gi)]
        self.rows, self.cols = np.mgrid[0:self.H, 0:self.W]
        self.node, self.expanded, self.rounds_run, self.created, self.outcome = {}, 0, 0, 0, 0

    def disc(self, c):
        return (self.rows - c // self.W) ** 2 + (self.cols - c % self.W) ** 2 < self.sep2

    def route(self, b, table):
        """(path, arrive) of robot b under the boolean table (T + 1, H, W), None when the route does not exist"""
        H, W, T = self.H, self.W, self.T
        s, gi = self.start[b], self.gi[b]
        reach = np.zeros((T + 1, H, W), dtype=bool)
        reach[0, s // W, s % W] = True
        for t in range(1, T + 1):
            pad = np.pad(reach[t - 1], 1)
            n = reach[t - 1].copy()
            for dc, dr in self.moves:
                n |= pad[1 - dr:1 - dr + H, 1 - dc:1 - dc + W]
            n &= self.free & ~table[t]
            reach[t] = n
            if not n.any():
                return None
        end = _end_cell(np.flatnonzero(reach[T].ravel()), np.asarray(self.fields[gi]).ravel())
        p = np.full(T + 1, end, dtype=np.int32)
        c = end
        for t in range(T, 0, -1):
            r, col = divmod(c, W)
            if not reach[t - 1, r, col]:
                for dc, dr in self.moves:
                    rr, cc = r - dr, col - dc
                    if 0 <= rr < H and 0 <= cc < W and reach[t - 1, rr, cc]:
                        c = rr * W + cc
                        break
            p[t - 1] = c
        return p, _arrive(p, int(self.goal_cells[gi]), T)

    def table(self, n, b):
        """robot b's table in node n: the constraints on b along the chain to the root"""
        table = np.zeros((self.T + 1, self.H, self.W), dtype=bool)
        while n is not None:
            con = n["con"]
            if con is not None and con[1] == b:
                kind, _, s, v = con
                if kind == 0:
                    table[max(1, s - self.lag):min(self.T, s + self.lag) + 1] |= self.disc(v)
                else:
                    table[s, v // self.W, v % self.W] = True
            n = self.node.get(n["parent"])
        return table

    def conflict(self, paths):
        """the least (min(t, s), i, j, t, s) as (i, t, j, s), None without one"""
        best = None
        live = [b for b in range(self.B) if not self.skipped[b]]
        for a, i in enumerate(live):
            for j in live[a + 1:]:
                for t in range(self.T + 1):
                    if best is not None and t - self.lag > best[0]:
                        break
                    for s in range(max(0, t - self.lag), min(self.T, t + self.lag) + 1):
                        if (t, s) != (0, 0) and _d2(int(paths[i, t]), int(paths[j, s]), self.W) < self.sep2:
                            key = (min(t, s), i, j, t, s)
                            if best is None or key < best:
                                best = key
        return None if best is None else (best[1], best[3], best[2], best[4])

    def _add(self, nid, parent, con, paths, arrive):
        conflict = self.conflict(paths)
        self.node[nid] = dict(parent=parent, con=con, paths=paths, arrive=arrive, cost=int(arrive.sum()),
                              conflict=conflict, state=SOLUTION if conflict is None else OPEN)
        self.created += 1

    def _root(self):
        paths = np.full((self.B, self.T + 1), -1, dtype=np.int32)
        arrive = np.full(self.B, self.T + 1, dtype=np.int32)
        empty = np.zeros((self.T + 1, self.H, self.W), dtype=bool)
        for b in range(self.B):
            if not self.skipped[b]:
                r = self.route(b, empty)
                if r is None:
                    return                      # the root is dead
                paths[b], arrive[b] = r
        self._add(0, None, None, paths, arrive)

    def _child(self, nid, pid, kind, b, s, v):
        parent = self.node[pid]
        child = dict(parent=pid, con=(kind, b, s, v))
        r = self.route(b, self.table(child, b))
        if r is None:
            return
        paths, arrive = parent["paths"].copy(), parent["arrive"].copy()
        paths[b], arrive[b] = r
        self._add(nid, pid, (kind, b, s, v), paths, arrive)

    def _ends(self):
        """(the incumbent's id or None, the open ids sorted by (cost, id))"""
        sol = sorted((n["cost"], k) for k, n in self.node.items() if n["state"] == SOLUTION)
        opn = sorted((n["cost"], k) for k, n in self.node.items() if n["state"] == OPEN)
        return (sol[0][1] if sol else None), [k for _, k in opn]

    def run(self, rounds, resume=False):
        if not resume:
            self._root()
        self.outcome = 0
        for _ in range(rounds):
            inc, opn = self._ends()
            lo = self.node[opn[0]]["cost"] if opn else INF
            if inc is not None and self.node[inc]["cost"] <= lo:
                self.outcome = SOLVED
                break
            if not opn and inc is None:
                self.outcome = INFEASIBLE
                break
            take = [k for k in opn if inc is None or self.node[k]["cost"] < self.node[inc]["cost"]][:self.E]
            if 2 * (self.expanded + len(take)) >= self.M:
                self.outcome = POOL
                break
            for k in take:
                x, n = self.expanded, self.node[k]
                i, t, j, s = n["conflict"]
                v = int(n["paths"][j, s])
                n["state"] = EXPANDED
                self.expanded += 1
                if t >= 1:
                    self._child(1 + 2 * x, k, 0, i, s, v)
                if s >= 1:
                    self._child(2 + 2 * x, k, 1, j, s, v)
            self.rounds_run += 1
        else:
            self.outcome = ROUNDS
        return self.result()

    def result(self):
        inc, opn = self._ends()
        k = inc if inc is not None else (opn[0] if opn else None)
        B, T = self.B, self.T
        out = dict(paths=np.full((B, T + 1), -1, dtype=np.int32), arrive=np.full(B, T + 1, dtype=np.int32),
                   status=np.array([OUTSIDE if sk else 0 for sk in self.skipped], dtype=np.int32))
        lo = self.node[opn[0]]["cost"] if opn else INF
        bound = min(lo, self.node[inc]["cost"] if inc is not None else INF)
        info = dict(outcome=self.outcome, node=-1 if k is None else k, conflict_free=int(inc is not None),
                    cost=INF if k is None else self.node[k]["cost"], bound=bound, created=self.created,
                    expanded=self.expanded, rounds_run=self.rounds_run)
        if k is not None:
            out["paths"], out["arrive"] = self.node[k]["paths"].copy(), self.node[k]["arrive"].copy()
        out["info"] = np.array([info[n] for n in INFO], dtype=np.int32)
        out.update(info)
        return out


def cbs_ref(grid, start, goal_index, fields, goal_cells, T, sep2, lag=1, movement=4, occ=0.8, nodes=4096, expand=1,
            rounds=4096, slices=None):
    """One search: dict(paths (B, T + 1), status, arrive (B,), info (8,) int32, and info's members by name).  ``slices``:
    the rounds of the first call and of every resumed one behind it, in place of ``rounds``."""
    search = CbsSearch(grid, start, goal_index, fields, goal_cells, T, sep2, lag, movement, occ, nodes, expand)
    out = None
    for k, r in enumerate([rounds] if slices is None else slices):
        out = search.run(r, resume=k > 0)
    return out


# ---- the exhaustive search, written apart -----------------------------------------------------------------------------
def joint_optimum(grid, start, goal_index, goal_cells, T, sep2, lag=1, movement=4, occ=0.8, n_fields=None):
    """The least sum of arrive over all conflict-free sets of paths of the window, None when there is none.  Layer by
    layer from T backwards over states (the joint cells of the layers t .. t + lag - 1, a flag per robot: "off its goal
    at a later layer"): a robot that is off its goal at t and has no flag arrives at t + 1, which is charged there and
    sets the flag; one that never leaves its goal arrives at 0.  Skipped robots count T + 1 each."""
    grid = np.asarray(grid, dtype=float)
    H, W = grid.shape
    n_fields = len(goal_cells) if n_fields is None else n_fields
    live = [b for b in range(len(start)) if not _skipped(int(start[b]), int(goal_index[b]), H * W, n_fields)]
    base = (T + 1) * (len(start) - len(live))
    if not live:
        return base
    S = [int(start[b]) for b in live]
    Gc = [int(goal_cells[int(goal_index[b])]) for b in live]
    n = len(live)
    free = [not (grid[c // W, c % W] >= occ) for c in range(H * W)]
    steps = [(0, 0)] + [(dc, dr) for dc, dr, _ in MOVES[movement]]

    def before(c):                      # the cells a robot can have stood on one layer before c
        r, col = divmod(c, W)
        return [(r - dr) * W + col - dc for dc, dr in steps if 0 <= r - dr < H and 0 <= col - dc < W]

    # forward: the cells each robot can stand on at layer t with nobody else on the map
    can = [[{S[k]}] for k in range(n)]
    for k in range(n):
        for t in range(1, T + 1):
            can[k].append({c for c in range(H * W) if free[c] and any(q in can[k][t - 1] for q in before(c))})
    near = lambda a, b: _d2(a, b, W) < sep2

    def clash(x, t, window):
        """joint cells x at layer t against themselves and the later layers of the window (window[0] is layer t + 1)"""
        for a in range(n):
            for b in range(n):
                if a == b:
                    continue
                if a < b and t > 0 and near(x[a], x[b]):
                    return True
                for later in window:
                    if near(x[a], later[b]):
                        return True
        return False

    charge = lambda x, t, flags: (sum(t + 1 for k in range(n) if x[k] != Gc[k] and not flags[k]),
                                  tuple(flags[k] or x[k] != Gc[k] for k in range(n)))
    value = {}
    for x in itertools.product(*[sorted(can[k][T]) for k in range(n)]):
        if not clash(x, T, ()):
            c, flags = charge(x, T, (False,) * n)
            value[((x,), flags)] = c
    for t in range(T - 1, -1, -1):
        nxt = {}
        for (window, flags), cost in value.items():
            options = [[q for q in before(window[0][k]) if q in can[k][t]] for k in range(n)]
            for x in itertools.product(*options):
                if clash(x, t, window[:lag]):
                    continue
                c, f2 = charge(x, t, flags)
                key = (((x,) + window)[:max(lag, 1)], f2)
                if cost + c < nxt.get(key, INF):
                    nxt[key] = cost + c
        value = nxt
    best = [c for (window, _), c in value.items() if list(window[0]) == S]
    return base + min(best) if best else None
