"""Focal conflict-based search over the timed routes, restated on the CPU from include/rmpc_ecbs.h: ``ecbs_ref`` is the
rule as written -- the penalty table, the focal route's layer recursion, candidate arrivals and backtrack, the nodes' lbs
and nconf, Lo over open and solution nodes, FOCAL and its order -- on top of ``CbsSearch`` of tests/cbs_reference.py,
whose route under a table, tables, ids and slices it uses as they are.  It asserts on every node that
cost * w_den <= w_num * lb and in every round that FOCAL is not empty.  tests/test_ecbs_cpu.py holds it against hand-worked
cases, ``cbs_ref`` and ``joint_optimum``; tests/test_gpu_ecbs.py holds the device against it bit for bit."""
import numpy as np

from cbs_reference import BAD_STATE, EXPANDED, INF, INFEASIBLE, OPEN, POOL, ROUNDS, SOLUTION, SOLVED, CbsSearch  # noqa: F401
from timed_reference import OUTSIDE, _arrive, _end_cell

INFO = ("outcome", "node", "conflict_free", "cost", "bound", "created", "expanded", "rounds_run", "lb", "nconf")
BIG = 2 ** 30          # a cost no cell of a layer has


class EcbsSearch(CbsSearch):
    """``CbsSearch`` with the weight ``w = (w_num, w_den)``.  ``late`` counts the focal routes that arrived after their
    least arrive, ``routes`` all of them."""

    def __init__(self, *a, w=(1, 1), **kw):
        super().__init__(*a, **kw)
        self.wn, self.wd = int(w[0]), int(w[1])
        assert 1 <= self.wd <= 1024 and self.wd <= self.wn <= 4 * self.wd
        self.late = self.routes = self.repasses = 0

    # ---- the focal route -------------------------------------------------------------------------------------------------
    def layers(self, b, table):
        """reach (T + 1, H, W) of robot b under the table, None when a layer is empty (the sweep of ``CbsSearch.route``)"""
        H, W, T = self.H, self.W, self.T
        s = self.start[b]
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
        return reach

    def shortest(self, b, reach):
        """(p, a) of ROUTE UNDER A TABLE from its layers: the end cell and the backtrack of ``CbsSearch.route``"""
        H, W, T = self.H, self.W, self.T
        gi = self.gi[b]
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

    def penalty(self, others):
        """pen (T + 1, H, W) against the paths ``others`` (each (T + 1,))"""
        T, lag = self.T, self.lag
        at = np.zeros((T + 1, self.H, self.W), dtype=np.int64)       # at[s]: the robots of O whose cell at s conflicts
        for p in others:
            for s in range(T + 1):
                at[s] += self.disc(int(p[s]))
        pen = np.zeros_like(at)
        for t in range(T + 1):
            for s in range(max(0, t - lag), min(T, t + lag) + 1):
                if (t, s) != (0, 0):
                    pen[t] += at[s]
        return pen

    def focal_route(self, b, table, others):
        """(path, arrive, lb) of robot b, None when the route does not exist"""
        H, W, T = self.H, self.W, self.T
        reach = self.layers(b, table)
        if reach is None:
            return None
        p, a = self.shortest(b, reach)
        self.routes += 1
        if a == T + 1:
            return p, a, a
        A = min(T, self.wn * a // self.wd)
        pen = self.penalty(others)
        s, g = self.start[b], int(self.goal_cells[self.gi[b]])
        gr, gc = divmod(g, W)
        hold = np.cumsum(pen[::-1, gr, gc])[::-1]
        steps = [(0, 0)] + list(self.moves)                 # the wait, then the moves in order
        c = np.full((A + 1, H, W), BIG, dtype=np.int64)
        frm = np.zeros((A + 1, H, W), dtype=np.int8)
        c[0, s // W, s % W] = pen[0, s // W, s % W]
        for t in range(1, A + 1):
            pad = np.pad(c[t - 1], 1, constant_values=BIG)
            prev = np.stack([pad[1 - dr:1 - dr + H, 1 - dc:1 - dc + W] for dc, dr in steps])
            frm[t] = np.argmin(prev, axis=0)                # the first that attains the minimum
            least = prev.min(axis=0)
            assert np.all(least[reach[t]] < BIG)            # a cell of reach[t] has an origin in reach[t - 1]
            c[t] = np.where(reach[t], pen[t] + least, BIG)
        best = None
        for a2 in range(a, A + 1):
            assert reach[a2, gr, gc]
            if a2 == 0:
                key = (int(hold[0]), 0, -1)
            else:
                origin = [(int(c[a2 - 1, gr - dr, gc - dc]), m) for m, (dc, dr) in enumerate(self.moves)
                          if 0 <= gr - dr < H and 0 <= gc - dc < W and c[a2 - 1, gr - dr, gc - dc] < BIG]
                if not origin:
                    continue
                least, m = min(origin)                      # the first move in order that attains it
                key = (least + int(hold[a2]), a2, m)
            if best is None or key[:2] < best[:2]:
                best = key
        assert best is not None                             # a2 = a exists
        total, a2, m = best
        path = np.full(T + 1, g, dtype=np.int32)
        if a2 >= 1:
            dc, dr = self.moves[m]
            r, col = gr - dr, gc - dc
            path[a2 - 1] = r * W + col
            for t in range(a2 - 1, 0, -1):
                dc, dr = steps[frm[t, r, col]]
                r, col = r - dr, col - dc
                path[t - 1] = r * W + col
            assert path[0] == s
        assert _arrive(path, g, T) == a2 and a2 * self.wd <= self.wn * a
        assert all(reach[t, path[t] // W, path[t] % W] for t in range(T + 1))
        self.late += a2 > a
        return path, a2, a

    # ---- nodes -----------------------------------------------------------------------------------------------------------
    def conflict_count(self, paths):
        """(the least conflict as ``CbsSearch.conflict`` gives it, the number of tuples (i < j, t, s))"""
        T, lag, W = self.T, self.lag, self.W
        live = [b for b in range(self.B) if not self.skipped[b]]
        best, n = None, 0
        if len(live) >= 2:
            P = paths[live].astype(np.int64)
            R, Cc = P // W, P % W
            for ds in range(-lag, lag + 1):
                t = np.arange(max(0, -ds), min(T, T - ds) + 1)
                d2 = (R[:, None, t] - R[None, :, t + ds]) ** 2 + (Cc[:, None, t] - Cc[None, :, t + ds]) ** 2
                hit = d2 < self.sep2
                if ds == 0:
                    hit[:, :, 0] &= t[0] != 0
                ii, jj, kk = np.nonzero(hit)
                for i, j, k in zip(ii[ii < jj], jj[ii < jj], kk[ii < jj]):
                    n += 1
                    key = (min(int(t[k]), int(t[k]) + ds), live[i], live[j], int(t[k]), int(t[k]) + ds)
                    if best is None or key < best:
                        best = key
        return (None if best is None else (best[1], best[3], best[2], best[4])), n

    def _put(self, nid, parent, con, paths, arrive, lbs):
        conflict, nconf = self.conflict_count(paths)
        n = dict(parent=parent, con=con, paths=paths, arrive=arrive, lbs=lbs, cost=int(arrive.sum()), lb=int(lbs.sum()),
                 nconf=nconf, conflict=conflict, state=SOLUTION if conflict is None else OPEN)
        assert n["cost"] * self.wd <= self.wn * n["lb"], (nid, n["cost"], n["lb"])
        assert parent is None or n["lb"] >= self.node[parent]["lb"]
        self.node[nid] = n
        self.created += 1

    def _root(self):
        B, T = self.B, self.T
        paths = np.full((B, T + 1), -1, dtype=np.int32)
        arrive = np.full(B, T + 1, dtype=np.int32)
        lbs = np.full(B, T + 1, dtype=np.int32)
        empty = np.zeros((T + 1, self.H, self.W), dtype=bool)
        routed = []
        for b in range(B):
            if not self.skipped[b]:
                r = self.focal_route(b, empty, [paths[j] for j in routed])
                if r is None:
                    return                      # the root is dead
                paths[b], arrive[b], lbs[b] = r
                routed.append(b)
        self._put(0, None, None, paths, arrive, lbs)

    def _child(self, nid, pid, kind, b, s, v):
        parent = self.node[pid]
        child = dict(parent=pid, con=(kind, b, s, v))
        others = [parent["paths"][j] for j in range(self.B) if j != b and not self.skipped[j]]
        r = self.focal_route(b, self.table(child, b), others)
        if r is None:
            return
        paths, arrive, lbs = parent["paths"].copy(), parent["arrive"].copy(), parent["lbs"].copy()
        paths[b], arrive[b], lbs[b] = r
        self._put(nid, pid, (kind, b, s, v), paths, arrive, lbs)

    def _state(self):
        """(the incumbent's id or None, the open ids, Lo)"""
        sol = sorted((n["cost"], k) for k, n in self.node.items() if n["state"] == SOLUTION)
        opn = [k for k, n in self.node.items() if n["state"] == OPEN]
        lo = min([n["lb"] for n in self.node.values() if n["state"] in (OPEN, SOLUTION)], default=INF)
        return (sol[0][1] if sol else None), opn, lo

    def _rank(self, ids):
        return sorted(ids, key=lambda k: (self.node[k]["nconf"], self.node[k]["cost"], k))

    def _passes(self, ranked, lists=256, keep=2):
        """how many passes k_ecbs_select needs for the first E of ``ranked``: the ids are dealt to ``lists`` threads by
        id % lists, a thread keeps its ``keep`` least per pass, and a pass ends before the least key that was let go.
        The result does not depend on it; the count tells a test whether it reached the second pass."""
        n, passes = 0, 0
        while n < min(self.E, len(ranked)):
            held, stop = {}, len(ranked)
            for pos in range(n, len(ranked)):
                t = ranked[pos] % lists
                held[t] = held.get(t, 0) + 1
                if held[t] > keep:
                    stop = pos
                    break
            n = min(stop, self.E, len(ranked))
            passes += 1
        return passes

    def run(self, rounds, resume=False):
        if not resume:
            self._root()
        self.outcome = 0
        wn, wd = self.wn, self.wd
        for _ in range(rounds):
            inc, opn, lo = self._state()
            if inc is not None and self.node[inc]["cost"] * wd <= wn * lo:
                self.outcome = SOLVED
                break
            if not opn and inc is None:
                self.outcome = INFEASIBLE
                break
            focal = [k for k in opn if self.node[k]["cost"] * wd <= wn * lo
                     and (inc is None or self.node[k]["cost"] < self.node[inc]["cost"])]
            assert focal, "FOCAL is empty"
            ranked = self._rank(focal)
            take = ranked[:self.E]
            self.repasses += self._passes(ranked) - 1
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
        inc, opn, lo = self._state()
        k = inc if inc is not None else (self._rank(opn)[0] if opn else None)
        B, T = self.B, self.T
        out = dict(paths=np.full((B, T + 1), -1, dtype=np.int32), arrive=np.full(B, T + 1, dtype=np.int32),
                   status=np.array([OUTSIDE if sk else 0 for sk in self.skipped], dtype=np.int32))
        n = None if k is None else self.node[k]
        info = dict(outcome=self.outcome, node=-1 if k is None else k, conflict_free=int(inc is not None),
                    cost=INF if n is None else n["cost"], bound=lo, created=self.created, expanded=self.expanded,
                    rounds_run=self.rounds_run, lb=INF if n is None else n["lb"], nconf=0 if n is None else n["nconf"])
        if n is not None:
            out["paths"], out["arrive"] = n["paths"].copy(), n["arrive"].copy()
        out["info"] = np.array([info[m] for m in INFO], dtype=np.int32)
        out.update(info, late=self.late, routes=self.routes, repasses=self.repasses)
        return out


def ecbs_ref(grid, start, goal_index, fields, goal_cells, T, sep2, lag=1, movement=4, occ=0.8, nodes=4096, expand=1,
             rounds=4096, slices=None, w=(1, 1)):
    """One search: dict(paths (B, T + 1), status, arrive (B,), info (10,) int32, info's members by name, ``late`` /
    ``routes``: the focal routes that arrived after their least arrive, and all, and ``repasses``: the further passes the
    device's selection needs).  ``slices`` as in ``cbs_ref``."""
    search = EcbsSearch(grid, start, goal_index, fields, goal_cells, T, sep2, lag, movement, occ, nodes, expand, w=w)
    out = None
    for k, r in enumerate([rounds] if slices is None else slices):
        out = search.run(r, resume=k > 0)
    return out
