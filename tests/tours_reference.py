"""The rules of include/rmpc_tours.h restated in numpy, written from the header: the cheapest-insertion build, the
improvement by relocations and exchanges with their orders, and the follower that stops.  ``tours_ref`` is vectorised
over the candidates of a step; ``tours_loop`` is a second, plain restatement that builds every candidate's tours as
Python lists and adds up their edges from scratch -- it knows no delta formula -- and pins the first on small cases.
``quantise`` is the one of the assignment (tests/assign_optimal_reference.py)."""
import numpy as np

from assign_optimal_reference import quantise

MODES = {"sum": 0, "span": 1}
B_SHIFT, T_SHIFT, KIND_SHIFT = 21, 11, 31       # (kind, i, j, l) and (b, t, k) packed in ascending significance
BIG = np.int64(1) << 62


def tour_cost(qs, qt, b, tour):
    """the sum of q along start_b -> tour [0] -> tour [1] -> ..., None when an edge is not takeable"""
    total, prev = 0, None
    for t in tour:
        e = int(qs[b][t]) if prev is None else int(qt[prev][t])
        if e < 0:
            return None
        total += e
        prev = t
    return total


def report(tours, c, B, T, K, build_steps, rounds):
    """the outputs of rmpc_tours_device for one problem"""
    out = dict(tours=np.full((B, K), -1, dtype=np.int32), len=np.zeros(B, dtype=np.int32),
               cost=np.asarray([int(x) for x in c], dtype=np.int64), owner=np.full(T, -1, dtype=np.int32),
               build_steps=int(build_steps), rounds=int(rounds))
    for b, tour in enumerate(tours):
        out["tours"][b, :len(tour)] = tour
        out["len"][b] = len(tour)
        out["owner"][tour] = b
    out["count"], out["total"], out["span"] = int(out["len"].sum()), int(out["cost"].sum()), int(out["cost"].max())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the plain restatement

def _admissible_key(mode, ds, pm_old, pm_new, tail):
    if mode == 0:
        return (ds,) + tail if ds < 0 else None
    if pm_new < pm_old or (pm_new == pm_old and ds < 0):
        return (pm_new - pm_old, ds) + tail
    return None


def tours_loop(qs, qt, K, mode, max_rounds, improve_from=None):
    """qs (B, T), qt (T, T) integer costs with -1 on the edges nobody may take -> report().  ``improve_from``: a list of
    tours to improve instead of building (for tests of the improvement alone)."""
    B, T = len(qs), len(qs[0])
    tours = [[] for _ in range(B)] if improve_from is None else [list(t) for t in improve_from]
    c = [tour_cost(qs, qt, b, tours[b]) for b in range(B)]
    build_steps = 0
    while improve_from is None:
        taken = {t for tour in tours for t in tour}
        best = None
        for b in range(B):
            if len(tours[b]) >= K:
                continue
            for t in range(T):
                if t in taken:
                    continue
                for k in range(len(tours[b]) + 1):
                    cn = tour_cost(qs, qt, b, tours[b][:k] + [t] + tours[b][k:])
                    if cn is None:
                        continue
                    key = ((cn - c[b]) if mode == 0 else cn, b, t, k)
                    if best is None or key < best[0]:
                        best = (key, cn)
        if best is None:
            break
        (_, b, t, k), cn = best
        tours[b].insert(k, t)
        c[b] = cn
        build_steps += 1
    rounds = 0
    while rounds < max_rounds:
        where = {t: (b, p) for b, tour in enumerate(tours) for p, t in enumerate(tour)}
        best = None
        for t, (b1, p1) in sorted(where.items()):
            short = tours[b1][:p1] + tours[b1][p1 + 1:]
            cs = tour_cost(qs, qt, b1, short)
            if cs is None:
                continue
            for b2 in range(B):
                if b2 != b1 and len(tours[b2]) >= K:
                    continue
                base = short if b2 == b1 else tours[b2]
                for k2 in range(len(base) + 1):
                    if b2 == b1 and k2 == p1:
                        continue
                    new = base[:k2] + [t] + base[k2:]
                    cn = tour_cost(qs, qt, b2, new)
                    if cn is None:
                        continue
                    if b2 == b1:
                        key = _admissible_key(mode, cn - c[b1], c[b1], cn, (0, t, b2, k2))
                        after = {b1: (new, cn)}
                    else:
                        key = _admissible_key(mode, cs + cn - c[b1] - c[b2], max(c[b1], c[b2]), max(cs, cn), (0, t, b2, k2))
                        after = {b1: (short, cs), b2: (new, cn)}
                    if key is not None and (best is None or key < best[0]):
                        best = (key, after)
        for ta in sorted(where):
            for tb in sorted(where):
                if not ta < tb:
                    continue
                swap = {ta: tb, tb: ta}
                touched = sorted({where[ta][0], where[tb][0]})
                after = {b: [swap.get(t, t) for t in tours[b]] for b in touched}
                after = {b: (tour, tour_cost(qs, qt, b, tour)) for b, tour in after.items()}
                if any(cn is None for _, cn in after.values()):
                    continue
                key = _admissible_key(mode, sum(cn for _, cn in after.values()) - sum(c[b] for b in touched),
                                      max(c[b] for b in touched), max(cn for _, cn in after.values()), (1, ta, tb, 0))
                if key is not None and (best is None or key < best[0]):
                    best = (key, after)
        if best is None:
            break
        for b, (tour, cn) in best[1].items():
            tours[b], c[b] = list(tour), cn
        rounds += 1
    return report(tours, c, B, T, K, build_steps, rounds)


# ---------------------------------------------------------------------------------------------------------------------
# the vectorised restatement

def _gaps(tours):
    """every position of every tour in the order (b, k): robot, k, predecessor (-1: the start), successor (-1: none)"""
    gb, gk, gp, gs = [], [], [], []
    for b, tour in enumerate(tours):
        n = len(tour)
        gb += [b] * (n + 1)
        gk += range(n + 1)
        gp += [-1] + tour
        gs += tour + [-1]
    return [np.asarray(x, dtype=np.int64) for x in (gb, gk, gp, gs)]


def _least(lead, ok, index):
    """the entry with the least (lead, index) among ok: (lead, index) or None"""
    if not ok.any():
        return None
    m = np.where(ok, lead, BIG).min()
    return int(m), int(index[ok & (lead == m)].min())


def tours_ref(qs, qt, K, mode, max_rounds, improve_from=None):
    """as tours_loop, vectorised over the candidates of a step"""
    qs, qt = np.asarray(qs, dtype=np.int64), np.asarray(qt, dtype=np.int64)
    B, T = qs.shape
    E = np.vstack([qs, qt])                                  # row b: from the start of b; row B + t: from task t
    tours = [[] for _ in range(B)] if improve_from is None else [list(map(int, t)) for t in improve_from]
    c = np.asarray([tour_cost(qs, qt, b, tours[b]) for b in range(B)], dtype=np.int64)
    owner = np.full(T, -1, dtype=np.int64)
    for b, tour in enumerate(tours):
        owner[tour] = b
    build_steps = 0
    while improve_from is None:
        U = np.flatnonzero(owner < 0)
        gb, gk, gp, gs = _gaps(tours)
        room = np.asarray([len(t) for t in tours])[gb] < K
        gb, gk, gp, gs = gb[room], gk[room], gp[room], gs[room]
        if not len(U) or not len(gb):
            break
        row, has = np.where(gp < 0, gb, B + gp), gs >= 0
        old = np.where(has, E[row, np.maximum(gs, 0)], 0)
        first = E[row[:, None], U[None, :]]
        second = qt[U[None, :], np.maximum(gs, 0)[:, None]]
        ok = (first >= 0) & (~has[:, None] | (second >= 0))
        delta = first + np.where(has[:, None], second, 0) - old[:, None]
        lead = delta if mode == 0 else c[gb][:, None] + delta
        index = (gb[:, None] << B_SHIFT) | (U[None, :] << T_SHIFT) | gk[:, None]
        best = _least(lead, ok, index)
        if best is None:
            break
        b, t, k = best[1] >> B_SHIFT, (best[1] >> T_SHIFT) & 1023, best[1] & 2047
        c[b] = best[0] if mode == 1 else c[b] + best[0]
        tours[b].insert(k, t)
        owner[t] = b
        build_steps += 1
    rounds = 0
    while rounds < max_rounds:
        A = np.flatnonzero(owner >= 0)
        if not len(A):
            break
        gb, gk, gp, gs = _gaps(tours)
        lens = np.asarray([len(t) for t in tours])
        pos = np.zeros(T, dtype=np.int64)
        pred, succ = np.full(T, -1, dtype=np.int64), np.full(T, -1, dtype=np.int64)
        for tour in tours:
            pos[tour] = np.arange(len(tour))
            pred[tour[1:]] = tour[:-1]
            succ[tour[:-1]] = tour[1:]
        ba, pa, na = owner[A], pred[A], succ[A]
        ra = np.where(pa < 0, ba, B + pa)
        e_in = E[ra, A]                                      # the edge into a, and the one out of it (0 without successor)
        e_out = np.where(na >= 0, qt[A, np.maximum(na, 0)], 0)
        # relocate: rows are the gaps, columns the assigned tasks
        bridge = np.where(na >= 0, E[ra, np.maximum(na, 0)], 0)
        rem = e_in + e_out - bridge
        row, has = np.where(gp < 0, gb, B + gp), gs >= 0
        old = np.where(has, E[row, np.maximum(gs, 0)], 0)
        first = E[row[:, None], A[None, :]]
        second = qt[A[None, :], np.maximum(gs, 0)[:, None]]
        own = gb[:, None] == ba[None, :]
        at_t = own & ((gk[:, None] == pos[A][None, :]) | (gk[:, None] == pos[A][None, :] + 1))
        ok = (first >= 0) & (~has[:, None] | (second >= 0)) & (bridge >= 0)[None, :] & ~at_t & (own | (lens[gb] < K)[:, None])
        ins = first + np.where(has[:, None], second, 0) - old[:, None]
        ds = ins - rem[None, :]
        c1, c2 = c[ba][None, :], c[gb][:, None]
        pm_old = np.where(own, c1, np.maximum(c1, c2))
        pm_new = np.where(own, c1 + ds, np.maximum(c1 - rem[None, :], c2 + ins))
        k2 = np.where(own & (gk[:, None] > pos[A][None, :]), gk[:, None] - 1, gk[:, None])
        index = (A[None, :] << B_SHIFT) | (gb[:, None] << T_SHIFT) | k2
        moves = [(ds, pm_old, pm_new, ok, index)]
        # exchange: rows a, columns b, a < b
        n = len(A)
        a_, b_ = A[:, None], A[None, :]
        e1 = E[ra[:, None], b_]                              # e(pred of a, b)
        e2 = qt[b_, np.maximum(na, 0)[:, None]]              # e(b, succ of a)
        e3 = E[ra[None, :], a_]                              # e(pred of b, a)
        e4 = qt[a_, np.maximum(na, 0)[None, :]]              # e(a, succ of b)
        ha, hb = (na >= 0)[:, None], (na >= 0)[None, :]
        da = e1 + np.where(ha, e2, 0) - (e_in + e_out)[:, None]
        db = e3 + np.where(hb, e4, 0) - (e_in + e_out)[None, :]
        ok = (e1 >= 0) & (~ha | (e2 >= 0)) & (e3 >= 0) & (~hb | (e4 >= 0))
        same = ba[:, None] == ba[None, :]
        ca, cb = c[ba][:, None], c[ba][None, :]
        ds = da + db
        pm_old = np.where(same, ca, np.maximum(ca, cb))
        pm_new = np.where(same, ca + ds, np.maximum(ca + da, cb + db))
        ab = na[:, None] == b_                               # a directly in front of b: pred a, b, a, succ b
        mid = qt[b_, a_]
        ds_ab = e1 + mid + np.where(hb, e4, 0) - (e_in[:, None] + e_in[None, :] + e_out[None, :])
        ok_ab = (e1 >= 0) & (mid >= 0) & (~hb | (e4 >= 0))
        ba_adj = na[None, :] == a_                           # b directly in front of a: pred b, a, b, succ a
        mid2 = qt[a_, b_]
        ds_ba = e3 + mid2 + np.where(ha, e2, 0) - (e_in[None, :] + e_in[:, None] + e_out[:, None])
        ok_ba = (e3 >= 0) & (mid2 >= 0) & (~ha | (e2 >= 0))
        ds = np.where(ab, ds_ab, np.where(ba_adj, ds_ba, ds))
        ok = np.where(ab, ok_ab, np.where(ba_adj, ok_ba, ok)) & np.triu(np.ones((n, n), dtype=bool), 1)
        pm_new = np.where(ab | ba_adj, ca + ds, pm_new)
        index = (np.int64(1) << KIND_SHIFT) | (a_ << B_SHIFT) | (b_ << T_SHIFT)
        moves.append((ds, pm_old, pm_new, ok, index + 0 * ds))
        best = None
        for ds, pm_old, pm_new, ok, index in moves:
            if mode == 0:
                lead, adm = ds, ds < 0
            else:
                pmd = pm_new - pm_old
                lead, adm = pmd * (1 << 25) + (ds + (1 << 24)), (pmd < 0) | ((pmd == 0) & (ds < 0))
            got = _least(lead, ok & adm, index)
            if got is not None and (best is None or got < best):
                best = got
        if best is None:
            break
        kind, i, j, l = best[1] >> KIND_SHIFT, (best[1] >> B_SHIFT) & 1023, (best[1] >> T_SHIFT) & 1023, best[1] & 2047
        if kind == 0:
            b1 = int(owner[i])
            tours[b1].remove(i)
            tours[j].insert(l, i)
            owner[i] = j
            touched = {b1, j}
        else:
            b1, b2 = int(owner[i]), int(owner[j])
            p1, p2 = tours[b1].index(i), tours[b2].index(j)
            tours[b1][p1], tours[b2][p2] = j, i
            owner[i], owner[j] = b2, b1
            touched = {b1, b2}
        for b in touched:                                    # (the deltas above are what chose the move; the properties
            c[b] = tour_cost(qs, qt, b, tours[b])            #  test holds the two against each other through tours_loop)
        rounds += 1
    return report(tours, c, B, T, K, build_steps, rounds)


def tours_problem_ref(start_cost, task_cost, K, mode=1, scale=1024.0, max_rounds=1 << 30, fn=tours_ref):
    """fp64 costs -> report(), as rmpc_tours_device gives it for one problem"""
    return fn(quantise(start_cost, scale), quantise(task_cost, scale), K, mode, max_rounds)


def objective(out, mode):
    return out["span"] if mode == 1 else out["total"]


def brute_force(qs, qt, K, mode):
    """the least objective over all ways to hand every task to a robot (at most K each) in some order; None when no
    way serves every task"""
    import itertools
    B, T = len(qs), len(qs[0])
    best = None
    costs = {}

    def cost(b, tour):
        if (b, tour) not in costs:
            costs[(b, tour)] = tour_cost(qs, qt, b, tour)
        return costs[(b, tour)]

    for owners in itertools.product(range(B), repeat=T):
        sets = [tuple(t for t in range(T) if owners[t] == b) for b in range(B)]
        if max(len(s) for s in sets) > K:
            continue
        cs = []
        for b, s in enumerate(sets):
            least = min((x for x in (cost(b, p) for p in itertools.permutations(s)) if x is not None), default=None)
            cs.append(least)
        if any(x is None for x in cs):
            continue
        value = max(cs) if mode == 1 else sum(cs)
        best = value if best is None or value < best else best
    return best


# ---------------------------------------------------------------------------------------------------------------------
# the follower of rmpc_follow_tour_device

def follow_tour_ref(paths, lens, idx, pos, W, x0, y0, cell, threshold, stop_at, leg, served, now, stop_tol):
    """one call, vectorised over the robots: idx, leg and served are updated in place, pos is (B, >= 2); returns goal
    (B, 3) with NaN rows for the robots that keep theirs (len <= 0)"""
    B, K = stop_at.shape
    goal = np.full((B, 3), np.nan)
    act = np.flatnonzero(lens > 0)
    if not len(act):
        return goal
    L = lens[act].astype(np.int64)
    i = np.clip(idx[act].astype(np.int64), 0, L - 1)
    lg = np.maximum(leg[act].astype(np.int64), 0)
    cells = paths[act, i].astype(np.int64)
    dx = (x0 + (cells % W).astype(np.float64) * cell) - pos[act, 0]
    dy = (y0 + (cells // W).astype(np.float64) * cell) - pos[act, 1]
    dist = np.sqrt(dx * dx + dy * dy)
    at_stop = (lg < K) & (stop_at[act, np.minimum(lg, K - 1)] == i)
    serve = at_stop & (dist <= stop_tol)
    served[act[serve], lg[serve]] = now
    lg = lg + serve
    again = (lg < K) & (stop_at[act, np.minimum(lg, K - 1)] == i)
    step = (i < L - 1) & np.where(at_stop, serve & ~again, dist <= threshold)
    i = i + step
    idx[act], leg[act] = i, lg
    cells = paths[act, i].astype(np.int64)
    goal[act, 0] = x0 + (cells % W).astype(np.float64) * cell
    goal[act, 1] = y0 + (cells // W).astype(np.float64) * cell
    goal[act, 2] = 0.0
    return goal


def follow_tour_loop(paths, lens, idx, pos, W, x0, y0, cell, threshold, stop_at, leg, served, now, stop_tol):
    """the same call robot by robot, from the header's sentences"""
    import math
    B, K = stop_at.shape
    goal = np.full((B, 3), np.nan)
    for b in range(B):
        L = int(lens[b])
        if L <= 0:
            continue
        i = min(max(int(idx[b]), 0), L - 1)
        lg = max(int(leg[b]), 0)
        cx, cy = x0 + float(paths[b, i] % W) * cell, y0 + float(paths[b, i] // W) * cell
        dist = math.sqrt((cx - pos[b, 0]) * (cx - pos[b, 0]) + (cy - pos[b, 1]) * (cy - pos[b, 1]))
        if lg < K and stop_at[b, lg] == i:
            if dist <= stop_tol:
                served[b, lg] = now
                lg += 1
                if i < L - 1 and not (lg < K and stop_at[b, lg] == i):
                    i += 1
        elif i < L - 1 and dist <= threshold:
            i += 1
        idx[b], leg[b] = i, lg
        goal[b] = (x0 + float(paths[b, i] % W) * cell, y0 + float(paths[b, i] // W) * cell, 0.0)
    return goal


def join_legs(legs, leg_lens, tour_len, max_len):
    """K legs (each (B, leg_max) cells with lens (B,)) -> (paths (B, max_len), lens (B,), stop_at (B, K)): the legs of a
    robot joined without the doubled junction cell; leg k counts for robots with tour_len > k.  A leg that is no path
    (len <= 0) ends the robot's route there."""
    K, B = len(legs), len(tour_len)
    paths = np.zeros((B, max_len), dtype=np.int32)
    lens = np.zeros(B, dtype=np.int32)
    stop_at = np.full((B, K), -1, dtype=np.int32)
    for b in range(B):
        route = []
        for k in range(min(K, int(tour_len[b]))):
            n = int(leg_lens[k][b])
            if n <= 0:
                break
            cells = legs[k][b, :n].tolist()
            route += cells if not route else cells[1:]
            stop_at[b, k] = len(route) - 1
        assert len(route) <= max_len
        paths[b, :len(route)] = route
        lens[b] = len(route)
    return paths, lens, stop_at


def plan_ref(data, starts, goals, K, mode=1, scale=1024.0, max_rounds=1 << 30, max_len=None):
    """TourPlanner.plan restated from the planner's restatements: the goals' fields, the route costs from the starts and
    between the goals, the tours, one descent per leg, the legs joined.  Returns dict(fields, start_cost, task_cost,
    out (report()), paths, lens, stop_at)."""
    from assignment_reference import route_costs_ref
    from global_planner_reference import descend_ref, field_ref
    H, W = data.shape
    B, T = len(starts), len(goals)
    fields = np.stack([field_ref(data, int(g)) for g in goals])
    start_cost = route_costs_ref(data, fields, starts)
    task_cost = route_costs_ref(data, fields, goals)
    out = tours_problem_ref(start_cost, task_cost, K, mode, scale, max_rounds)
    max_len = max_len if max_len is not None else min(H * W, 4 * (H + W))
    legs = [np.zeros((B, max_len), dtype=np.int32) for _ in range(K)]
    leg_lens = [np.zeros(B, dtype=np.int32) for _ in range(K)]
    for b in range(B):
        at = int(starts[b])
        for k in range(int(out["len"][b])):
            t = int(out["tours"][b, k])
            route = descend_ref(data, fields[t], at, int(goals[t]))
            legs[k][b, :len(route)] = route
            leg_lens[k][b] = len(route)
            at = int(goals[t])
    paths, lens, stop_at = join_legs(legs, leg_lens, out["len"], K * max_len)
    return dict(fields=fields, start_cost=start_cost, task_cost=task_cost, out=out, paths=paths, lens=lens, stop_at=stop_at)
