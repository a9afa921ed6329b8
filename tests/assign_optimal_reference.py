"""The rule of include/rmpc_assign_opt.h restated in numpy and Python integers, written from the header: quantisation,
orientation, the shortest-augmenting-path loop with its order of rows and ties, the report and the step count."""
import math

import numpy as np

MAX_Q = 1 << 20
BIG = 1 << 62


def quantise(cost, scale=1024.0):
    """q (B, T) int64: rint(cost * scale) of a takeable pair, -1 of any other"""
    cost = np.asarray(cost, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(cost * np.float64(scale))
        take = (cost >= 0.0) & (cost < math.inf) & (r <= MAX_Q)
    return np.where(take, r, -1.0).astype(np.int64)


def oriented(q):
    """(C (m, n) int64 with P on the pairs nobody may take, P, by_robot): the rows are the robots when B <= T"""
    B, T = q.shape
    by_robot = B <= T
    Q = q if by_robot else q.T
    qmax = int(Q.max()) if (Q >= 0).any() else 0
    P = Q.shape[0] * qmax + 1
    return np.where(Q >= 0, Q, P).astype(np.int64), P, by_robot


def sap(C):
    """The loop on an integer matrix C (m <= n): (row of every column p [1..n] with p [0] unused, steps).  Vectorised
    over the columns; np.argmin takes the first of equal values, which is the lowest column."""
    C = np.asarray(C, dtype=np.int64)
    m, n = C.shape
    assert 1 <= m <= n
    u = np.zeros(m + 1, dtype=np.int64)
    v = np.zeros(n + 1, dtype=np.int64)
    p = np.zeros(n + 1, dtype=np.int64)
    way = np.zeros(n + 1, dtype=np.int64)
    steps = 0
    for i in range(1, m + 1):
        p[0] = i
        j0 = 0
        minv = np.full(n + 1, BIG, dtype=np.int64)
        used = np.zeros(n + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = C[i0 - 1] - u[i0] - v[1:]
            better = ~used[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            j1 = int(np.argmin(np.where(used[1:], BIG + 1, minv[1:]))) + 1
            delta = minv[j1]
            u[p[used]] += delta                      # the rows of the used columns are distinct
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            steps += 1
            if p[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return p, steps


def sap_python(C):
    """The same loop on Python integers, element by element, with the extremes the header bounds: returns
    (p, steps, dict(u_max, v_min, minv_max, key_max)); u_min, v_max and minv_min are asserted on the way."""
    m, n = len(C), len(C[0])
    assert 1 <= m <= n
    u, v, p, way = [0] * (m + 1), [0] * (n + 1), [0] * (n + 1), [0] * (n + 1)
    ext = dict(u_max=0, v_min=0, minv_max=0, key_max=0)
    steps = 0
    for i in range(1, m + 1):
        p[0], j0 = i, 0
        minv, used = [BIG] * (n + 1), [False] * (n + 1)
        while True:
            used[j0] = True
            i0 = p[j0]
            best = None
            for j in range(1, n + 1):
                if used[j]:
                    continue
                cur = int(C[i0 - 1][j - 1]) - u[i0] - v[j]
                assert cur >= 0
                if cur < minv[j]:
                    minv[j], way[j] = cur, j0
                ext["minv_max"] = max(ext["minv_max"], minv[j])
                key = (minv[j] << 13) | j
                ext["key_max"] = max(ext["key_max"], key)
                if best is None or key < best:
                    best = key
            j1, delta = best & 8191, best >> 13
            assert delta == minv[j1] and delta >= 0
            for j in range(n + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            ext["u_max"], ext["v_min"] = max(ext["u_max"], max(u)), min(ext["v_min"], min(v[1:]))
            assert min(u) >= 0 and max(v[1:]) <= 0 and min(minv[1:]) >= 0
            j0 = j1
            steps += 1
            if p[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return p, steps, ext


def assign_optimal_ref(cost, scale=1024.0):
    """cost (B, T) -> (assign (B,) int32, total, count, steps) as rmpc_assign_optimal_device reports them"""
    q = quantise(cost, scale)
    B, T = q.shape
    C, P, by_robot = oriented(q)
    p, steps = sap(C)
    assign = np.full(B, -1, dtype=np.int32)
    total = count = 0
    for j in range(1, C.shape[1] + 1):
        i = int(p[j])
        if i == 0:
            continue
        b, t = (i - 1, j - 1) if by_robot else (j - 1, i - 1)
        if q[b, t] >= 0:
            assign[b] = t
            total += int(q[b, t])
            count += 1
    return assign, total, count, steps


def check_matching(q, assign):
    """assign is a matching on takeable pairs: (count, sum of q)"""
    taken = assign[assign >= 0]
    assert len(set(taken.tolist())) == len(taken) and (assign >= -1).all() and (assign < q.shape[1]).all()
    rows = np.flatnonzero(assign >= 0)
    assert (q[rows, assign[rows]] >= 0).all()
    return len(rows), int(q[rows, assign[rows]].sum())
