"""Conflict-free timed routes for a fleet, in the plain frame of ``batch.py``: ``TimedRoutes`` plans B
robots in space-time on the grid for several priority orders at once (``rmpc_timed_plan_device``: cooperative A* as a
layered reachability sweep, one workgroup per order), ``TimedFollower`` hands every robot its next waypoint once per
control step and lets it pass only when the robots planned ahead of it have cleared the cells around it
(``rmpc_timed_follow_device``).  ``priority_orders`` makes the orders on the host, once."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .batch import MOVES, _dev_tensor, pick_routes


def priority_orders(B, G, seed=0):
    """(G, B) int32: the identity, then G - 1 seeded permutations of 0 .. B - 1 (``numpy.random.default_rng(seed)``)"""
    rng = np.random.default_rng(seed)
    return np.stack([np.arange(B)] + [rng.permutation(B) for _ in range(G - 1)]).astype(np.int32)


def pick_spaced_routes(raw, ok, B, rng, x0, y0, cell, sep2):
    """B (start, goal) cell pairs drawn one at a time by ``pick_routes`` and kept when the start is at least ``sep2``
    (squared cells) from every kept start and the goal from every kept goal: the premise of the plan's guarantee at
    layer 0, and goals that can all be held at once."""
    W = raw.shape[1]
    d2 = lambda a, b: (a // W - b // W) ** 2 + (a % W - b % W) ** 2
    starts, goals = [], []
    while len(starts) < B:
        s, g = pick_routes(raw, ok, 1, rng, x0, y0, cell)
        s, g = int(s[0]), int(g[0])
        if all(d2(s, q) >= sep2 for q in starts) and all(d2(g, q) >= sep2 for q in goals):
            starts.append(s); goals.append(g)
    return np.array(starts, np.int32), np.array(goals, np.int32)


class TimedRoutes:
    """Space-time routes on ``grid`` (H, W) (numpy or device tensor) over the window t = 0 .. T: two robots of one
    order that both have status 0 are never closer than ``sep2`` (squared cells) within ``lag`` layers of each other.
    ``orders``: a (G, B) array of permutations, or their number G (``priority_orders`` at the first ``plan``).
    ``plan(start_cells, goal_cells)`` launches the fields of the distinct goals and the plan and reads nothing back.
    ``repair`` = R > 0: every order is repaired on the device for up to R rounds (``rmpc_timed_plan_repair_device``,
    DESIGN.md 27): the robots that failed or came late are planned first in the next round; ``self.order_out`` (G, B) is
    then the order each row's plan belongs to, ``self.rounds_run`` and ``self.round_best`` (G,) what the search did."""

    def __init__(self, grid, movement, occupancy_threshold, T, sep2, lag=1, orders=4, occupancy_cost_factor=3.0, seed=0,
                 device=None, repair=0):
        import torch
        if movement not in MOVES:
            raise ValueError("Unknown movement")
        dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
        self.grid = _dev_tensor(grid, torch.float64, dev)
        self.device, self.movement, self.threshold = dev, MOVES[movement], float(occupancy_threshold)
        self.cost_factor, self.T, self.sep2, self.lag, self.seed = float(occupancy_cost_factor), int(T), int(sep2), int(lag), seed
        self.orders = orders if isinstance(orders, int) else _dev_tensor(np.asarray(orders), torch.int32, dev)
        self.repair = int(repair)
        if not 0 <= self.repair <= _lib.TIMED_MAX_ROUNDS:
            raise ValueError("repair must lie in [0, TIMED_MAX_ROUNDS]")
        self.work = None

    def plan(self, start_cells, goal_cells, stream=None):
        """start_cells, goal_cells (B,) cell indices -> (paths (G, B, T + 1), status (G, B), arrive (G, B), best (1,))
        int32 on the device, as ``rmpc_timed_plan_device`` writes them; ``self.key`` (G,) int64 its keys."""
        import torch
        dev, g = self.device, self.grid
        H, W = int(g.shape[0]), int(g.shape[1])
        s = _dev_tensor(start_cells, torch.int32, dev).reshape(-1)
        gc = _dev_tensor(goal_cells, torch.int32, dev).reshape(-1)
        B = int(s.shape[0])
        if B != gc.shape[0] or B < 1:
            raise ValueError("start_cells and goal_cells must both be (B,), B >= 1")
        if isinstance(self.orders, int):
            self.orders = _dev_tensor(priority_orders(B, self.orders, self.seed), torch.int32, dev)
        G = int(self.orders.shape[0])
        uniq, inv = torch.unique(gc, return_inverse=True)     # (the count of distinct goals sizes the fields)
        uniq, inv = uniq.to(torch.int32).contiguous(), inv.to(torch.int32).contiguous()
        Gf = int(uniq.shape[0])
        fields = torch.empty((Gf, H, W), dtype=torch.float64, device=dev)
        fstatus = torch.empty(Gf, dtype=torch.int32, device=dev)
        if self.repair:                                       # (the repair's workspace grows with B)
            nbytes = _lib.timed_plan_repair_work_bytes(H, W, self.T, G, B)
            if self.work is None or self.work.numel() < nbytes:
                self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        elif self.work is None:
            self.work = torch.empty(_lib.timed_plan_work_bytes(H, W, self.T, G), dtype=torch.uint8, device=dev)
        paths = torch.empty((G, B, self.T + 1), dtype=torch.int32, device=dev)
        status = torch.empty((G, B), dtype=torch.int32, device=dev)
        arrive = torch.empty((G, B), dtype=torch.int32, device=dev)
        self.key = torch.empty(G, dtype=torch.int64, device=dev)
        best = torch.empty(1, dtype=torch.int32, device=dev)
        st = _lib.stream_handle(stream, dev)
        _lib.grid_fields_device(g, uniq, fields, fstatus, self.movement, self.threshold, self.cost_factor, stream=st)
        if self.repair:
            self.order_out = torch.empty((G, B), dtype=torch.int32, device=dev)
            self.rounds_run = torch.empty(G, dtype=torch.int32, device=dev)
            self.round_best = torch.empty(G, dtype=torch.int32, device=dev)
            args = _lib.timed_repair_args(g, s, inv, fields, uniq, self.orders, self.work, paths, status, arrive, self.key,
                                          best, self.order_out, self.rounds_run, self.round_best, self.repair,
                                          movement=self.movement, occ_threshold=self.threshold, sep2=self.sep2, lag=self.lag)
            _lib.timed_plan_repair_device(args, stream=st)
        else:
            args = _lib.timed_plan_args(g, s, inv, fields, uniq, self.orders, self.work, paths, status, arrive, self.key,
                                        best, movement=self.movement, occ_threshold=self.threshold, sep2=self.sep2,
                                        lag=self.lag)
            _lib.timed_plan_device(args, stream=st)
        self.fields, self.field_status = fields, fstatus
        return paths, status, arrive, best


class TimedFollower:
    """One order's timed routes ``paths`` (B, T + 1) on the device; ``step(xinit, goal)`` is one
    ``rmpc_timed_follow_device`` launch between two index buffers that change roles: a robot at its waypoint moves on
    when every robot planned through the cells around its next one has left them, and every robot with a route gets
    its waypoint's centre written into ``goal`` (B, 3).  ``blocked`` (B,) names the robot each one waits for, or -1."""

    def __init__(self, paths, W, x0, y0, cell, threshold, sep2, lag=1):
        import torch
        self.paths = paths.contiguous()
        B = int(paths.shape[0])
        self.idx = torch.zeros(B, dtype=torch.int32, device=paths.device)
        self._next = torch.zeros(B, dtype=torch.int32, device=paths.device)
        self.blocked = torch.full((B,), -1, dtype=torch.int32, device=paths.device)
        self.W, self.x0, self.y0, self.cell, self.threshold = int(W), float(x0), float(y0), float(cell), float(threshold)
        self.sep2, self.lag = int(sep2), int(lag)

    def step(self, xinit, goal, stream=None):
        _lib.timed_follow_device(self.paths, self.idx, self._next, xinit, goal, self.W, self.x0, self.y0, self.cell,
                                 self.threshold, self.sep2, self.lag, blocked=self.blocked,
                                 stream=_lib.stream_handle(stream, goal.device))
        self.idx, self._next = self._next, self.idx
