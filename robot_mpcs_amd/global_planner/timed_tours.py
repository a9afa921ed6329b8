"""Timed tours: ``TimedTours`` lets a ``TourPlanner`` decide which robot serves which picks in which
order and then plans the fleet in space-time through every robot's stops, for several priority orders at once
(``rmpc_timed_tours_plan_device``, include/rmpc_timed_tours.h): routes that are conflict-free by construction and stand
``dwell`` layers on every pick.  ``TimedTourFollower`` keeps the plan's order and serves a pick only when the robot is
on it (``rmpc_timed_tours_follow_device``).  Launches on one stream, no host read."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .batch import _dev_tensor, pick_routes
from .timed import priority_orders


def pick_spaced_tours(raw, ok, B, picks, rng, x0, y0, cell, sep2, start_sep2=None):
    """B start cells and ``picks`` pick cells drawn as ``pick_spaced_routes`` draws: one ``pick_routes`` pair at a time,
    its start kept while fewer than B are and it is at least ``start_sep2`` (squared cells; ``sep2`` when None) from
    every kept start, its goal kept as a pick while fewer than ``picks`` are and it is at least ``sep2`` from every kept
    pick -- starts that can all be held at once (the premise of the plan's guarantee at layer 0), and picks that can.
    A body that reaches ahead of its base needs the wider ``start_sep2``: the cells speak of base centres."""
    W = raw.shape[1]
    d2 = lambda a, b: (a // W - b // W) ** 2 + (a % W - b % W) ** 2
    start_sep2 = sep2 if start_sep2 is None else start_sep2
    starts, goals = [], []
    while len(starts) < B or len(goals) < picks:
        s, g = pick_routes(raw, ok, 1, rng, x0, y0, cell)
        s, g = int(s[0]), int(g[0])
        if len(starts) < B and all(d2(s, q) >= start_sep2 for q in starts):
            starts.append(s)
        if len(goals) < picks and all(d2(g, q) >= sep2 for q in goals):
            goals.append(g)
    return np.array(starts, np.int32), np.array(goals, np.int32)


class TimedTours:
    """``tour_planner``: a ``TourPlanner``, whose grid, movement, goal cells and goal fields are used as they are.  T the
    window, ``sep2`` (squared cells) and ``lag`` as in ``TimedRoutes``, ``dwell`` the layers a robot stands on a pick after
    it reaches it, ``orders`` a (G, B) array of permutations or their number.  ``park``: where a robot goes after its last
    pick -- "last": it stays by it (an open tour; a robot without a tour parks by its own start), "start": back to its
    start, or (B,) cells, a depot per robot.  The fields of the B extra cells are computed behind the picks' fields: by
    ``plan`` for the starts, once for given cells."""

    def __init__(self, tour_planner, T, sep2, lag=1, dwell=0, orders=4, park="last", seed=0):
        import torch
        tp = self.tp = tour_planner
        dev = self.device = tp.grid.device
        self.T, self.sep2, self.lag, self.dwell, self.seed = int(T), int(sep2), int(lag), int(dwell), seed
        if not 1 <= tp.K <= _lib.TIMED_TOURS_MAX_STOPS or not 0 <= self.dwell <= _lib.TIMED_TOURS_MAX_DWELL:
            raise ValueError(f"TimedTours: need K <= {_lib.TIMED_TOURS_MAX_STOPS} and 0 <= dwell <= {_lib.TIMED_TOURS_MAX_DWELL}")
        self.orders = orders if isinstance(orders, int) else _dev_tensor(np.asarray(orders), torch.int32, dev)
        self.park = park if isinstance(park, str) else _dev_tensor(np.asarray(park), torch.int32, dev).reshape(-1)
        if isinstance(park, str) and park not in ("last", "start"):
            raise ValueError("TimedTours: park must be 'last', 'start' or (B,) cells")
        self.B = 0

    def _sized(self, B):
        import torch
        tp, dev = self.tp, self.device
        if B == self.B:
            return
        self.B = B
        G = self.orders if isinstance(self.orders, int) else int(self.orders.shape[0])
        if isinstance(self.orders, int):
            self.orders = _dev_tensor(priority_orders(B, G, self.seed), torch.int32, dev)
        i32 = torch.int32
        self.fields = torch.empty((tp.T + B, tp.H, tp.W), dtype=torch.float64, device=dev)
        self.fields[:tp.T].copy_(tp.fields)
        self.field_status = torch.empty(B, dtype=i32, device=dev)
        self.goal_cells = torch.empty(tp.T + B, dtype=i32, device=dev)
        self.goal_cells[:tp.T].copy_(tp.goal_cells)
        self.own = torch.arange(tp.T, tp.T + B, dtype=i32, device=dev)        # the index of every robot's extra field
        self.park_index = self.own.clone()
        self.work = torch.empty(_lib.timed_tours_work_bytes(tp.H, tp.W, self.T, G), dtype=torch.uint8, device=dev)
        self.paths = torch.empty((G, B, self.T + 1), dtype=i32, device=dev)
        self.status, self.arrive, self.served = (torch.empty((G, B), dtype=i32, device=dev) for _ in range(3))
        self.serve_at = torch.empty((G, B, tp.K), dtype=i32, device=dev)
        self.key = torch.empty(G, dtype=torch.int64, device=dev)
        self.unserved = torch.empty(G, dtype=i32, device=dev)
        self.best = torch.empty(1, dtype=i32, device=dev)
        if not isinstance(self.park, str):
            if int(self.park.shape[0]) != B:
                raise ValueError("TimedTours: park needs one cell per robot")
            self._extra_fields(self.park, _lib.stream_handle(None, dev))

    def _extra_fields(self, cells, st):
        tp = self.tp
        self.goal_cells[tp.T:].copy_(cells)
        _lib.grid_fields_device(tp.grid, self.goal_cells[tp.T:], self.fields[tp.T:], self.field_status, tp.movement, tp.occ,
                                tp.factor, stream=st)

    def plan(self, start_cells, stream=None):
        """start_cells (B,) -> (paths (G, B, T + 1), serve_at (G, B, K), status, served, arrive (G, B), best (1,)) int32
        on the device, as ``rmpc_timed_tours_plan_device`` writes them; ``self.key`` (G,) int64 and ``self.unserved`` (G,)
        rank the orders.  The tours are ``tour_planner.tours`` / ``tour_len``.  Enqueues on ``stream`` (a
        ``torch.cuda.Stream``; None = the current one) and never synchronises."""
        import torch
        tp = self.tp
        with torch.cuda.stream(stream):
            s = _dev_tensor(start_cells, torch.int32, self.device).reshape(-1).contiguous()
            self._sized(int(s.shape[0]))
            tours, lens = tp.assign(s)
            st = torch.cuda.current_stream(self.device).cuda_stream
            if isinstance(self.park, str):
                self._extra_fields(s, st)
                if self.park == "last":
                    last = tours.gather(1, (lens.long() - 1).clamp(min=0)[:, None])[:, 0]
                    self.park_index = torch.where(lens > 0, last, self.own).contiguous()
            args = _lib.timed_tours_args(tp.grid, s, tours, lens, self.park_index, self.fields, self.goal_cells, self.orders,
                                         self.work, self.paths, self.status, self.arrive, self.key, self.best, self.serve_at,
                                         self.served, self.unserved, dwell=self.dwell, movement=tp.movement,
                                         occ_threshold=tp.occ, sep2=self.sep2, lag=self.lag)
            _lib.timed_tours_plan_device(args, stream=st)
        return self.paths, self.serve_at, self.status, self.served, self.arrive, self.best


class TimedTourFollower:
    """One order's timed tour ``paths`` (B, T + 1) and ``serve_at`` (B, K) on the device; ``step(pos, goal)`` is one
    ``rmpc_timed_tours_follow_device`` launch between two index buffers that change roles, as ``TimedFollower.step``: a
    robot on the layer of its next stop stays until it is within ``stop_tol`` of the cell, then ``served`` (B, K) takes
    the step's number.  ``pos`` is any (B, >= 2) fp64 device tensor whose rows are ``pos.stride(0)`` apart.  ``leg`` (B,)
    counts the stops served, ``now`` the calls made, ``blocked`` (B,) names the robot each one waits for, or -1."""

    def __init__(self, paths, serve_at, W, x0, y0, cell, threshold, stop_tol, sep2, lag=1):
        import torch
        self.paths, self.serve_at = paths.contiguous(), serve_at.contiguous()
        B, K = int(serve_at.shape[0]), int(serve_at.shape[1])
        dev = paths.device
        self.idx = torch.zeros(B, dtype=torch.int32, device=dev)
        self._next = torch.zeros(B, dtype=torch.int32, device=dev)
        self.leg = torch.zeros(B, dtype=torch.int32, device=dev)
        self.served = torch.full((B, K), -1, dtype=torch.int32, device=dev)
        self.blocked = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.W, self.x0, self.y0, self.cell = int(W), float(x0), float(y0), float(cell)
        self.threshold, self.stop_tol, self.sep2, self.lag, self.now = float(threshold), float(stop_tol), int(sep2), int(lag), 0

    def step(self, pos, goal, stream=None):
        if pos.stride(1) != 1:
            pos = pos.contiguous()
        _lib.timed_tours_follow_device(self.paths, self.idx, self._next, pos, goal, self.W, self.x0, self.y0, self.cell,
                                       self.threshold, self.sep2, self.lag, self.serve_at, self.leg, self.served, self.now,
                                       self.stop_tol, blocked=self.blocked, stream=_lib.stream_handle(stream, goal.device))
        self.idx, self._next = self._next, self.idx
        self.now += 1

    def replace(self, paths, serve_at, idx, leg):
        """swaps in new ``paths`` (B, T + 1), ``serve_at`` (B, K), indices and legs (B,) int32 -- a re-plan in the old
        plan's layer frame (``lifelong.rebase``); ``served`` starts again at -1 for the new stops.  The tensors are
        copied where they are not contiguous int32 already; idx and leg are always copied."""
        import torch
        self.paths, self.serve_at = paths.contiguous(), serve_at.contiguous()
        self.idx, self.leg = idx.to(torch.int32).clone(), leg.to(torch.int32).clone()
        self._next = torch.zeros_like(self.idx)
        self.served = torch.full_like(self.serve_at, -1)

    def served_count(self):
        """() int64 on the device: the stops served so far"""
        return (self.served >= 0).sum()
