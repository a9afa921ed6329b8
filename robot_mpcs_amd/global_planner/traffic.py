"""Traffic-aware routes for a fleet, planned on the device (include/rmpc_traffic.h): guide routes that
know about each other.  A flow table counts, per cell, the routes that visit it and the steps that leave it by each of
the eight moves; a route pays ``w_visit`` for every other route on a cell it enters (congestion) and ``w_contra`` for
every route that steps the other way over the same edge (contraflow), so lanes form on their own.  ``TrafficRoutes``
plans every robot on the empty table, then re-plans the fleet group by group against the flow of the others for a
number of rounds -- with groups of one this is a best-response iteration whose potential ``L + w_visit V + w_contra C``
never rises.  The routes are the ``paths`` / ``lens`` layout of ``plan_batch``: ``RouteFollower``, ``VisibleFollower``,
``shorten_routes`` and ``route_lengths`` read them as they are.  There is no CPU path."""
from __future__ import annotations

import contextlib

import numpy as np

from .. import _lib
from .batch import MOVES, _dev_tensor, cells_from_positions


class TrafficRoutes:
    """``TrafficRoutes(grid, starts, goal_cells, movement="8N", costs=None, groups=None, rounds=2)``: grid (H, W) occupancy
    (numpy or device tensor, at most ``_lib.GRID_MAX_CELLS`` cells), starts and goal_cells (B,) cell indices,
    ``costs`` a ``_lib.traffic_costs()`` (None: its defaults, the untuned weights of DESIGN.md 30), ``groups`` J: the robots
    with b % J == j are re-planned together, blind to each other within the step (None: min(8, B)); ``rounds`` R.
    The two ends: J = B re-plans one robot at a time, the best-response iteration whose potential never rises; J = 1
    removes the whole fleet's routes before it re-plans them, so every round repeats the blind plan.

    ``plan()``: 1. every robot on the empty table, all routes added; 2. R times, for each group j: the group's routes are
    removed from the table, fields for the group's distinct goals are made on the others' flow, the new routes descended
    and added; 3. a score row (L, V, C) after the initial plan and after every round.  Everything is queued on one
    stream, nothing is read on the host; the per-group goal lists are made once, here.  Afterwards ``paths`` (B, max_len)
    int32, ``lens`` (B,) int32 (as ``rmpc_grid_paths_device`` reports them), ``flow`` (9, H, W) int32 and ``scores``
    (R + 1, 3) int64 hold the result, on the device."""

    def __init__(self, grid, starts, goal_cells, movement="8N", costs=None, groups=None, rounds=2, occupancy_threshold=0.8,
                 max_len=None, device=None):
        import torch
        if movement not in MOVES:
            raise ValueError("Unknown movement")
        dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
        self.device, self.movement, self.occ = dev, MOVES[movement], float(occupancy_threshold)
        self.grid = _dev_tensor(grid, torch.float64, dev)
        H, W = int(self.grid.shape[0]), int(self.grid.shape[1])
        if H * W > _lib.GRID_MAX_CELLS:
            raise ValueError("TrafficRoutes: maps above GRID_MAX_CELLS = %d cells are not supported" % _lib.GRID_MAX_CELLS)
        goals = np.asarray(goal_cells.cpu() if torch.is_tensor(goal_cells) else goal_cells).astype(np.int32).reshape(-1)
        self.starts = _dev_tensor(starts, torch.int32, dev).reshape(-1).clone()
        B, R = int(goals.shape[0]), int(rounds)
        J = min(8, B) if groups is None else int(groups)
        if B < 1 or int(self.starts.shape[0]) != B:
            raise ValueError("TrafficRoutes: starts and goal_cells must both be (B,), B >= 1")
        if not 1 <= J <= B or R < 0:
            raise ValueError("TrafficRoutes: need 1 <= groups <= B and rounds >= 0")
        self.H, self.W, self.B, self.groups, self.rounds = H, W, B, J, R
        self.costs = costs if costs is not None else _lib.traffic_costs()
        self.max_len = int(max_len) if max_len is not None else min(H * W, 4 * (H + W))
        i32 = dict(dtype=torch.int32, device=dev)
        # the goal lists: of the whole fleet for the initial plan, of every group for the rounds
        uniq, inv = np.unique(goals, return_inverse=True)
        self._all = (torch.from_numpy(uniq).to(dev), torch.from_numpy(inv.astype(np.int32)).to(dev))
        self._groups = []
        for j in range(J):
            idx = np.arange(j, B, J)
            u, gi = np.unique(goals[idx], return_inverse=True)
            select = np.zeros(B, np.int32)
            select[idx] = 1
            self._groups.append(dict(idx=torch.from_numpy(idx).to(dev), select=torch.from_numpy(select).to(dev),
                                     goals=torch.from_numpy(u).to(dev), index=torch.from_numpy(gi.astype(np.int32)).to(dev),
                                     starts=torch.empty(len(idx), **i32), paths=torch.empty((len(idx), self.max_len), **i32),
                                     lens=torch.empty(len(idx), **i32)))
        G = max([len(uniq)] + [int(g["goals"].shape[0]) for g in self._groups])
        self.fields = torch.empty((G, H, W), **i32)
        self.status = torch.empty(G, **i32)
        self.flow = torch.zeros((_lib.TRAFFIC_PLANES, H, W), **i32)
        self.paths = torch.zeros((B, self.max_len), **i32)
        self.lens = torch.zeros(B, **i32)
        self.scores = torch.zeros((R + 1, 3), dtype=torch.int64, device=dev)

    def _route(self, goals, index, starts, paths, lens, st):
        G = int(goals.shape[0])
        _lib.grid_fields_traffic_device(self.grid, self.flow, self.costs, goals, self.fields[:G], self.status[:G], self.movement,
                                        self.occ, stream=st)
        _lib.grid_paths_traffic_device(self.grid, self.flow, self.costs, self.fields[:G], goals, starts, index, paths, lens,
                                       self.movement, self.occ, stream=st)

    def _score(self, row, st):
        _lib.grid_traffic_score_device(self.flow, self.scores[row], self.costs.base_axial, self.costs.base_diag, stream=st)

    def plan(self, stream=None):
        """Runs the initial plan and the rounds; returns (paths, lens).  ``stream``: a raw handle, or None for the stream
        torch's operations run on on this device -- the tensor operations between the launches are queued there too.
        ``paths`` and ``lens`` are this object's buffers, written again by the next ``plan()``: a follower that is to
        outlive it gets copies."""
        import torch
        on = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device)) if stream is not None \
            else contextlib.nullcontext()
        with torch.cuda.device(self.device), on:
            st = _lib.stream_handle(stream, self.device)
            self.flow.zero_()
            self._route(*self._all, self.starts, self.paths, self.lens, st)
            _lib.grid_traffic_add_device(self.flow, self.paths, self.lens, 1, stream=st)
            self._score(0, st)
            for r in range(self.rounds):
                for g in self._groups:
                    _lib.grid_traffic_add_device(self.flow, self.paths, self.lens, -1, select=g["select"], stream=st)
                    torch.index_select(self.starts, 0, g["idx"], out=g["starts"])
                    self._route(g["goals"], g["index"], g["starts"], g["paths"], g["lens"], st)
                    # (rows of g["paths"] past their length hold what an earlier step left: no reader looks there)
                    self.paths.index_copy_(0, g["idx"], g["paths"])
                    self.lens.index_copy_(0, g["idx"], g["lens"])
                    _lib.grid_traffic_add_device(self.flow, self.paths, self.lens, 1, select=g["select"], stream=st)
                self._score(r + 1, st)
        return self.paths, self.lens

    def replan(self, follower, xinit, stream=None):
        """Re-bases the starts on the robots' present cells (``rmpc_grid_cells_device`` of xinit (B, stride >= 2) in the
        follower's frame), runs ``plan()`` and swaps the result in through ``follower.replace``, as ``batch.replan``
        does: a robot without a new route (outside the map, on an occupied cell) keeps the one it has.  Returns
        (paths, lens)."""
        import torch
        on = torch.cuda.stream(torch.cuda.ExternalStream(stream, device=self.device)) if stream is not None \
            else contextlib.nullcontext()
        with on:
            cells = cells_from_positions(xinit, self.H, self.W, follower.x0, follower.y0, follower.cell, stream=stream)
            self.starts.copy_(cells)
        paths, lens = self.plan(stream=stream)
        with on:
            follower.replace(paths, lens)
        return paths, lens
