"""Frontier exploration for a fleet that maps as it drives, on the device: ``FrontierGoals`` turns the
evidence of a ``FleetMap`` into routes to the nearest frontier -- a known free cell next to unknown space -- for every
robot, so that a fleet without a map and without goals explores until no frontier is left.  One re-plan is the chain

    FleetMap.occupancy (unknown = free value) -> grid_inflate_device -> grid_frontier_device
    -> grid_fields_seeded_device (G = 1) -> cells_from_positions -> grid_descend_device -> RouteFollower.replace

on one stream without a host read.  There is no CPU path.

With ``tile`` > 0 the robots are coordinated: the frontier is cut into one target per tile, every
robot-target pair is priced by its route cost and the pairs are shared out greedily, so that robots which start together
part instead of following each other to the same nearest frontier cell:

    ... -> grid_frontier_device -> grid_targets_device -> grid_fields_seeded_device (G = T, seeds = tseeds)
    -> cells_from_positions -> grid_route_costs_device -> assign_greedy_device
    -> grid_descend_device (field_index = assign, seeds = tseeds) -> RouteFollower.replace
"""
from __future__ import annotations

import numpy as np

from .. import _lib
from ..global_planner import FREE, OCC
from ..store import clear_cells


def corner_starts(raw, B, clear=2):
    """The B cells nearest the corner (row 0, col 0) of the map ``raw`` (H, W; > 0.5 occupied) that stay free when the
    map is dilated by ``clear`` cells (Chebyshev): a fleet unloaded in one corner.  (B,) int32 cell indices row * W + col,
    ordered by distance, then by index."""
    W = raw.shape[1]
    cells = np.flatnonzero(clear_cells(raw, clear).ravel())
    if len(cells) < B:
        raise ValueError(f"corner_starts: the map has {len(cells)} clear cells, {B} asked for")
    d2 = (cells // W) ** 2 + (cells % W) ** 2
    return cells[np.lexsort((cells, d2))][:B].astype(np.int32)


class FrontierGoals:
    """Routes to the nearest frontier of ``fmap`` (a ``FleetMap``) for its B robots.

    Owns ``enlarged``, ``plan``, ``seed`` (H, W) fp64, ``count`` (1,) int32, one ``field`` (1, H, W) fp64 with its
    ``status`` and ``sweeps`` (1,) int32, ``cells`` (B,) int32, ``paths`` (B, max_len) int32 and ``lens`` (B,) int32.
    ``size_robot`` and ``threshold`` are those of ``grid_inflate_device`` on the classified map, whose unknown cells get
    the free value; the planning grid ``plan`` then holds ``unknown_value`` (>= ``occ_threshold``: routes stay inside
    what has been seen) on the cells without evidence, which are not dilated.  ``frontier_moves`` (4 or 8): which
    neighbours count as next to unknown space.  The first ``replan`` must come after the first ``FleetMap.mark``: a map
    without evidence has no frontier.

    ``tile`` > 0: routes to distinct targets instead, T = ``grid_tiles(H, W, tile)`` of them.  The object then also owns
    ``targets`` (T,) int32, ``tseeds`` and ``fields`` (T, H, W) fp64 with ``status`` and ``sweeps`` (T,) int32 (in place
    of the single ``field``'s), ``cost`` (B, T) fp64, ``assign`` and ``passes`` (B,) int32.  A robot that no target
    takes (``assign`` -1) keeps the route it has."""

    def __init__(self, fmap, size_robot, threshold=0.29, free_value=FREE, occ_value=OCC, unknown_value=1.0,
                 occ_threshold=0.8, cost_factor=3.0, movement=8, frontier_moves=4, max_len=None, tile=0):
        import torch
        if not float(unknown_value) >= float(occ_threshold):
            raise ValueError("FrontierGoals: unknown_value must be >= occ_threshold (unknown cells are not planned through)")
        self.tile = int(tile)
        if self.tile < 0:
            raise ValueError("FrontierGoals: tile must be >= 0 (0: every robot goes to the nearest frontier cell)")
        if self.tile:
            self.T = _lib.grid_tiles(fmap.H, fmap.W, self.tile)
            if self.T > _lib.ASSIGN_MAX_TARGETS:
                raise ValueError(f"FrontierGoals: tile = {self.tile} cuts the {fmap.H} x {fmap.W} map into {self.T} "
                                 f"targets, more than RMPC_ASSIGN_MAX_TARGETS = {_lib.ASSIGN_MAX_TARGETS}")
            if fmap.B > _lib.ASSIGN_MAX_ROBOTS:
                raise ValueError(f"FrontierGoals: {fmap.B} robots exceed RMPC_ASSIGN_MAX_ROBOTS = {_lib.ASSIGN_MAX_ROBOTS}")
        self.fmap = fmap
        self.size_robot, self.threshold = float(size_robot), float(threshold)
        self.free_value, self.occ_value, self.unknown_value = float(free_value), float(occ_value), float(unknown_value)
        self.occ_threshold, self.cost_factor = float(occ_threshold), float(cost_factor)
        self.movement, self.frontier_moves = int(movement), int(frontier_moves)
        H, W, B, dev = fmap.H, fmap.W, fmap.B, fmap.device
        self.max_len = int(max_len) if max_len is not None else min(H * W, 4 * (H + W))
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        self.enlarged = torch.zeros((H, W), **f64)
        self.plan = torch.zeros((H, W), **f64)
        self.seed = torch.full((H, W), float("inf"), **f64)
        self.count = torch.zeros(1, **i32)
        self.field = torch.full((1, H, W), float("inf"), **f64)
        self.status = torch.zeros(1, **i32)
        self.sweeps = torch.zeros(1, **i32)
        self.cells = torch.zeros(B, **i32)
        self.field_index = torch.zeros(B, **i32)
        self.paths = torch.zeros((B, self.max_len), **i32)
        self.lens = torch.zeros(B, **i32)
        if self.tile:
            T = self.T
            self.targets = torch.full((T,), -1, **i32)
            self.tseeds = torch.full((T, H, W), float("inf"), **f64)
            self.fields = torch.full((T, H, W), float("inf"), **f64)
            self.status = torch.zeros(T, **i32)
            self.sweeps = torch.zeros(T, **i32)
            self.cost = torch.full((B, T), float("inf"), **f64)
            self.assign = torch.full((B,), -1, **i32)
            self.passes = torch.full((B,), -1, **i32)
        self._stream = None

    def replan(self, follower, xinit, stream=None):
        """xinit (B, stride >= 2) the robots' states; ``follower`` a ``RouteFollower``.  Enqueues the whole chain on
        ``stream`` (a ``torch.cuda.Stream``; None = the current one) and never synchronises.  A robot with
        ``lens`` <= 0 (no frontier reachable, outside the map, route too long) keeps the route it has; one that stands
        on a frontier cell gets the route of that one cell.  Returns (paths, lens) of the new plan."""
        import torch
        fm = self.fmap
        with torch.cuda.stream(stream):     # (None: the current one stays)
            self._stream = torch.cuda.current_stream(fm.device)
            st = self._stream.cuda_stream
            grid = fm.occupancy(self.free_value, self.occ_value, self.free_value, stream=st)
            _lib.grid_inflate_device(grid, self.enlarged, fm.cell, self.size_robot, self.threshold, stream=st)
            self.count.zero_()
            _lib.grid_frontier_device(fm.hits, fm.misses, self.enlarged, self.plan, self.seed, self.count,
                                      self.occ_threshold, self.frontier_moves, self.unknown_value, stream=st)
            if self.tile:
                self._coordinated(xinit, st)
            else:
                _lib.grid_fields_seeded_device(self.plan, self.seed[None], self.field, self.status, self.movement,
                                               self.occ_threshold, self.cost_factor, sweeps=self.sweeps, stream=st)
                _lib.grid_cells_device(xinit, self.cells, fm.H, fm.W, fm.x0, fm.y0, fm.cell, stream=st)
                _lib.grid_descend_device(self.plan, self.field, self.seed[None], self.cells, self.field_index,
                                         self.paths, self.lens, self.movement, self.occ_threshold, self.cost_factor,
                                         stream=st)
            follower.replace(self.paths, self.lens)
        return self.paths, self.lens

    def _coordinated(self, xinit, st):
        """frontier -> one target per tile -> a field per target -> route costs -> assignment -> each robot's descent of
        its target's field (``assign`` -1: RMPC_GRID_OUTSIDE, the robot keeps its route)"""
        fm = self.fmap
        _lib.grid_targets_device(self.seed, self.tile, self.targets, self.tseeds, stream=st)
        _lib.grid_fields_seeded_device(self.plan, self.tseeds, self.fields, self.status, self.movement,
                                       self.occ_threshold, self.cost_factor, sweeps=self.sweeps, stream=st)
        _lib.grid_cells_device(xinit, self.cells, fm.H, fm.W, fm.x0, fm.y0, fm.cell, stream=st)
        _lib.grid_route_costs_device(self.plan, self.fields, self.cells, self.cost, self.movement, self.occ_threshold,
                                     self.cost_factor, stream=st)
        _lib.assign_greedy_device(self.cost, self.assign, self.passes, stream=st)
        _lib.grid_descend_device(self.plan, self.fields, self.tseeds, self.cells, self.assign, self.paths, self.lens,
                                 self.movement, self.occ_threshold, self.cost_factor, stream=st)

    def frontier_cells(self):
        """The number of frontier cells the last ``replan`` found: the one host read (it waits for the device)."""
        if self._stream is not None:
            self._stream.synchronize()
        return int(self.count.item())
