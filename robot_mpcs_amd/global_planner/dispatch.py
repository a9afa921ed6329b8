"""Who goes where: ``GoalAssigner`` pairs a fleet's robots with a set of goal cells at the least sum of route costs and
plans the routes, on the device.  The cost-to-go fields of the T goals are built once; ``assign`` reads the B x T route
costs off them (``rmpc_grid_route_costs_device``) and solves the minimum-cost assignment
(``rmpc_assign_optimal_device``, include/rmpc_assign_opt.h); ``plan`` also descends every robot's field
(``rmpc_grid_paths_device``).  Tensor operations and launches on one stream, no host read."""
from __future__ import annotations

from .. import _lib
from .batch import MOVES, _dev_tensor


class GoalAssigner:
    """grid (H, W) occupancy (numpy or device tensor), goal_cells (T,) cell indices row * W + col.  Owns ``fields``
    (T, H, W), ``status`` (T,), ``cost`` (B, T) fp64, ``assignment`` (B,) int32 (what ``assign`` returns), ``total`` (1,)
    int64 -- the sum of rint(cost * scale) over the pairs --, ``count`` (1,) and ``steps`` (1,) int32, the workspace,
    ``paths`` and ``lens``; the tensors that depend on B are made at the first call and again when B changes."""

    def __init__(self, grid, goal_cells, movement="8N", occupancy_threshold=0.8, occupancy_cost_factor=3.0, scale=1024.0,
                 max_len=None, device=None):
        import torch
        if movement not in MOVES:
            raise ValueError("Unknown movement")
        dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
        self.grid = _dev_tensor(grid, torch.float64, dev)
        self.H, self.W = int(self.grid.shape[0]), int(self.grid.shape[1])
        self.goal_cells = _dev_tensor(goal_cells, torch.int32, dev).reshape(-1)
        self.T = int(self.goal_cells.shape[0])
        if not 1 <= self.T <= _lib.ASSIGN_MAX_TARGETS:
            raise ValueError(f"GoalAssigner: need 1 <= T <= {_lib.ASSIGN_MAX_TARGETS} goal cells")
        self.movement, self.occ, self.factor = MOVES[movement], float(occupancy_threshold), float(occupancy_cost_factor)
        self.scale = float(scale)
        self.max_len = int(max_len) if max_len is not None else min(self.H * self.W, 4 * (self.H + self.W))
        self.fields = torch.empty((self.T, self.H, self.W), dtype=torch.float64, device=dev)
        self.status = torch.empty(self.T, dtype=torch.int32, device=dev)
        self.total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=dev)
        self.steps = torch.zeros(1, dtype=torch.int32, device=dev)
        self.B = 0
        # a map beyond one workgroup's LDS takes the tiled entry, as in plan_batch
        fields_device = _lib.grid_fields_large_device if self.H * self.W > _lib.GRID_MAX_CELLS else _lib.grid_fields_device
        fields_device(self.grid, self.goal_cells, self.fields, self.status, self.movement, self.occ, self.factor,
                      stream=_lib.stream_handle(None, dev))

    def _sized(self, B):
        import torch
        if B != self.B:
            dev = self.grid.device
            self.B = B
            self.cost = torch.empty((B, self.T), dtype=torch.float64, device=dev)
            self.assignment = torch.empty(B, dtype=torch.int32, device=dev)
            self.work = torch.empty(_lib.assign_optimal_work_bytes(1, B, self.T), dtype=torch.uint8, device=dev)
            self.paths = torch.empty((B, self.max_len), dtype=torch.int32, device=dev)
            self.lens = torch.empty(B, dtype=torch.int32, device=dev)

    def _starts(self, start_cells):
        import torch
        s = _dev_tensor(start_cells, torch.int32, self.grid.device).reshape(-1)
        if not 1 <= int(s.shape[0]) <= _lib.ASSIGN_MAX_ROBOTS:
            raise ValueError(f"GoalAssigner: need 1 <= B <= {_lib.ASSIGN_MAX_ROBOTS} start cells")
        self._sized(int(s.shape[0]))
        return s

    def assign(self, start_cells, stream=None):
        """start_cells (B,) -> assign (B,) int32 on the device (``self.assignment``): the index into goal_cells of every
        robot's goal, -1 for a robot without one (more robots than goals, or no route to a goal that is left).  Enqueues
        on ``stream`` (a ``torch.cuda.Stream``; None = the current one) and never synchronises."""
        import torch
        with torch.cuda.stream(stream):     # (None: the current one stays)
            return self._assign(self._starts(start_cells))

    def _assign(self, s):
        import torch
        st = torch.cuda.current_stream(self.grid.device).cuda_stream
        _lib.grid_route_costs_device(self.grid, self.fields, s, self.cost, self.movement, self.occ, self.factor, stream=st)
        _lib.assign_optimal_device(self.cost, self.assignment, self.scale, self.total, self.count, self.steps, self.work,
                                   stream=st)
        return self.assignment

    def plan(self, start_cells, stream=None):
        """``assign``, then every robot's route down its goal's field: (paths (B, max_len) int32, lens (B,) int32) in
        ``plan_batch``'s format, lens = 0 for a robot left without a goal -- what ``RouteFollower`` and
        ``RouteFollower.replace`` take."""
        import torch
        with torch.cuda.stream(stream):
            s = self._starts(start_cells)
            a = self._assign(s)
            _lib.grid_paths_device(self.grid, self.fields, self.goal_cells, s, a, self.paths, self.lens, self.movement,
                                   self.occ, self.factor, stream=torch.cuda.current_stream(self.grid.device).cuda_stream)
            self.lens.masked_fill_(a < 0, 0)
            return self.paths, self.lens

    def goal_cells_of(self, assign=None):
        """(B,) int32: the goal cell of every robot under ``assign`` (the last one when None), -1 where it has none --
        the goal_cells of ``TimedRoutes.plan``"""
        import torch
        a = self.assignment if assign is None else assign
        cells = self.goal_cells[a.clamp(min=0).long()]
        return torch.where(a >= 0, cells, torch.full_like(cells, -1))
