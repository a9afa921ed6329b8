"""More picks than robots: ``TourPlanner`` hands every robot a tour of up to K of a set of goal cells and plans the
route through them, ``TourFollower`` drives along it and stops at every pick, on the device.  The cost-to-go fields of
the T goals and the T x T costs between them are built once; ``plan`` reads the B x T route costs off the fields
(``rmpc_grid_route_costs_device``), decides the tours (``rmpc_tours_device``, include/rmpc_tours.h), descends one field
per leg (``rmpc_grid_paths_device``) and joins the legs.  Tensor operations and launches on one stream, no host read."""
from __future__ import annotations

from .. import _lib
from .batch import MOVES, _dev_tensor


def join_legs(legs, leg_lens, paths):
    """legs (K, B, max_len) int32 and leg_lens (K, B) int32 as K calls of ``rmpc_grid_paths_device`` gave them, leg k
    starting on the last cell of leg k - 1 -> the robots' routes written into paths (B, >= K max_len), and (lens (B,)
    int32, stop_at (B, K) int32): a leg that is no path (leg_lens <= 0) ends the route, every leg but the first drops its
    first cell, the junction, and stop_at [b][k] is the index of the last cell of leg k, -1 when the route ended before
    it.  Tensor operations only."""
    import torch
    K, B, max_len = legs.shape
    ok = torch.cumprod((leg_lens > 0).long(), 0)
    n = leg_lens.long().clamp(min=0) * ok
    n[1:] -= ok[1:]
    end = torch.cumsum(n, 0)
    cols = torch.arange(max_len, device=legs.device)
    R = paths.shape[1]
    for k in range(K):
        # in ascending order whatever a leg writes past its end is overwritten by the next one or lies past lens
        skip = 1 if k else 0
        dest = ((end[k] - n[k])[:, None] + cols[None, :max_len - skip]).clamp(max=R - 1)
        paths.scatter_(1, dest, legs[k][:, skip:])
    stop_at = torch.where(ok.bool(), end - 1, torch.full_like(end, -1)).t().to(torch.int32).contiguous()
    return end[-1].to(torch.int32), stop_at


class TourPlanner:
    """grid (H, W) occupancy (numpy or device tensor), goal_cells (T,) cell indices row * W + col, K the most goals per
    robot, mode "span" (the longest tour as short as the rule gets it) or "sum".  Owns ``fields`` (T, H, W), ``status``
    (T,), ``task_cost`` (T, T) fp64 -- goal i to goal j --, and after ``plan`` ``start_cost`` (B, T), ``tours`` (B, K)
    int32 (indices into goal_cells, -1 padded), ``tour_len`` (B,), ``tour_cost`` (B,) int64 (the quantised costs),
    ``owner`` (T,), ``count``, ``build_steps``, ``rounds`` (1,) int32, ``total``, ``span`` (1,) int64, ``paths``
    (B, K max_len), ``lens`` (B,), ``stop_at`` (B, K); the tensors that depend on B are made at the first call and again
    when B changes."""

    def __init__(self, grid, goal_cells, K, mode="span", scale=1024.0, max_rounds=1 << 30, movement="8N",
                 occupancy_threshold=0.8, occupancy_cost_factor=3.0, max_len=None, device=None):
        import torch
        if movement not in MOVES:
            raise ValueError("Unknown movement")
        if mode not in ("span", "sum"):
            raise ValueError("TourPlanner: mode must be 'span' or 'sum'")
        dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
        self.grid = _dev_tensor(grid, torch.float64, dev)
        self.H, self.W = int(self.grid.shape[0]), int(self.grid.shape[1])
        self.goal_cells = _dev_tensor(goal_cells, torch.int32, dev).reshape(-1)
        self.T, self.K = int(self.goal_cells.shape[0]), int(K)
        if not 1 <= self.T <= _lib.TOURS_MAX_TASKS or not 1 <= self.K <= self.T:
            raise ValueError(f"TourPlanner: need 1 <= T <= {_lib.TOURS_MAX_TASKS} goal cells and 1 <= K <= T")
        self.movement, self.occ, self.factor = MOVES[movement], float(occupancy_threshold), float(occupancy_cost_factor)
        self.mode, self.scale, self.max_rounds = mode, float(scale), int(max_rounds)
        self.max_len = int(max_len) if max_len is not None else min(self.H * self.W, 4 * (self.H + self.W))
        self.fields = torch.empty((self.T, self.H, self.W), dtype=torch.float64, device=dev)
        self.status = torch.empty(self.T, dtype=torch.int32, device=dev)
        self.task_cost = torch.empty((self.T, self.T), dtype=torch.float64, device=dev)
        self.count, self.build_steps, self.rounds = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(3))
        self.total, self.span = (torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(2))
        self.owner = torch.empty(self.T, dtype=torch.int32, device=dev)
        self.B = 0
        st = _lib.stream_handle(None, dev)
        # a map beyond one workgroup's LDS takes the tiled entry, as in GoalAssigner
        fields_device = _lib.grid_fields_large_device if self.H * self.W > _lib.GRID_MAX_CELLS else _lib.grid_fields_device
        fields_device(self.grid, self.goal_cells, self.fields, self.status, self.movement, self.occ, self.factor, stream=st)
        # goal i to goal j: field j at the cell of goal i
        _lib.grid_route_costs_device(self.grid, self.fields, self.goal_cells, self.task_cost, self.movement, self.occ,
                                     self.factor, stream=st)

    def _sized(self, B):
        import torch
        if B != self.B:
            dev = self.grid.device
            self.B = B
            self.start_cost = torch.empty((B, self.T), dtype=torch.float64, device=dev)
            self.tours = torch.empty((B, self.K), dtype=torch.int32, device=dev)
            self.tour_len = torch.empty(B, dtype=torch.int32, device=dev)
            self.tour_cost = torch.empty(B, dtype=torch.int64, device=dev)
            self.work = torch.empty(_lib.tours_work_bytes(1, B, self.T), dtype=torch.uint8, device=dev)
            self.legs = torch.zeros((self.K, B, self.max_len), dtype=torch.int32, device=dev)
            self.leg_lens = torch.zeros((self.K, B), dtype=torch.int32, device=dev)
            self.paths = torch.zeros((B, self.K * self.max_len), dtype=torch.int32, device=dev)

    def _starts(self, start_cells):
        import torch
        s = _dev_tensor(start_cells, torch.int32, self.grid.device).reshape(-1)
        if not 1 <= int(s.shape[0]) <= _lib.TOURS_MAX_ROBOTS:
            raise ValueError(f"TourPlanner: need 1 <= B <= {_lib.TOURS_MAX_ROBOTS} start cells")
        self._sized(int(s.shape[0]))
        return s

    def assign(self, start_cells, available=None, stream=None):
        """start_cells (B,) -> (tours (B, K) int32, tour_len (B,) int32) on the device: every robot's goals in the order
        it visits them, as indices into goal_cells.  ``available`` (B,): a robot whose entry is 0 gets start costs of
        +inf, which the tours' rule never takes, and so no goal; None = every robot.  Enqueues on ``stream`` (a
        ``torch.cuda.Stream``; None = the current one) and never synchronises."""
        import torch
        with torch.cuda.stream(stream):     # (None: the current one stays)
            self._assign(self._starts(start_cells), available)
            return self.tours, self.tour_len

    def _assign(self, s, available=None):
        import torch
        st = torch.cuda.current_stream(self.grid.device).cuda_stream
        _lib.grid_route_costs_device(self.grid, self.fields, s, self.start_cost, self.movement, self.occ, self.factor, stream=st)
        if available is not None:
            out = _dev_tensor(available, torch.int32, self.grid.device).reshape(-1) == 0
            self.start_cost.masked_fill_(out[:, None], float("inf"))
        _lib.tours_device(self.start_cost, self.task_cost, self.tours, self.tour_len, self.tour_cost, self.mode, self.scale,
                          self.max_rounds, self.owner, self.count, self.total, self.span, self.build_steps, self.rounds,
                          self.work, stream=st)

    def plan(self, start_cells, stream=None, available=None):
        """``assign`` (``available`` as there), then the route of every robot through its goals: (paths (B, K max_len) int32, lens (B,) int32,
        stop_at (B, K) int32).  Leg k runs from the cell before it (the start, then goal k - 1) down the field of goal k;
        the legs are joined without the doubled junction cell, and stop_at [b][k] is the index of goal k in the robot's
        path, -1 past its tour -- what ``TourFollower`` takes.  lens = 0 for a robot without a goal."""
        import torch
        with torch.cuda.stream(stream):
            s = self._starts(start_cells)
            self._assign(s, available)
            st = torch.cuda.current_stream(self.grid.device).cuda_stream
            at = s
            for k in range(self.K):
                index = self.tours[:, k].contiguous()       # -1 past the tour's end: the descent reports no path
                _lib.grid_paths_device(self.grid, self.fields, self.goal_cells, at, index, self.legs[k], self.leg_lens[k],
                                       self.movement, self.occ, self.factor, stream=st)
                at = self.goal_cells[index.clamp(min=0).long()].contiguous()
            self.lens, self.stop_at = join_legs(self.legs, self.leg_lens, self.paths)
            return self.paths, self.lens, self.stop_at

    def goal_cells_of(self, tours=None):
        """(B, K) int32: the goal cells of every robot's tour (the last one's when None), -1 past its end"""
        import torch
        t = self.tours if tours is None else tours
        cells = self.goal_cells[t.clamp(min=0).long()]
        return torch.where(t >= 0, cells, torch.full_like(cells, -1))


class TourFollower:
    """Routes with stops of B robots on the device; ``step(pos, goal)`` is one ``rmpc_follow_tour_device`` launch: as
    ``RouteFollower.step``, but a robot whose waypoint is its next stop stays on it until it is within ``stop_tol`` of
    it; then ``served`` (B, K) takes the step's number and the robot moves on.  ``pos`` is any (B, >= 2) fp64 device
    tensor whose rows are ``pos.stride(0)`` apart -- xinit, or the end links' positions.  ``leg`` (B,) counts the stops
    served, ``now`` the calls made."""

    def __init__(self, paths, lens, stop_at, W, x0, y0, cell, threshold=1.3, stop_tol=0.25):
        import torch
        self.paths, self.lens, self.stop_at = paths, lens, stop_at
        B, K = int(stop_at.shape[0]), int(stop_at.shape[1])
        self.idx = torch.zeros(B, dtype=torch.int32, device=paths.device)
        self.leg = torch.zeros(B, dtype=torch.int32, device=paths.device)
        self.served = torch.full((B, K), -1, dtype=torch.int32, device=paths.device)
        self.W, self.x0, self.y0, self.cell = int(W), float(x0), float(y0), float(cell)
        self.threshold, self.stop_tol, self.now = float(threshold), float(stop_tol), 0

    def step(self, pos, goal, stream=None):
        if pos.stride(1) != 1:
            pos = pos.contiguous()
        _lib.follow_tour_device(self.paths, self.lens, self.idx, pos, goal, self.W, self.x0, self.y0, self.cell,
                                self.threshold, self.stop_at, self.leg, self.served, self.now, self.stop_tol,
                                stream=_lib.stream_handle(stream, goal.device))
        self.now += 1

    def served_count(self):
        """() int64 on the device: the stops served so far"""
        return (self.served >= 0).sum()
