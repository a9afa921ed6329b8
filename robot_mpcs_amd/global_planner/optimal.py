"""Optimal timed routes for a fleet (include/rmpc_cbs.h): ``OptimalTimedRoutes`` runs conflict-based
search over the cells, layers and conflicts of ``TimedRoutes`` on the device (``rmpc_cbs_device``).  For a handful of
robots it proves the least sum of arrivals; beyond that its ``bound`` is a lower bound that any prioritised plan can be
held against, and a conflict-free node it reports is a plan ``TimedFollower`` takes as it stands.

``BoundedTimedRoutes`` (include/rmpc_ecbs.h) is the focal search beside it (``rmpc_ecbs_device``): a
conflict-free plan for the whole fleet whose sum of arrivals is proven to lie within the factor ``w`` of the least one."""
from __future__ import annotations

from .. import _lib
from .batch import MOVES, _dev_tensor


class OptimalTimedRoutes:
    """Space-time routes on ``grid`` (H, W) (numpy or device tensor) over the window t = 0 .. T with the least sum of
    arrivals among all sets of routes in which no two robots come closer than ``sep2`` (squared cells) within ``lag``
    layers.  ``nodes``: the pool of search nodes, ``expand``: nodes taken per round, ``rounds``: rounds per call.
    ``plan(start_cells, goal_cells)`` launches the fields of the distinct goals and the search and reads nothing back;
    ``more(rounds)`` continues it; ``info`` (CBS_INFO,) int32 on the device holds outcome, node, conflict_free, cost,
    bound, created, expanded, rounds_run at ``_lib.CBS_OUTCOME`` and so on."""
    _work_bytes = staticmethod(_lib.cbs_work_bytes)      # (the focal search below brings its own)
    _info_len = _lib.CBS_INFO

    def __init__(self, grid, movement, occupancy_threshold, T, sep2, lag=1, nodes=4096, expand=16, rounds=64,
                 occupancy_cost_factor=3.0, device=None):
        import torch
        if movement not in MOVES:
            raise ValueError("Unknown movement")
        dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
        self.grid = _dev_tensor(grid, torch.float64, dev)
        self.device, self.movement, self.threshold = dev, MOVES[movement], float(occupancy_threshold)
        self.cost_factor, self.T, self.sep2, self.lag = float(occupancy_cost_factor), int(T), int(sep2), int(lag)
        self.nodes, self.expand, self.rounds = int(nodes), int(expand), int(rounds)
        self.work = None

    def _call(self, rounds, resume, stream):
        a = self._inputs
        args = _lib.cbs_args(self.grid, *a, self.work, self.paths, self.status, self.arrive, self.info, self.nodes,
                             self.expand, rounds, resume=resume, movement=self.movement, occ_threshold=self.threshold,
                             sep2=self.sep2, lag=self.lag)
        _lib.cbs_device(args, stream=_lib.stream_handle(stream, self.device))
        return self.paths, self.status, self.arrive, self.info

    def plan(self, start_cells, goal_cells, stream=None):
        """start_cells, goal_cells (B,) cell indices -> (paths (B, T + 1), status (B,), arrive (B,), info (CBS_INFO,)) int32
        on the device, as ``rmpc_cbs_device`` writes them after ``rounds`` rounds from the root"""
        import torch
        dev, g = self.device, self.grid
        H, W = int(g.shape[0]), int(g.shape[1])
        s = _dev_tensor(start_cells, torch.int32, dev).reshape(-1)
        gc = _dev_tensor(goal_cells, torch.int32, dev).reshape(-1)
        B = int(s.shape[0])
        if B != gc.shape[0] or B < 1:
            raise ValueError("start_cells and goal_cells must both be (B,), B >= 1")
        uniq, inv = torch.unique(gc, return_inverse=True)     # (the count of distinct goals sizes the fields)
        uniq, inv = uniq.to(torch.int32).contiguous(), inv.to(torch.int32).contiguous()
        Gf = int(uniq.shape[0])
        self.fields = torch.empty((Gf, H, W), dtype=torch.float64, device=dev)
        self.field_status = torch.empty(Gf, dtype=torch.int32, device=dev)
        nbytes = self._work_bytes(H, W, self.T, B, self.nodes, self.expand)
        if self.work is None or self.work.numel() != nbytes:
            self.work = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.paths = torch.empty((B, self.T + 1), dtype=torch.int32, device=dev)
        self.status = torch.empty(B, dtype=torch.int32, device=dev)
        self.arrive = torch.empty(B, dtype=torch.int32, device=dev)
        self.info = torch.empty(self._info_len, dtype=torch.int32, device=dev)
        self._inputs = (s, inv, self.fields, uniq)
        _lib.grid_fields_device(g, uniq, self.fields, self.field_status, self.movement, self.threshold, self.cost_factor,
                                stream=_lib.stream_handle(stream, dev))
        return self._call(self.rounds, False, stream)

    def more(self, rounds=None, stream=None):
        """``rounds`` more rounds (the class's by default) of the search that ``plan`` began, into the same outputs"""
        if self.work is None:
            raise ValueError("more() continues a search: call plan() first")
        return self._call(self.rounds if rounds is None else int(rounds), True, stream)

    def gap(self, timed_arrive):
        """(2,) int64 on the device: the sum of a prioritised plan's ``timed_arrive`` (B,) less ``bound``, and less the
        cost of the reported node -- how far the plan is from what is possible at the least, and from this search's
        plan; no host read"""
        import torch
        total = timed_arrive.to(torch.int64).sum()
        return torch.stack([total - self.info[_lib.CBS_BOUND].to(torch.int64), total - self.info[_lib.CBS_COST].to(torch.int64)])


class BoundedTimedRoutes(OptimalTimedRoutes):
    """``OptimalTimedRoutes`` with a weight ``w = (w_num, w_den)`` >= 1: the search prefers nodes with few conflicts among
    those within ``w`` of the lower bound, and routes a robot up to ``w`` times later than it could arrive when that saves
    conflicts.  With outcome SOLVED the reported plan is conflict-free and ``cost * w_den <= w_num * bound``.  ``info``
    (ECBS_INFO,) int32 holds the members of ``OptimalTimedRoutes.info`` and the reported node's lb and nconf at
    ``_lib.ECBS_LB`` and ``_lib.ECBS_NCONF``; ``plan``, ``more`` and ``gap`` are the base class's."""
    _work_bytes = staticmethod(_lib.ecbs_work_bytes)
    _info_len = _lib.ECBS_INFO

    def __init__(self, grid, movement, occupancy_threshold, T, sep2, w=(11, 10), lag=1, nodes=4096, expand=1, rounds=512,
                 occupancy_cost_factor=3.0, device=None):
        super().__init__(grid, movement, occupancy_threshold, T, sep2, lag=lag, nodes=nodes, expand=expand, rounds=rounds,
                         occupancy_cost_factor=occupancy_cost_factor, device=device)
        self.w = (int(w[0]), int(w[1]))

    def _call(self, rounds, resume, stream):
        args = _lib.ecbs_args(self.grid, *self._inputs, self.work, self.paths, self.status, self.arrive, self.info,
                              self.nodes, self.expand, rounds, w=self.w, resume=resume, movement=self.movement,
                              occ_threshold=self.threshold, sep2=self.sep2, lag=self.lag)
        _lib.ecbs_device(args, stream=_lib.stream_handle(stream, self.device))
        return self.paths, self.status, self.arrive, self.info

    def ratio(self):
        """(2,) int64 on the device: (cost, bound) of the search as it stands; with outcome SOLVED
        ``cost * w_den <= w_num * bound``; no host read"""
        import torch
        return torch.stack([self.info[_lib.CBS_COST], self.info[_lib.CBS_BOUND]]).to(torch.int64)
