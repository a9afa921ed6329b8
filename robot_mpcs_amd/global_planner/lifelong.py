"""Lifelong timed tours: picks arrive while the fleet is under way.  ``rebase`` brings the plan the
followers are on into a frame in which every robot that is re-planned begins at a layer of its own; ``LifelongTours``
reserves the routes that are kept (``rmpc_timed_reserve_device``), re-plans the others around them from where they stand
(``rmpc_timed_tours_replan_device``, include/rmpc_timed_replan.h) and hands the merged plan to the follower.  Tensor
operations and launches on one stream; one host read per dispatch (the picks that found no robot), none per control
step."""
from __future__ import annotations

import numpy as np

from .. import _lib
from .batch import _dev_tensor
from .timed_tours import TimedTourFollower
from .tours import TourPlanner


def rebase(paths, serve_at, idx, leg, active):
    """paths (B, T + 1), serve_at (B, K), idx, leg, active (B,) integer tensors on one device (CPU tensors too) ->
    (paths', serve_at', idx', begin, start (all int32), m (a 0-dim int64 tensor)).  For an active robot e_b is the first
    layer of the standing run that ends at idx_b, the least i with p[i .. idx_b] all one cell; m is the least of the
    kept robots' idx and the active robots' e_b.  Every path is shifted by the same m, p'[t] = p[min(t + m, T)] -- a
    uniform shift keeps the plan's guarantee --, pending serve_at entries are lowered by m and served ones become -1,
    idx' = idx - m for a kept robot, begin_b = idx'_b = e_b - m and start_b = p[idx_b] for an active one (begin = idx'
    and start = p[idx] are written for the kept ones too; a re-plan does not read them).  Tensor operations only."""
    import torch
    B, T = int(paths.shape[0]), int(paths.shape[1]) - 1
    idx = idx.long().clamp(0, T)
    cols = torch.arange(T + 1, device=paths.device)
    here = paths.gather(1, idx[:, None])
    differs = (paths != here) & (cols[None, :] < idx[:, None])
    run = torch.where(differs, cols[None, :] + 1, torch.zeros_like(cols)[None, :]).max(1).values
    e = torch.where(active != 0, run, idx)
    m = e.min()
    shifted = paths.gather(1, (cols[None, :] + m).clamp(max=T).expand(B, -1))
    K = int(serve_at.shape[1])
    pending = (torch.arange(K, device=paths.device)[None, :] >= leg.long()[:, None]) & (serve_at >= 0)
    sa = torch.where(pending, serve_at.long() - m, torch.full_like(serve_at, -1).long())
    i32 = torch.int32
    new_idx = (e - m).to(i32)
    return shifted.to(i32).contiguous(), sa.to(i32).contiguous(), new_idx, new_idx.clone(), here[:, 0].to(i32).contiguous(), m


class LifelongTours:
    """Timed tours that take picks while the fleet is under way.  grid (H, W) occupancy, K the most picks per robot and
    dispatch, T the window, ``sep2``, ``lag``, ``dwell`` and ``orders`` as in ``TimedTours``; W, x0, y0, cell,
    ``threshold`` and ``stop_tol`` are the follower's.  ``start`` plans the first wave from layer 0 (``TimedTours.plan``)
    and makes ``follower``, a ``TimedTourFollower``; ``dispatch`` re-plans in the frame ``follower`` is in and swaps the
    merged plan in.  ``stop_cells`` (B, K) and ``nstops`` (B,) say which cells every robot is to serve in the plan it
    follows; ``served_before``, ``clash_sum``, ``plan_failures`` and ``plan_unserved`` add up over the dispatches (device
    tensors), ``last`` holds what the last dispatch planned."""

    MODES = ("idle", "all")

    def __init__(self, grid, K, T, sep2, lag=1, dwell=0, orders=4, W=None, x0=0.0, y0=0.0, cell=1.0, threshold=1.3,
                 stop_tol=0.1, movement="8N", seed=0, device=None):
        import torch
        dev = torch.device(device) if device is not None else (grid.device if torch.is_tensor(grid) else torch.device("cuda", 0))
        self.grid = _dev_tensor(grid, torch.float64, dev)
        self.device, self.H, self.Wd = dev, int(self.grid.shape[0]), int(self.grid.shape[1])
        self.K, self.T, self.sep2, self.lag, self.dwell = int(K), int(T), int(sep2), int(lag), int(dwell)
        self.orders, self.movement, self.seed = orders, movement, seed
        self.geom = (int(W) if W is not None else self.Wd, float(x0), float(y0), float(cell), float(threshold), float(stop_tol))
        self.follower = None

    def _planner(self, picks):
        picks = np.asarray(picks, dtype=np.int32).reshape(-1)
        return TourPlanner(self.grid, picks, min(self.K, len(picks)), movement=self.movement, device=self.device)

    def start(self, start_cells, picks):
        """the first wave, planned from layer 0 -> the picks (numpy) that found no robot or no service in the window"""
        import torch
        from .timed_tours import TimedTours
        tp = self._planner(picks)
        tt = TimedTours(tp, self.T, self.sep2, lag=self.lag, dwell=self.dwell, orders=self.orders, park="last", seed=self.seed)
        paths, serve_at, status, served, arrive, best = tt.plan(start_cells)
        g = int(best.item())                               # (the host read of the plan: which order to follow)
        if g < 0:
            raise ValueError("LifelongTours: no row of orders is a permutation")
        dev, B = self.device, int(paths.shape[1])
        self.B, self.orders = B, tt.orders
        W, x0, y0, cell, threshold, stop_tol = self.geom
        sa = self._padded(serve_at[g])
        self.follower = TimedTourFollower(paths[g].clone(), sa, W, x0, y0, cell, threshold, stop_tol, self.sep2, self.lag)
        self.stop_cells = self._padded(tp.goal_cells_of())
        self.nstops = served[g].clone()
        self.work = torch.empty(_lib.timed_replan_work_bytes(self.H, self.Wd, self.T, int(tt.orders.shape[0])),
                                dtype=torch.uint8, device=dev)
        self.res = torch.empty(_lib.timed_reserve_words(self.H, self.Wd, self.T), dtype=torch.int64, device=dev)
        self.clash = torch.zeros(B, dtype=torch.int32, device=dev)
        z = lambda: torch.zeros((), dtype=torch.int64, device=dev)
        self.served_before, self.clash_sum, self.plan_failures, self.plan_unserved = z(), z(), (status[g] > 0).sum(), z()
        self.plan_unserved = self.plan_unserved + tt.unserved[g]
        self.last = dict(best=g, active=torch.ones(B, dtype=torch.int32, device=dev), m=z())
        return self._left(tp.goal_cells, tp.tours, served[g], torch.ones(tp.T, dtype=torch.bool, device=dev))

    def _padded(self, a):
        """(B, k <= K) -> (B, K) with -1"""
        import torch
        out = torch.full((int(a.shape[0]), self.K), -1, dtype=torch.int32, device=a.device)
        out[:, :a.shape[1]] = a
        return out

    @staticmethod
    def _left(goal_cells, stops, served, wanted):
        """the cells among ``goal_cells [wanted]`` that no robot serves in its plan: those that are not among the first
        ``served`` stops of a robot (rows with served = 0 place nothing)"""
        import torch
        col = torch.arange(int(stops.shape[1]), device=stops.device)[None, :]
        placed = stops[(stops >= 0) & (col < served[:, None])].long()
        left = wanted.clone()
        left[placed] = False
        return goal_cells[left].cpu().numpy()              # (the host read of a dispatch)

    def idle(self):
        """(B,) bool: every stop served, and standing on the parking cell"""
        fol = self.follower
        here = fol.paths.gather(1, fol.idx.long().clamp(0, self.T)[:, None])[:, 0]
        return (fol.leg >= self.nstops) & (here == fol.paths[:, self.T])

    def dispatch(self, picks, mode="idle", stream=None):
        """new ``picks`` (cells) -> the picks (numpy) that found no robot or no service in the window, and in mode
        "all" the stops a busy robot had left that its new plan does not serve, for the next dispatch.  mode "idle": the idle robots take the picks and are re-planned around the others' reserved routes;
        "all": every robot is re-planned from its layer, the busy ones with their remaining stops, with no table.
        rebase, reserve, re-plan, merge and ``replace`` run on ``stream`` (a ``torch.cuda.Stream``; None = the current
        one); the host reads the best order and the picks left."""
        import torch
        if mode not in self.MODES:
            raise ValueError("LifelongTours: mode must be 'idle' or 'all'")
        with torch.cuda.stream(stream):
            fol, dev, B, K, T = self.follower, self.device, self.B, self.K, self.T
            i32 = torch.int32
            st = torch.cuda.current_stream(dev).cuda_stream
            idle = self.idle()
            active = (idle if mode == "idle" else torch.ones_like(idle)).to(i32)
            paths, serve_at, idx, begin, start, m = rebase(fol.paths, fol.serve_at, fol.idx, fol.leg, active)
            tp = self._planner(picks)
            tours, lens = tp.assign(start, available=idle.to(i32))
            Tn = tp.T
            # the stops a busy robot that is re-planned has left, moved to the front; their cells and the robots' own cells get fields
            # behind the picks': goal_cells = picks, the B K cells left (a robot's own cell where there is none), B own
            col = torch.arange(K, device=dev)[None, :]
            src = col + fol.leg.long()[:, None]
            has = (src < self.nstops.long()[:, None]) & (~idle & active.bool())[:, None]
            left_cells = torch.where(has, self.stop_cells.gather(1, src.clamp(max=K - 1)), torch.full_like(self.stop_cells, -1))
            extra = torch.cat([torch.where(has, left_cells, start[:, None].expand(-1, K)).reshape(-1), start]).contiguous()
            fields = torch.empty((Tn + B * K + B, self.H, self.Wd), dtype=torch.float64, device=dev)
            fields[:Tn].copy_(tp.fields)
            fstat = torch.empty(B * K + B, dtype=i32, device=dev)
            _lib.grid_fields_device(tp.grid, extra, fields[Tn:], fstat, tp.movement, tp.occ, tp.factor, stream=st)
            goal_cells = torch.cat([tp.goal_cells, extra]).contiguous()
            own_left = (Tn + torch.arange(B, device=dev)[:, None] * K + col).to(i32)
            stops = torch.where(idle[:, None], self._padded(tours), torch.where(has, own_left, torch.full_like(own_left, -1)))
            n = torch.where(idle, lens, has.sum(1).to(i32)).contiguous()
            own = (Tn + B * K + torch.arange(B, device=dev)).to(i32)
            last = stops.gather(1, (n.long() - 1).clamp(min=0)[:, None])[:, 0]
            park = torch.where(n > 0, last, own).contiguous()
            stops = stops.clamp(min=0).contiguous()        # (entries past len are not read)
            res0 = None
            if mode == "idle":
                _lib.timed_reserve_device(paths, self.res, self.H, self.Wd, self.sep2, self.lag, use=(1 - active).contiguous(),
                                          clear=True, stream=st)
                res0 = self.res
            G = int(self.orders.shape[0])
            out = dict(paths=torch.empty((G, B, T + 1), dtype=i32, device=dev), serve_at=torch.empty((G, B, K), dtype=i32, device=dev),
                       key=torch.empty(G, dtype=torch.int64, device=dev), best=torch.empty(1, dtype=i32, device=dev),
                       unserved=torch.empty(G, dtype=i32, device=dev))
            out.update({k: torch.empty((G, B), dtype=i32, device=dev) for k in ("status", "arrive", "served")})
            args = _lib.timed_tours_args(tp.grid, start, stops, n, park, fields, goal_cells, self.orders, self.work, out["paths"],
                                         out["status"], out["arrive"], out["key"], out["best"], out["serve_at"], out["served"],
                                         out["unserved"], dwell=self.dwell, movement=tp.movement, occ_threshold=tp.occ,
                                         sep2=self.sep2, lag=self.lag)
            x = _lib.timed_replan_args(self.work, res0, active, begin, self.clash)
            _lib.timed_tours_replan_device(args, x, stream=st)
            g = int(out["best"].item())                    # (the host read of the plan: which order to follow)
            if g < 0:
                raise ValueError("LifelongTours: no row of orders is a permutation")
            on = active.bool()
            new_paths = torch.where(on[:, None], out["paths"][g], paths)
            new_sa = torch.where(on[:, None], out["serve_at"][g], serve_at)
            new_leg = torch.where(on, torch.zeros_like(fol.leg), fol.leg)
            cells = goal_cells[stops.long()]
            served = out["served"][g]
            self.stop_cells = torch.where(on[:, None], torch.where(col < served[:, None], cells, torch.full_like(cells, -1)),
                                          self.stop_cells)
            self.nstops = torch.where(on, served, self.nstops)
            was = fol.served
            self.served_before = self.served_before + ((was >= 0) & on[:, None]).sum()
            self.clash_sum = self.clash_sum + self.clash.sum()
            self.plan_failures = self.plan_failures + (out["status"][g] > 0).sum()
            self.plan_unserved = self.plan_unserved + out["unserved"][g]
            fol.replace(new_paths, new_sa, idx, new_leg)
            fol.served = torch.where(on[:, None], fol.served, was)         # a kept robot keeps its record
            self.last = dict(out, best=g, active=active, begin=begin, start=start, m=m, stops=stops, lens=n, park=park,
                             goal_cells=goal_cells, fields=fields, tours=tours, tour_len=lens, rebased=(paths, serve_at, idx))
            # what goes back to the caller: the picks, and the stops a busy robot had left, that the plan does not serve
            wanted = torch.zeros(int(goal_cells.shape[0]), dtype=torch.bool, device=dev)
            wanted[:Tn] = True
            wanted[own_left[has].long()] = True
            return self._left(goal_cells, stops, served * active, wanted)

    def served_count(self):
        """() int64 on the device: the stops served so far, over every dispatch"""
        return self.served_before + self.follower.served_count()
