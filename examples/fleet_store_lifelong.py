#!/usr/bin/env python3
"""Picks that arrive while the boxers are under way, served on lifelong timed tours, entirely on the device (DESIGN.md
26).  The store, the 16 boxers and the loop are those of examples/fleet_store_timed_tours.py.  Wave 0 has 24 picks;
``--waves`` further waves of 16 picks arrive every ``--every`` control steps (16: the first wave takes 27, so part of
the fleet is under way when a wave arrives), together with whatever picks the last dispatch could not place.  ``--replan`` says what a wave does to the plan the fleet is on:

    idle    LifelongTours.dispatch(mode="idle"): the robots that have served their stops and stand parked take the
            picks; the routes of the others are reserved and the idle ones are planned around them in space-time, each
            from the layer it stands at (rmpc_timed_reserve_device, rmpc_timed_tours_replan_device)
    all     LifelongTours.dispatch(mode="all"): every robot is re-planned from its layer, the busy ones with the stops
            they have left, the idle ones with the picks; no table
    static  TourPlanner.plan(available=idle) + TourFollower: the idle robots descend the fields of their
            picks, blind to the others' routes

    python examples/fleet_store_lifelong.py [--waves 2] [--every 16] [--replan idle|all|static] [--steps 400] [--seed 0]
                                            [--dwell 3]

The loop ends once every planned pick of every wave is served (and stood on for ``dwell`` steps on timed tours), or
``--steps`` control steps after the last dispatch.  Prints one JSON line: the report fields of the store examples, the
picks planned and served per wave, the step of the last service, the least distance between two end links less
r_i + r_j, the failed share, the fewest consecutive steps a robot stood on a pick, the sum of ``clash``, the plan
failures, and the ms per dispatch (wall clock around the call, the device synchronised before and after).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEP2, START_SEP2, LAG, T, ORDERS = 9, 25, 1, 255, 16        # as examples/fleet_store_timed_tours.py
K_LIDAR, K_FLEET, RAYS = 4, 2, 64
FOLLOW_M = 1.3
MODES = ("idle", "all", "static")
WAVE0, WAVE = 24, 16


def spaced_cells(ok, n, rng, W, sep2):
    """n cells of the mask ``ok`` drawn from ``rng``, pairwise at least sep2 (squared cells) apart"""
    free, out = np.flatnonzero(ok.ravel()), []
    while len(out) < n:
        c = int(rng.choice(free))
        if all((c // W - q // W) ** 2 + (c % W - q % W) ** 2 >= sep2 for q in out):
            out.append(c)
    return np.array(out, np.int32)


class StaticWaves:
    """the static plan behind LifelongTours' interface: ``TourPlanner.plan`` for the idle robots, one ``TourFollower``"""

    def __init__(self, grid, K, S, threshold, tol):
        self.grid, self.K, self.S, self.threshold, self.tol = grid, K, S, threshold, tol
        self.follower = None

    def _plan(self, cells, picks, idle):
        import torch
        from robot_mpcs_amd.global_planner import TourPlanner
        tp = TourPlanner(self.grid, np.asarray(picks, np.int32), self.K)
        paths, lens, stop_at = tp.plan(cells, available=None if idle is None else idle.to(torch.int32))
        owned = torch.zeros(tp.T, dtype=torch.bool, device=paths.device)
        owned[tp.tours[(tp.tours >= 0) & (stop_at >= 0)].long()] = True
        return tp, paths.clone(), lens.clone(), stop_at.clone(), tp.goal_cells[~owned].cpu().numpy()

    def start(self, starts, picks):
        import torch
        from robot_mpcs_amd.global_planner import TourFollower
        S = self.S
        tp, paths, lens, stop_at, left = self._plan(starts, picks, None)
        self.cells = starts.clone()
        self.follower = TourFollower(paths, lens, stop_at, S.W, S.x0, S.y0, S.cell, threshold=self.threshold, stop_tol=self.tol)
        self.stop_cells, self.nstops = tp.goal_cells_of(), (stop_at >= 0).sum(1).to(torch.int32)
        self.served_before = torch.zeros((), dtype=torch.int64, device=paths.device)
        return left

    def idle(self):
        fol = self.follower
        return (fol.leg >= self.nstops) & (fol.idx >= fol.lens - 1)

    def dispatch(self, picks, mode=None):
        import torch
        fol, idle = self.follower, self.idle()
        at = fol.paths.gather(1, fol.idx.long().clamp(min=0)[:, None])[:, 0]
        self.cells = torch.where(fol.lens > 0, at, self.cells).contiguous()
        tp, paths, lens, stop_at, left = self._plan(self.cells, picks, idle)
        on = idle[:, None]
        self.served_before = self.served_before + ((fol.served >= 0) & on).sum()
        fol.paths, fol.lens = torch.where(on, paths, fol.paths).contiguous(), torch.where(idle, lens, fol.lens).contiguous()
        fol.stop_at = torch.where(on, stop_at, fol.stop_at).contiguous()
        fol.idx, fol.leg = fol.idx * ~idle, fol.leg * ~idle
        fol.served = torch.where(on, torch.full_like(fol.served, -1), fol.served)
        self.stop_cells = torch.where(on, tp.goal_cells_of(), self.stop_cells)
        self.nstops = torch.where(idle, (stop_at >= 0).sum(1).to(torch.int32), self.nstops)
        return left

    def served_count(self):
        return self.served_before + self.follower.served_count()


def run(B=16, K=2, waves=2, every=16, steps=400, seed=0, dev="cuda:0", replan="idle", dwell=3, orders=ORDERS, check_every=4,
        threshold=FOLLOW_M):
    import torch
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.fleet import MixedFleetShard
    from robot_mpcs_amd.global_planner import LifelongTours, pick_spaced_tours, png_values
    from robot_mpcs_amd.store import STORE as S, BoxerStore, clear_cells, store_map

    if replan not in MODES:
        raise ValueError("replan must be one of " + ", ".join(MODES))
    rng = np.random.default_rng(seed)
    raw = store_map(seed)
    g_raw = torch.from_numpy(png_values(raw)).to(dev)
    g_inf = torch.empty_like(g_raw)
    _lib.grid_inflate_device(g_raw, g_inf, S.cell, S.size_robot, 0.29)
    ok = clear_cells(raw, S.clear_cells) & (g_inf.cpu().numpy() < 0.8)
    starts, picks0 = pick_spaced_tours(raw > 0.5, ok, B, WAVE0, rng, S.x0, S.y0, S.cell, SEP2, START_SEP2)
    fleet = BoxerStore(B, seed, dev, K_LIDAR, RAYS, starts, rng, neighbours=K_FLEET)
    wave_picks = [spaced_cells(ok, WAVE, rng, S.W, SEP2) for _ in range(waves)]
    tol = MixedFleetShard.ARRIVE_TOL["cfg3"]
    timed = replan != "static"
    if timed:
        ll = LifelongTours(g_inf, K, T, SEP2, LAG, dwell, orders, W=S.W, x0=S.x0, y0=S.y0, cell=S.cell, threshold=threshold,
                           stop_tol=tol, seed=seed)
    else:
        ll = StaticWaves(g_inf, K, S, threshold, tol)
    left = ll.start(torch.from_numpy(starts).to(dev), picks0)
    planned = [WAVE0 - len(left)]
    need = dwell if timed else 0

    far = torch.full((1, 2), 1e9, dtype=torch.float64, device=dev)
    def pick_centres():
        c = ll.stop_cells.long()
        xy = torch.stack([S.x0 + (c % S.W) * S.cell, S.y0 + (c // S.W) * S.cell], 2)
        return torch.where((c >= 0)[:, :, None], xy, far)
    pick_xy = pick_centres()
    stood = torch.zeros((B, K), dtype=torch.int64, device=dev)
    stood_max = torch.zeros((B, K), dtype=torch.int64, device=dev)
    least_stood = torch.full((), 1 << 30, dtype=torch.int64, device=dev)

    last_srv = torch.full((), -1, dtype=torch.int64, device=dev)

    def fold(rows):
        """the served stops of ``rows`` (their records end with a dispatch) -> (least_stood, last_srv) with them"""
        srv = ll.follower.served
        m = (srv >= 0) & rows[:, None]
        return (torch.minimum(least_stood, torch.where(m, stood_max, torch.full_like(stood_max, 1 << 30)).min()),
                torch.maximum(last_srv, torch.where(m, srv, torch.full_like(srv, -1)).max().long()))

    upper = torch.triu(torch.ones((B, B), dtype=torch.bool, device=dev), diagonal=1)
    rsum = fleet.rad[:, None] + fleet.rad[None, :]
    min_gap = torch.full((), float("inf"), dtype=torch.float64, device=dev)
    gap_step = torch.zeros((), dtype=torch.int64, device=dev)
    x = fleet.x
    ee = x[:, :2] + S.ee_offset * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)
    served_by_wave, dispatch_ms, wave, last_dispatch = [], [], 0, 0
    everyone = torch.ones(B, dtype=torch.bool, device=dev)

    torch.cuda.synchronize()
    t_loop = time.perf_counter()
    done = 0
    for step in range(waves * every + steps):
        if wave < waves and step == (wave + 1) * every:
            rows = everyone if replan == "all" else ll.idle()
            least_stood, last_srv = fold(rows)
            served_by_wave.append(int(ll.served_count().item()))
            picks = np.concatenate([left, wave_picks[wave]]).astype(np.int32)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            left = ll.dispatch(picks, replan)
            torch.cuda.synchronize()
            dispatch_ms.append(round(1e3 * (time.perf_counter() - t0), 3))
            planned.append(len(picks) - len(left))
            pick_xy = pick_centres()
            stood, stood_max = stood * ~rows[:, None], stood_max * ~rows[:, None]
            wave, last_dispatch = wave + 1, step
        ll.follower.step(ee, fleet.goal)
        fleet.scan()
        ee = fleet.drive()
        d = (ee[:, None, :] - ee[None, :, :]).norm(dim=2)
        gap = torch.where(upper, d - rsum, torch.full_like(d, float("inf"))).min()
        gap_step = torch.where(gap < min_gap, torch.full_like(gap_step, step), gap_step)
        min_gap = torch.minimum(min_gap, gap)
        on = (ee[:, None, :] - pick_xy).norm(dim=2) <= tol
        stood = (stood + 1) * on
        stood_max = torch.maximum(stood_max, stood)
        done = step + 1
        if check_every and done % check_every == 0:
            if wave == waves and int(ll.served_count().item()) == sum(planned) and int(fold(everyone)[0].item()) >= need:
                break
            if wave == waves and step - last_dispatch >= steps:
                break
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t_loop) / max(done, 1)
    least_stood, last_srv = fold(everyone)
    total = int(ll.served_count().item())
    served_by_wave.append(total)
    extra = {}
    if timed:
        extra = dict(clash_sum=int(ll.clash_sum.item()), plan_failures=int(ll.plan_failures.item()),
                     plan_unserved=int(ll.plan_unserved.item()), dwell=dwell)
    out = dict(fleet.report(), replan=replan, waves=waves, every=every, tour_K=K, steps=done, seed=seed, K_fleet=K_FLEET,
               picks_planned=planned, picks_left=int(len(left)),
               picks_served=[b - a for a, b in zip([0] + served_by_wave, served_by_wave)], picks_served_total=total,
               last_service_step=int(last_srv.item()) + 1, steps_after_last_dispatch=done - last_dispatch,
               min_pair_gap_m=float(min_gap.item()), min_pair_gap_step=int(gap_step.item()),
               min_steps_on_a_pick=int(least_stood.item()) if total else 0, dispatch_ms=dispatch_ms,
               ms_per_step=round(ms, 3), stop_tol_m=tol, **extra)
    fleet.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=2)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--replan", default="idle", choices=MODES)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dwell", type=int, default=3)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(waves=a.waves, every=a.every, steps=a.steps, seed=a.seed, replan=a.replan, dwell=a.dwell)))


if __name__ == "__main__":
    main()
