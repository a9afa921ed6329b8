"""The boxer fleet in the store, once: the store's frame and model constants (``STORE``), the masks and distances the
store examples measure with (``clear_cells``, ``box_distance``, ``map_errors``) and ``BoxerStore``, the closed-loop
block of B boxers with a lidar in that store.  A store example is ``BoxerStore(...)`` once, then per control step whatever
fills the scene (``RouteFollower.step``, ``BoxerStore.scan``, ``FleetMap.mark``, a re-plan, in the loop's own order) and
``BoxerStore.drive``.  Importing this module needs no GPU.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from .fleet import dev_f64, limit_tensors, make_block, step_block
from .global_planner import RouteFollower, cell_xy, shelf_map, store_routes
from .scenarios import LIMITS, make_scenario
from .utils.lidar import LidarPlanes, boxes_from_grid
from .utils.mapping import FleetMap

_STORE = dict(
    # the store: 41 x 41 cells of 0.45 m centred on the origin (inside the boxer's +-10 m position limits); aisles of
    # 6 cells (2.7 m) and passages of 5 cells through the shelves, for a body of r_body = 0.6 m around the end link
    H=41, W=41, cell=0.45, x0=-9.0, y0=-9.0, aisle=6, shelf=2, gap=5,
    size_robot=0.45,     # k = 1, as in fleet_global_route.py: the route alone does not keep r_body clear
    r_body=0.6,
    ee_offset=0.4,       # ee_link ahead of base_link (boxer_fk.urdf); the lidar sits there too (compute_point_cloud)
    # starts and goals: no shelf cell within this many cells (Chebyshev), i.e. >= 1.125 m from a shelf's edge, so that
    # the end link starts outside r_body of every shelf whatever the heading
    clear_cells=2)
STORE = namedtuple("Store", _STORE)(**_STORE)     # the record of the store's frame and model constants


def store_map(seed):
    """the store's true map (H, W): ``shelf_map`` with the store's shelves, from a generator of its own"""
    return shelf_map(STORE.H, STORE.W, seed=seed, aisle=STORE.aisle, gap=STORE.gap, shelf=STORE.shelf)


def clear_cells(raw, k):
    """free cells with no occupied cell within Chebyshev distance k"""
    H, W = raw.shape
    occ = np.pad(raw > 0.5, k, constant_values=True)
    near = np.zeros((H, W), dtype=bool)
    for dr in range(-k, k + 1):
        for dc in range(-k, k + 1):
            near |= occ[k + dr:k + dr + H, k + dc:k + dc + W]
    return ~near


def clear_routes(raw, B, rng, device):
    """``store_routes`` in the store's frame among the cells ``STORE.clear_cells`` clear of every shelf"""
    return store_routes(raw, B, rng, STORE.x0, STORE.y0, STORE.cell, STORE.size_robot, device,
                        ok=clear_cells(raw, STORE.clear_cells))


def box_distance(p, boxes):
    """(B,) least distance from the points p (B, 2) to the boxes (nbox, 4) = (cx, cy, lx, ly); 0 inside"""
    return ((p[:, None, :] - boxes[None, :, :2]).abs() - 0.5 * boxes[None, :, 2:]).clamp(min=0.0).norm(dim=2).min(dim=1).values


def map_errors(fmap, raw):
    """(seen, wrong): the cells of the ``FleetMap`` with evidence, and those among them whose class differs from the
    true map ``raw``.  Reads the device."""
    import torch
    seen = (fmap.hits.long() + fmap.misses.long()) > 0
    truth = torch.from_numpy(raw > 0.5).to(fmap.device)
    wrong = seen & ((fmap.occupancy(0.0, 1.0, 0.0) > 0.5) != truth)
    return int(seen.sum().item()), int(wrong.sum().item())


class BoxerStore:
    """B boxers (boxerMpc.yaml with K linear constraints) on the cells ``start_cells`` of the store ``store_map(seed)``,
    headings drawn from ``rng`` (B draws, after whatever the caller drew for the start cells), each with a lidar of
    ``rays`` rays at its end link whose planes are the scene's ``lin_constrs`` (``lidar=False``: in an empty world) and
    its own position as its first goal.  Owns ``raw``, ``boxes`` (nbox, 4), the scenario ``sc``, ``lp``
    (``LidarPlanes``), ``goal`` (B, 3), the block ``f`` with its ``x, z, ef``, and on the device the statistics
    ``fails``, ``ee_clear``, ``base_clear`` (B,) of the ``steps`` control steps driven so far.  With ``neighbours`` > 0
    the model has K + neighbours linear constraints: ``planes`` (B, N, K + neighbours, 4) holds the lidar's planes in
    its first K slots (copied by ``scan``) and the fleet's separating planes (``npl``: ``NeighbourPlanes`` within
    ``neighbour_range`` m) in the others."""

    def __init__(self, B, seed, device, K, rays, start_cells, rng, lidar=True, neighbours=0, neighbour_range=3.0):
        import torch
        S = STORE
        self.B, self.K, self.rays, self.device = B, K, rays, device
        self.raw = store_map(seed)
        boxes = boxes_from_grid(self.raw, S.x0, S.y0, S.cell)
        self.boxes = dev_f64(boxes, device)
        self.sc = sc = make_scenario("boxer", B=B, seed=seed, number_obstacles=K + neighbours)
        xinit = np.zeros((B, sc.desc["nx"]))
        xinit[:, :2] = cell_xy(start_cells, S.W, S.x0, S.y0, S.cell)
        xinit[:, 2] = rng.uniform(-math.pi, math.pi, B)
        self.lp = LidarPlanes(B, sc.desc["N"], K, boxes=boxes if lidar else None, rays=rays, offset=(S.ee_offset, 0.0),
                              device=device)
        self.goal = dev_f64(np.concatenate([xinit[:, :2], np.zeros((B, 1))], 1), device)
        self.rad = dev_f64(np.full(B, S.r_body), device)
        self.planes, self.npl = self.lp.planes, None
        if neighbours > 0:
            from .utils.separation import NeighbourPlanes
            self.planes = torch.zeros((B, sc.desc["N"], K + neighbours, 4), dtype=torch.float64, device=device)
            self.npl = NeighbourPlanes(B, sc.desc["N"], neighbours, range=neighbour_range, heading=1,
                                       offset=(S.ee_offset, 0.0), slot0=K, planes=self.planes)
        self.f = f = make_block(sc.desc, sc.setup["mpc"]["weights"], B, xinit, device, goal=self.goal,
                                r_body=self.rad, lin_constrs=self.planes,
                                **limit_tensors(*LIMITS["boxer"], B, device))
        self.x, self.z, self.ef = f["x"], f["z"], f["ef"]
        self.fails = torch.zeros((), dtype=torch.int64, device=device)
        self.ee_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=device)
        self.base_clear = torch.full((B,), float("inf"), dtype=torch.float64, device=device)
        self.steps = 0

    def follower(self, threshold, paths=None, lens=None, max_len=None):
        """A ``RouteFollower`` in the store's frame on (paths, lens), else on B empty routes of ``max_len`` cells
        (``plan_batch``'s default: ``replace()`` then never has to pad)"""
        import torch
        S = STORE
        if paths is None:
            max_len = max_len if max_len is not None else min(S.H * S.W, 4 * (S.H + S.W))
            paths = torch.zeros((self.B, max_len), dtype=torch.int32, device=self.device)
            lens = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        return RouteFollower(paths, lens, S.W, S.x0, S.y0, S.cell, threshold=threshold)

    def fleet_map(self):
        """An empty ``FleetMap`` of the store for this fleet's scans"""
        S, lp = STORE, self.lp
        return FleetMap(self.B, S.H, S.W, S.x0, S.y0, S.cell, self.rays, lp.max_range, lp.offset, lp.height,
                        device=self.device)

    def scan(self):
        """``LidarPlanes.step`` at the current poses, seeded by the previous plan (before the first ``drive``: by none);
        with neighbours, ``NeighbourPlanes.step`` beside it.  Returns the scene's planes."""
        first = self.steps == 0
        z, ef = (None, None) if first else (self.z, self.ef)
        planes = self.lp.step(self.x, z, ef)
        if self.npl is None:
            return planes
        self.planes[:, :, :self.K].copy_(planes)
        return self.npl.step(self.x, self.rad, z, ef)

    def drive(self):
        """One control step (``step_block``), then the statistics of the new poses.  Returns the end links' positions
        (B, 2)."""
        import torch
        step_block(self.f, previous_plan=True)
        self.steps += 1
        self.fails += (self.ef < 0).sum()
        x = self.x
        ee = x[:, :2] + STORE.ee_offset * torch.stack([torch.cos(x[:, 2]), torch.sin(x[:, 2])], 1)
        self.ee_clear = torch.minimum(self.ee_clear, box_distance(ee, self.boxes))
        self.base_clear = torch.minimum(self.base_clear, box_distance(x[:, :2], self.boxes))
        return ee

    def report(self):
        """The fields every store example prints.  Reads the device."""
        fails, ee, base = int(self.fails.item()), self.ee_clear, self.base_clear
        return dict(robots=self.B, K=self.K, rays=self.rays, fused=self.f["s"].is_fused(), nbox=int(len(self.boxes)),
                    failed_solves=fails, failed_share=fails / (self.B * max(self.steps, 1)),
                    min_ee_clearance_m=float(ee.min().item()), ee_clearance_p10=float(ee.quantile(0.1).item()),
                    ee_below_half_r_body=int((ee < 0.5 * STORE.r_body).sum().item()),
                    min_base_clearance_m=float(base.min().item()), base_inside=int((base <= 0).sum().item()),
                    r_body=STORE.r_body)

    def close(self):
        self.f["s"].close()
