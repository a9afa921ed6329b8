"""Constructed inputs that the wide-window localisation tests share (tests/test_scan_search_cpu.py,
tests/test_gpu_scan_search.py): maps for the pyramid, the launches of the search with their exhaustive results (cached,
read only).  A launch is dict(pose, points, ranges, geom, top_log2, levels, active) with geom the keyword set of
localization_reference.match_ref."""
import functools
import math

import numpy as np

from lidar_reference import scan_ref
from localization_cases import LIDAR, clear_poses, store_world
from localization_reference import edge_distance_ref, project_ref
from robot_mpcs_amd.global_planner import shelf_map
from robot_mpcs_amd.store import STORE
from robot_mpcs_amd.utils.localization import rotation_table
from scan_search_reference import Robot, match_wide_ref, min_pyramid_ref, search_ref, top_bound_ref

WIDE = dict(nxy=40, step_xy=0.0375, nth=20, step_th=0.02)            # 81 x 81 x 41: +-1.5 m, +-0.4 rad
ODD = dict(miss=3, few=5, nan_pose=9, nan_ranges=12, outside=20)     # robots of store_fleet that are not ordinary
INACTIVE = [1, 8, 17, 26, 33, 42, 55, 63]


def default_levels(top_log2, step_xy, sub, cell):
    """enough levels for the window of a top-level block (ScanSearcher's default)"""
    return math.ceil(math.log2((1 << top_log2) * step_xy * sub / cell + 2.0)) + 1


# ---- maps for the pyramid ------------------------------------------------------------------------------------------------
def small_map_12x9():
    g = np.zeros((9, 12))
    g[4:6, 3:9] = 1.0
    return g


@functools.lru_cache(maxsize=None)
def pyramid_case(name):
    """(d2, sub, levels), read only"""
    rng = np.random.default_rng(11)
    if name == "7x5_sub3":
        d2, sub, levels = edge_distance_ref((rng.uniform(size=(7, 5)) < 0.35).astype(float), 0.5, 3, 40), 3, 4
    elif name == "12x9_sub3_beyond_the_map":
        d2, sub, levels = edge_distance_ref(small_map_12x9(), 0.5, 3, 20), 3, 8      # windows of 64 and 128 on 27 x 36
    elif name == "store":
        d2, sub, levels = store_world()[2], 8, 5
    elif name == "128x128_sub2_levels12":
        d2, sub, levels = edge_distance_ref(shelf_map(128, 128, seed=3, aisle=9, shelf=4, gap=6), 0.5, 2, 256), 2, 12
    else:
        raise KeyError(name)
    d2 = np.array(d2)
    d2.setflags(write=False)
    return d2, sub, levels


CPU_PYRAMIDS = ("7x5_sub3", "12x9_sub3_beyond_the_map", "store")
GPU_PYRAMIDS = CPU_PYRAMIDS + ("128x128_sub2_levels12",)


# ---- launches of the search ------------------------------------------------------------------------------------------------
def store_geom(d2=None, sub=8, cap=256, nxy=3, step_xy=0.03, nth=4, step_th=0.01, min_hits=8):
    return dict(max_range=LIDAR["max_range"], d2=store_world()[2] if d2 is None else d2, H=STORE.H, W=STORE.W, sub=sub,
                cap=cap, x0=STORE.x0, y0=STORE.y0, cell=STORE.cell, nxy=nxy, step_xy=step_xy, nth=nth, step_th=step_th,
                rot=rotation_table(nth, step_th), min_hits=min_hits)


def project(pose, t):
    L = LIDAR
    with np.errstate(invalid="ignore"):
        return project_ref(pose, t, L["angle_min"], L["angle_max"], L["offset"], L["height"])


def store_scan(true, rays):
    L = LIDAR
    return scan_ref(true, rays, L["angle_min"], L["angle_max"], L["max_range"], L["offset"], L["height"], store_world()[1])[1]


def store_robots(B, rays, seed, spread, true=None):
    """true poses in the store, their scan and a prior off by up to `spread` (x, y, heading); pose has a stride of 8"""
    rng = np.random.default_rng(seed)
    if true is None:
        true = clear_poses(store_world()[0], B, rng, 2, 0.2)
    t = store_scan(true, rays)
    pose = np.zeros((B, 8))
    pose[:, :3] = true + rng.uniform(-1, 1, (B, 3)) * spread
    pose[:, 3:] = rng.normal(size=(B, 5))
    return pose, t, true


def _launch(pose, t, geom, top_log2, levels=None, active=None, points=None):
    levels = levels or default_levels(top_log2, geom["step_xy"], geom["sub"], geom["cell"])
    return dict(pose=pose, points=project(pose, t) if points is None else points, ranges=t, geom=geom, top_log2=top_log2,
                levels=min(levels, 12), active=active)


def _three_rays(nxy, nth, seed):
    pose, t, _ = store_robots(1, 3, seed, (0.5, 0.5, 0.1))
    t[0] = np.minimum(t[0], 6.0)                                      # (each ray a hit whatever it met)
    return _launch(pose, t, store_geom(nxy=nxy, step_xy=0.02, nth=nth, step_th=0.003, min_hits=1), 3)


def _mirror():
    """Two shelves, columns 2 and 10 of 9 x 13 cells of 0.5 m, mirror images about x = 0; sub 4, cap 4: a fine cell
    beside a face costs 1, every other 4.  The robot stands on the axis and its six rays end 0.44 m short of the two
    faces: four steps of 0.125 m to either side put three ends on a face (3 + 12 = 15 against 24 at the centre), so
    ix = +4 and ix = -4 share the least (score, m) and k decides."""
    g = np.zeros((9, 13))
    g[:, 2] = g[:, 10] = 1.0
    pose = np.array([[0.0, 0.0, 0.5 * math.pi]])
    ends = np.array([[sx * 1.31, dy] for sx in (-1.0, 1.0) for dy in (-0.5, 0.0, 0.5)])
    points = np.concatenate([ends, np.full((6, 1), 0.02)], axis=1)[None]
    t = np.hypot(ends[:, 0], ends[:, 1])[None]
    geom = dict(max_range=10.0, d2=edge_distance_ref(g, 0.5, 4, 4), H=9, W=13, sub=4, cap=4, x0=-3.0, y0=-2.0, cell=0.5,
                nxy=6, step_xy=0.125, nth=1, step_th=0.01, rot=rotation_table(1, 0.01), min_hits=2)
    return _launch(pose, t, geom, 2, points=points)


@functools.lru_cache(maxsize=None)
def launch(name):
    d2 = store_world()[2]
    if name == "one_candidate":
        pose, t, _ = store_robots(1, 1, 0, (0.08, 0.08, 0.03))
        t[0, 0] = 2.5
        return _launch(pose, t, store_geom(nxy=0, step_xy=0.0, nth=0, step_th=0.0, min_hits=1), 3, levels=2)
    if name in ("every_node_a_leaf", "one_top_node_per_rotation"):
        pose, t, _ = store_robots(3, 5, 1, (0.08, 0.08, 0.03))
        return _launch(pose, t, store_geom(nxy=1, step_xy=0.05, nth=1, step_th=0.02, min_hits=2),
                       0 if name == "every_node_a_leaf" else 7)
    if name == "store_fleet":
        pose, t, _ = store_robots(64, 64, 2, (1.5, 1.5, 0.4))
        t[ODD["miss"]] = LIDAR["max_range"]
        t[ODD["few"], 5:] = LIDAR["max_range"]
        pose[ODD["nan_pose"], 0] = math.nan
        t[ODD["nan_ranges"], ::3] = math.nan
        t[ODD["nan_ranges"], 1] = math.inf
        pose[ODD["outside"], 0] += 40.0
        active = np.ones(64, np.int32)
        active[INACTIVE] = 0
        return _launch(pose, t, store_geom(**WIDE), 3, active=active)
    if name == "nxy_127":
        return _three_rays(127, 2, 5)
    if name == "nth_127":
        return _three_rays(20, 127, 6)
    if name == "255_cubed":
        return _three_rays(127, 127, 7)
    if name in ("empty_map", "all_occupied"):
        pose, t, _ = store_robots(4, 64, 4, (0.3, 0.3, 0.1))
        table = np.full_like(d2, 256) if name == "empty_map" else edge_distance_ref(np.ones((STORE.H, STORE.W)), 0.5, 8, 256)
        return _launch(pose, t, store_geom(table, nxy=10, step_xy=0.04, nth=3, step_th=0.02), 2)
    if name == "mirror":
        return _mirror()
    if name == "300_rays":
        pose, t, _ = store_robots(4, 300, 4, (0.3, 0.3, 0.05))
        return _launch(pose, t, store_geom(nxy=9, step_xy=0.04, nth=2, step_th=0.02), 2)
    if name == "12x9_map":
        # a table smaller than a top-level block's window: 27 x 36 fine cells, blocks of 16 steps of 0.2 m = 19 fine cells
        pose, t, _ = store_robots(4, 64, 8, (0.3, 0.3, 0.1))
        pose[:, :2] *= 0.25                                           # (into and around the little map)
        geom = dict(store_geom(edge_distance_ref(small_map_12x9(), 0.5, 3, 20), sub=3, cap=20, nxy=12, step_xy=0.2, nth=1,
                               step_th=0.05), H=9, W=12, x0=-2.0, y0=-1.0, cell=0.5)
        return _launch(pose, t, geom, 4)
    if name == "border":
        # within one cell of the map's border, one robot per side and two in corners: blocks straddle the edge
        lo, hi = STORE.x0 - 0.4 * STORE.cell, STORE.x0 + (STORE.W - 1) * STORE.cell + 0.4 * STORE.cell
        true = np.array([[lo, 0.3, 0.2], [hi, -1.1, 2.0], [0.7, lo, -1.0], [-2.2, hi, 3.0], [lo + 0.2, lo + 0.1, 0.8],
                         [hi - 0.1, hi - 0.3, -2.5]])
        pose, t, _ = store_robots(6, 64, 9, (0.5, 0.5, 0.1), true=true)
        return _launch(pose, t, store_geom(nxy=20, step_xy=0.0375, nth=4, step_th=0.025, min_hits=4), 3)
    raise KeyError(name)


LAUNCHES = ("one_candidate", "every_node_a_leaf", "one_top_node_per_rotation", "store_fleet", "nxy_127", "nth_127",
            "255_cubed", "empty_map", "all_occupied", "mirror", "300_rays", "12x9_map", "border")


@functools.lru_cache(maxsize=None)
def pyramid_of(name):
    L = launch(name)
    pyr = min_pyramid_ref(L["geom"]["d2"], L["levels"])
    pyr.setflags(write=False)
    return pyr


@functools.lru_cache(maxsize=None)
def exhaustive(name):
    """match_wide_ref of the launch, read only"""
    L = launch(name)
    out = match_wide_ref(L["pose"], L["points"], L["ranges"], active=L["active"], **L["geom"])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def searched(name):
    """search_ref of the launch (with its own leaf counts), read only"""
    L = launch(name)
    out = search_ref(L["pose"], L["points"], L["ranges"], pyramid_of(name), L["top_log2"], active=L["active"], **L["geom"])
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def top_bounds(name):
    """(B, ntop) int32: top_bound of the launch; rows of robots that are not searched are None in `rows`"""
    L = launch(name)
    ex = exhaustive(name)
    return [top_bound_ref(Robot(L["pose"][b], L["points"][b], L["ranges"][b], pyramid_of(name), **L["geom"]), L["top_log2"])
            if ex["best"][b] >= 0 else None for b in range(len(L["pose"]))]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def check_refusals(lib, P):
    """Every refusal rmpc_scan_search_device adds to those of rmpc_scan_match_device, the work-size query's and the
    pyramid's: -1 with the entry's own message, never the HIP runtime's.  P stands for every pointer and is never
    dereferenced: each call is refused before any HIP call."""
    import ctypes as C
    L = lib.load_library()

    def refused(rc, want, what):
        msg = L.rmpc_last_error().decode()
        assert rc == -1 and want in msg and "hip" not in msg.lower(), (what, msg)

    def search(B=1, null=False, **kw):
        a = lib.ScanSearchArgs()
        a.struct_size, a.rays, a.range, a.pose_stride, a.min_hits = C.sizeof(lib.ScanSearchArgs), 4, 10.0, 8, 1
        a.H, a.W, a.sub, a.cap, a.x0, a.y0, a.cell = 2, 2, 2, 16, 0.0, 0.0, 0.5
        a.nxy, a.nth, a.step_xy, a.step_th, a.levels, a.top_log2 = 3, 1, 0.03, 0.01, 2, 1
        for k in ("pose", "points", "ranges", "d2", "rot", "pose_out", "best", "score", "pyr", "work"):
            setattr(a, k, P)
        a.work_bytes = lib.scan_search_work_bytes(max(B, 1), 3, 1, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.rmpc_scan_search_device(B, None if null else C.byref(a), None)

    full = lib.scan_search_work_bytes(1, 3, 1, 1)
    assert full == 4 * 3 * 4 * 4 == 4 * lib.scan_search_top_nodes(3, 1, 1)
    for kw, want in [(dict(null=True), "null argument"), (dict(struct_size=C.sizeof(lib.ScanMatchArgs)), "struct_size mismatch"),
                     (dict(B=0), "need B >= 1"), (dict(nxy=-1), "must lie in [0, 127]"), (dict(nxy=128), "must lie in [0, 127]"),
                     (dict(nth=-1), "must lie in [0, 127]"), (dict(nth=128), "must lie in [0, 127]"),
                     (dict(top_log2=-1), "top_log2 must lie in [0, 7]"), (dict(top_log2=8), "top_log2 must lie in [0, 7]"),
                     (dict(levels=0), "levels must lie in [1, 12]"), (dict(levels=13), "levels must lie in [1, 12]"),
                     (dict(pyr=None), "null argument"), (dict(work=None), "null argument"), (dict(d2=None), "null argument"),
                     (dict(work_bytes=full - 1), "work_bytes"), (dict(work_bytes=0), "work_bytes"),
                     (dict(rays=0), "RMPC_MATCH_MAX_RAYS"), (dict(min_hits=0), "min_hits >= 1"),
                     (dict(step_xy=0.0), "a step of 0"), (dict(cap=65536), "cap must lie in [1, 65535]")]:
        refused(search(**kw), want, kw)
    for args in [(0, 3, 1, 1), (1, 128, 1, 1), (1, -1, 1, 1), (1, 3, -1, 1), (1, 3, 128, 1), (1, 3, 1, 8), (1, 3, 1, -1)]:
        assert L.rmpc_scan_search_work_bytes(*args) == -1 and "scan search work bytes" in L.rmpc_last_error().decode(), args
    assert lib.scan_search_work_bytes(3, 127, 127, 0) == 3 * 255 ** 3 * 4
    assert lib.scan_search_work_bytes(2, 127, 127, 7) == 2 * 255 * 2 * 2 * 4
    for kw, want in [(dict(d2=None), "null argument"), (dict(pyr=None), "null argument"), (dict(H=0), "need H, W >= 1"),
                     (dict(H=129, W=128), "RMPC_GRID_MAX_CELLS"), (dict(sub=0), "sub must lie in [1, 8]"),
                     (dict(sub=9), "sub must lie in [1, 8]"), (dict(levels=0), "levels must lie in [1, 12]"),
                     (dict(levels=13), "levels must lie in [1, 12]")]:
        a = dict(dict(H=2, W=2, sub=2, d2=P, levels=2, pyr=P), **kw)
        refused(L.rmpc_grid_min_pyramid_device(a["H"], a["W"], a["sub"], a["d2"], a["levels"], a["pyr"], None), want, kw)
