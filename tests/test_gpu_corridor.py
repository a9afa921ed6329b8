"""Safe corridors on the device (rmpc_grid_occ_sums_device, rmpc_grid_corridor_device, include/rmpc_corridor.h,
DESIGN.md 29) against the restatement of tests/corridor_reference.py: the summed-area table bit for bit on the edge
shapes and at the wavefront's 64-cell steps; rectangles, statuses and the uint64 view of the planes equal on every free
cell of the small maps and on seeded points (cell boundaries, occupied cells, outside, NaN, infinities) at the sizes
where the launch's blocks switch, into buffers prefilled with a sentinel so that the slots beside the corridor's four
must keep it; ``MapCorridors`` against the two entries called by hand; one small closed loop of the store example.

Where a plane is not a number (a point that is not finite) the comparison is of *being* NaN, not of the NaN's sign and
payload (``canonical_bits``): inf - inf yields the processor's default NaN, which differs between the host that runs the
restatement and the device.  Every other double is compared in all 64 bits."""
import numpy as np
import pytest

from corridor_cases import (EXACT, FRAME, OCC, free_centres, hand_map, random_points, small_maps, sparse_map, store_frame,
                            store_raw, sums_maps)
from corridor_reference import canonical_bits, corridor_ref, occ_sums_ref
from example_loader import load_example
from gpu_support import DEV, _t

pytestmark = pytest.mark.gpu

FILL, FILL_F = -9, -7.0
NOBST, SLOT0 = 7, 2
REACHES = (1, 2, 8, 64, 256)
# The closed loop's bound.  A solve counts as converged with flag 1 or 2.  Flag 1 stops with every inequality row above
# -tol_ineq = -1e-8 (the descriptor's options), flag 2 (the acceptable level) with feasibility <= 1e-6; the
# larger of the two is what the stopping rule admits on a LinearConstraints row, whose unit is metres (|a| = 1).
ADMITTED_VIOLATION = 1e-6
REFS = {}


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    from robot_mpcs_amd.utils import MapCorridors
    return dict(torch=torch, lib=_lib, MapCorridors=MapCorridors)


def device_sums(rt, grid):
    torch, lib = rt["torch"], rt["lib"]
    H, W = grid.shape
    S = torch.full((H + 1, W + 1), FILL, dtype=torch.int32, device=DEV)
    assert S.numel() * 4 == lib.corridor_sums_bytes(H, W)
    lib.grid_occ_sums_device(_t(torch, grid), S, OCC)
    return S


# ---- the summed-area table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sums_maps()))
def test_sums_equal_the_cumsum_bit_for_bit(rt, name):
    grid = sums_maps()[name]
    got = device_sums(rt, grid).cpu().numpy()
    want = occ_sums_ref(grid, OCC)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


# ---- the corridors ----------------------------------------------------------------------------------------------------
def corridors(rt, grid, frame, pts, reach, rect=True, status=True):
    """one call into outputs filled with a sentinel: (planes, rect or None, status or None) as numpy"""
    torch, lib = rt["torch"], rt["lib"]
    B, N = pts.shape[:2]
    S = device_sums(rt, grid)
    planes = torch.full((B, N, NOBST, 4), FILL_F, dtype=torch.float64, device=DEV)
    r = torch.full((B, N, 4), FILL, dtype=torch.int32, device=DEV) if rect else None
    s = torch.full((B, N), FILL, dtype=torch.int32, device=DEV) if status else None
    lib.grid_corridor_device(S, _t(torch, pts), planes, *frame, reach=reach, slot0=SLOT0, rect=r, status=s)
    return planes.cpu().numpy(), None if r is None else r.cpu().numpy(), None if s is None else s.cpu().numpy()


def reference(key, grid, frame, pts, reach):
    """(planes, rect, status) of the restatement, computed once per key and left unchanged"""
    if key not in REFS:
        planes = np.full(pts.shape[:2] + (NOBST, 4), FILL_F)
        REFS[key] = (planes,) + corridor_ref(occ_sums_ref(grid, OCC), *frame, pts, reach, planes, SLOT0)
    return REFS[key]


def same(got, want):
    planes, rect, status = got
    assert np.array_equal(status, want[2]), np.argwhere(status != want[2])[:5]
    assert np.array_equal(rect, want[1]), np.argwhere(rect != want[1])[:5]
    a, b = canonical_bits(planes), canonical_bits(want[0])
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]
    assert (planes[:, :, :SLOT0] == FILL_F).all() and (planes[:, :, SLOT0 + 4:] == FILL_F).all()     # slots 0, 1 and 6


SMALL = dict(small_maps(), hand=hand_map())


@pytest.mark.parametrize("name", list(SMALL))
def test_corridors_from_every_free_cell_of_the_small_maps(rt, name):
    grid = SMALL[name]
    pts = free_centres(grid, FRAME)
    for reach in (1, 2, 8):
        want = reference(("small", name, reach), grid, FRAME, pts, reach)
        assert (want[2] == 1).all()
        same(corridors(rt, grid, FRAME, pts, reach), want)
    if name == "hand":
        cells = np.rint((pts[:, 0, :2] - FRAME[:2]) / FRAME[2]).astype(int)
        at = {(2, 2): (0, 4, 2, 3), (0, 0): (0, 2, 0, 3), (4, 6): (2, 4, 2, 6)}
        rect = corridors(rt, grid, FRAME, pts, 8)[1]
        for (r, c), box in at.items():
            assert tuple(rect[np.flatnonzero((cells[:, 1] == r) & (cells[:, 0] == c))[0], 0]) == box


BIG = {"store": (lambda: store_raw(0), store_frame), "sparse": (sparse_map, lambda: EXACT)}
SIZES = [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (3, 20), (13, 20)]


@pytest.mark.parametrize("B,N", SIZES)
@pytest.mark.parametrize("name", list(BIG))
def test_corridors_on_seeded_points(rt, name, B, N):
    grid, frame = BIG[name][0](), BIG[name][1]()
    pts = random_points(grid, frame, B, N, seed=100 + B)
    for reach in REACHES:
        want = reference((name, B, N, reach), grid, frame, pts, reach)
        same(corridors(rt, grid, frame, pts, reach), want)
    if B * N >= 255:                                          # (the case holds what it is there for)
        st = reference((name, B, N, 8), grid, frame, pts, 8)[2]
        assert (st == 1).sum() > 100 and (st == -1).sum() > 10 and (st == 0).sum() > 3
        big = reference((name, B, N, 256), grid, frame, pts, 256)[1]
        small = reference((name, B, N, 8), grid, frame, pts, 8)[1]
        assert (big[..., 1] - big[..., 0] > small[..., 1] - small[..., 0]).any()


def test_rect_and_status_may_be_null(rt):
    grid, frame = store_raw(0), store_frame()
    pts = random_points(grid, frame, 65, 1, seed=165)
    want = reference(("store", 65, 1, 8), grid, frame, pts, 8)
    for rect, status in ((False, False), (True, False), (False, True)):
        planes, r, s = corridors(rt, grid, frame, pts, 8, rect=rect, status=status)
        assert np.array_equal(canonical_bits(planes), canonical_bits(want[0]))
        assert (r is None or np.array_equal(r, want[1])) and (s is None or np.array_equal(s, want[2]))


# ---- the class --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heading", (0, 1))
def test_map_corridors_step_is_the_two_entries_and_set_grid_a_fresh_object(rt, heading):
    torch, lib, MapCorridors = rt["torch"], rt["lib"], rt["MapCorridors"]
    B, N, nvar, nobst, slot0, reach = 37, 20, 9, 6, 1, 8
    frame = store_frame()
    grid, other = _t(torch, store_raw(0)), _t(torch, store_raw(1))
    rng = np.random.default_rng(35)
    z = rng.uniform(-9.5, 9.5, (B, N, nvar))
    xinit = _t(torch, np.concatenate([rng.uniform(-9.0, 9.0, (B, 2)), rng.uniform(-3.0, 3.0, (B, 5))], 1))[:, :6]   # stride 7
    ef = np.ones(B, dtype=np.int32)
    ef[::5] = -6
    z_d, ef_d = _t(torch, z), _t(torch, ef, torch.int32)
    kw = dict(heading=heading, offset=(0.4, 0.0) if heading else (0.0, 0.0), height=0.05)
    shared = torch.full((B, N, nobst, 4), FILL_F, dtype=torch.float64, device=DEV)
    mc = MapCorridors(B, N, grid, *frame, occupancy_threshold=OCC, reach=reach, slot0=slot0, planes=shared, **kw)
    assert mc.planes is shared and mc.nobst == nobst

    def by_hand(g, z_prev, flags):
        S = device_sums(rt, g.cpu().numpy())
        pts = torch.zeros((B, N, 3), dtype=torch.float64, device=DEV)
        lib.fleet_points_device(xinit, pts, z_prev, flags, heading, kw["offset"], kw["height"])
        planes = torch.full((B, N, nobst, 4), FILL_F, dtype=torch.float64, device=DEV)
        rect, st = torch.zeros((B, N, 4), dtype=torch.int32, device=DEV), torch.zeros((B, N), dtype=torch.int32, device=DEV)
        lib.grid_corridor_device(S, pts, planes, *frame, reach=reach, slot0=slot0, rect=rect, status=st)
        return S, pts, planes, rect, st

    def equal(m, want):
        got = (m.sums, m.points, m.planes, m.rects, m.status)
        for a, b in zip(got, want):
            assert rt["torch"].equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                     b.view(torch.int64) if b.dtype == torch.float64 else b)

    assert mc.step(xinit) is shared                           # the first step: from the pose
    equal(mc, by_hand(grid, None, None))
    mc.step(xinit, z_d, ef_d)                                 # from the shifted plan, the failed solves from the pose
    want = by_hand(grid, z_d, ef_d)
    equal(mc, want)
    assert (want[4] == 1).sum() > 100 and (shared[:, :, 0] == FILL_F).all() and (shared[:, :, 5] == FILL_F).all()
    mc.set_grid(other)
    mc.step(xinit, z_d, ef_d)
    fresh = MapCorridors(B, N, other, *frame, occupancy_threshold=OCC, reach=reach, slot0=slot0, nobst=nobst, **kw)
    assert fresh.planes.shape == shared.shape and fresh.planes is not shared
    fresh.planes.fill_(FILL_F)
    fresh.step(xinit, z_d, ef_d)
    equal(mc, (fresh.sums, fresh.points, fresh.planes, fresh.rects, fresh.status))
    assert not torch.equal(mc.rects, want[3])                 # (the other map is another map)


# ---- the closed loop --------------------------------------------------------------------------------------------------
def test_store_example_keeps_r_body_from_the_shelves_where_its_solves_converge():
    """examples/fleet_store_corridor.py, 32 robots, 150 steps, seed 0, with corridors: over the robot-steps whose solve
    converged (flag 1 or 2) the robot's centre stays r_body - ADMITTED_VIOLATION from every raw-occupied cell, and at
    most 2 % of the robot-steps are left out as not converged.  The example's defaults, its waypoint threshold of 0.6 m
    among them (the point robot's look-ahead of fleet_crossing.py, set before it was measured).  Measured on the MI355X:
    28 failed solves of 4800 (0.58 %), every one with a seed closer than r_body to a face of its own rectangle, no seed
    without a corridor, least clearance 0.425 m.  At the reference's threshold of 1.3 m the same loop misses both
    bounds (15 % not converged, a robot inside a shelf), and the full loop of 256 robots misses the clearance at 0.6 m
    too, after failed solves: DESIGN.md 29 has the table and the cause."""
    ex = load_example("fleet_store_corridor")
    r = ex.run(B=32, steps=150, seed=0)
    print(r)
    assert r["routes"] == 32 and r["corridor"] and r["neighbours"] == 0
    assert r["not_converged_share"] <= 0.02, r
    assert r["min_clearance_converged_m"] >= ex.R_BODY - ADMITTED_VIOLATION, r
    assert 0.0 <= r["seeds_without_corridor_share"] < 1.0, r
