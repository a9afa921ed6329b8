"""The global planner's rules as restated in tests/global_planner_reference.py from the reference
(robotmpcs/global_planner/: a_star.py, gridmap.py, globalPlanner.py), checked on hand-computed grids;
tests/test_gpu_global_planner.py holds the device against them."""
import math

import numpy as np
import pytest

from global_planner_reference import S2, LocalGoalRef, astar_ref, descend_ref, field_ref, inflate_ref, path_cost


# ------------------------------------------------------------------------------------------------ hand-computed grids
def test_corridor():
    data = np.zeros((1, 5))
    assert np.array_equal(field_ref(data, 4)[0], [4.0, 3.0, 2.0, 1.0, 0.0])
    path, cost = astar_ref(data, (0, 0), (4, 0))
    assert path == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)] and cost == 4.0
    assert descend_ref(data, field_ref(data, 4), 0, 4) == [0, 1, 2, 3, 4]


def test_graded_corridor_prices_the_entered_cell():
    data = np.array([[0.0, 0.5, 0.1]])
    D = field_ref(data, 2)[0]
    assert D[2] == 0.0 and D[1] == 1.0 + (3.0 * 0.1 + 0.0) and D[0] == 1.0 + (3.0 * 0.5 + D[1])
    assert astar_ref(data, (0, 0), (2, 0))[1] == pytest.approx(D[0], rel=1e-15)


def test_diagonal_squeeze_between_two_occupied_cells():
    data = np.array([[0.0, 1.0], [1.0, 0.0]])
    D = field_ref(data, 3)
    assert D[0, 0] == S2 and np.isinf(D[0, 1]) and np.isinf(D[1, 0])
    assert astar_ref(data, (0, 0), (1, 1)) == ([(0, 0), (1, 1)], S2)
    assert np.isinf(field_ref(data, 3, movement=4)[0, 0])
    assert astar_ref(data, (0, 0), (1, 1), movement=4) == ([], math.inf)


def test_unreachable_pocket():
    data = np.zeros((5, 5))
    data[1:4, 1:4] = 1.0
    data[2, 2] = 0.0
    data[1, 1] = data[1, 3] = data[3, 1] = data[3, 3] = 1.0
    D = field_ref(data, 0)
    assert np.isinf(D[2, 2]) and np.isfinite(D[4, 4])
    assert astar_ref(data, (2, 2), (0, 0)) == ([], math.inf)
    with pytest.raises(Exception, match="Start node"):
        astar_ref(data, (1, 1), (0, 0))
    with pytest.raises(Exception, match="Goal node"):
        astar_ref(data, (0, 0), (1, 2))


def test_4n_against_8n():
    data = np.zeros((3, 3))
    assert field_ref(data, 8)[0, 0] == S2 + S2
    assert field_ref(data, 8, movement=4)[0, 0] == 4.0
    p8, c8 = astar_ref(data, (0, 0), (2, 2))
    p4, c4 = astar_ref(data, (0, 0), (2, 2), movement=4)
    assert c8 == 2 * S2 and len(p8) == 3 and c4 == 4.0 and len(p4) == 5
    # move order decides ties in the descent: right before up
    assert descend_ref(data, field_ref(data, 8, movement=4), 0, 8, movement=4) == [0, 1, 2, 5, 8]


def test_field_dijkstra_equals_astar_cost_on_random_binary_maps():
    rng = np.random.default_rng(0)
    for _ in range(5):
        data = (rng.uniform(size=(12, 15)) < 0.25).astype(float)
        free = np.flatnonzero(data.ravel() < 0.8)
        s, g = rng.choice(free, 2, replace=False)
        D = field_ref(data, g)
        path, cost = astar_ref(data, (s % 15, s // 15), (g % 15, g // 15))
        if np.isinf(D.ravel()[s]):
            assert path == []
            continue
        cells = descend_ref(data, D, s, g)
        assert cells[0] == s and cells[-1] == g
        assert path_cost(data, cells) == pytest.approx(D.ravel()[s], rel=1e-12) == pytest.approx(cost, rel=1e-12)


def test_inflation_restatement():
    data = np.zeros((7, 7))
    data[3, 3] = 1.0
    out, conv = inflate_ref(data, cell=0.4, size_robot=0.4)   # k = 1: 3x3 mean 1/9 < 0.29
    assert np.array_equal(out, np.zeros((7, 7))) and conv[2, 2] == 1.0 / 9
    data[3, 2] = data[3, 4] = 1.0                              # three in a row: 3/9 > 0.29 beside its middle only
    out, _ = inflate_ref(data, cell=0.4, size_robot=0.4)
    assert out[2, 3] == out[4, 3] == out[3, 3] == 1.0 and out[2, 2] == out[3, 2] == 0.0 and out.sum() == 3
    data[0, 0] = 0.5                                           # the border band keeps its raw value
    assert inflate_ref(data, cell=0.4, size_robot=0.4)[0][0, 0] == 1.0


def test_local_goal_restatement():
    path = [(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)]
    lg = LocalGoalRef(1.3)
    assert lg((0.0, 0.0), path) == (1.0, 0.0)       # within 1.3 of waypoint 0: one step on
    assert lg((0.0, 0.0), path) == (2.0, 0.0)       # within 1.3 of waypoint 1
    assert lg((-5.0, 0.0), path) == (2.0, 0.0)      # the last waypoint stays
    lg = LocalGoalRef(1.3)
    assert lg((5.0, 5.0), path) == (0.0, 0.0)       # too far: stays


# ------------------------------------------------------------------------------------------------ the mirror on the host
def test_package_imports_without_gpu():
    import robot_mpcs_amd.global_planner as gp
    assert {"OccupancyGridMap", "a_star", "GlobalPlanner", "RouteFollower", "plan_batch", "shelf_map"} <= set(gp.__all__)


def test_convert_meters_matches_reference_formulas():
    from robot_mpcs_amd.global_planner import GlobalPlanner
    low, high = np.array([-5.0, -5.0, 0.0]), np.array([10.0, 10.0, 1.0])
    gp = GlobalPlanner(dim_pixels=np.array([41, 41, 5]), limits_low=low, limits_high=high, BOOL_PLOTTING=False)
    dim = -low + high
    assert gp.cell_size == dim[0] / 41
    rng = np.random.default_rng(1)
    for _ in range(20):
        p = np.array([rng.uniform(-5, 10), rng.uniform(-5, 10), rng.uniform(0, 1)])
        u = p - low
        ref = [u[1], dim[1] - u[0], p[2]]
        got = gp.convert_meters(p)
        assert got == ref
        back = gp.convert_meters_reversed(tuple(got[:2]))
        assert np.array_equal(back, [dim[1] - got[1], got[0], 0.0] + low)
        assert np.allclose(back[:2], p[:2], rtol=0, atol=1e-12)
    assert np.array_equal(gp.convert_path([(1.0, 2.0)])[0], [dim[1] - 2.0, 1.0, 0.0] + low)


def test_gridmap_conventions():
    from robot_mpcs_amd.global_planner import OccupancyGridMap
    data = np.zeros((3, 4))
    data[2, 1] = 0.9
    m = OccupancyGridMap(data, 0.5)
    assert m.get_index_from_coordinates(0.25, 0.75) == (0, 2)      # round half to even
    assert m.get_index_from_coordinates(0.75, 1.25) == (2, 2)
    assert m.get_coordinates_from_index(3, 2) == (1.5, 1.0)
    assert m.is_occupied_idx((1, 2)) and not m.is_occupied_idx((2, 1))
    assert m.is_inside_idx((3, 2)) and not m.is_inside_idx((4, 0)) and not m.is_inside_idx((0, 3))
    with pytest.raises(Exception, match="outside"):
        m.is_occupied_idx((-1, 0))


def test_from_png_normalisation(tmp_path):
    from PIL import Image
    from robot_mpcs_amd.global_planner import OccupancyGridMap
    img = np.zeros((2, 3, 4), dtype=np.uint8)
    img[0, :, 0] = [0, 128, 255]          # top image row
    img[1, :, 0] = [64, 32, 16]
    img[..., 1] = 200
    Image.fromarray(img, "RGBA").save(tmp_path / "m.png")
    m = OccupancyGridMap.from_png(str(tmp_path / "m.png"), 0.1)
    assert np.array_equal(m.data, np.array([[64, 32, 16], [0, 128, 255]]) / 256.0)


def test_shelf_map_is_seeded_and_walled():
    from robot_mpcs_amd.global_planner import shelf_map
    a, b = shelf_map(41, 41, seed=3), shelf_map(41, 41, seed=3)
    assert np.array_equal(a, b) and not np.array_equal(a, shelf_map(41, 41, seed=4))
    assert a[0].all() and a[-1].all() and a[:, 0].all() and a[:, -1].all()
    assert 0.15 < a.mean() < 0.5
    # every free cell reaches every other (the gaps and end lanes connect the aisles)
    D = field_ref(a, int(np.flatnonzero(a.ravel() < 0.8)[0]))
    assert np.isfinite(D[a < 0.8]).all()


def test_pick_routes_is_seeded_and_every_line_crosses_a_shelf():
    from robot_mpcs_amd.global_planner import cell_xy, pick_routes, png_values, shelf_map
    raw = shelf_map(41, 41, seed=0)
    ok = inflate_ref(png_values(raw), 0.45, 0.45)[0] < 0.8
    starts, goals = pick_routes(raw > 0.5, ok, 256, np.random.default_rng(0), -9.0, -9.0, 0.45)
    again = pick_routes(raw > 0.5, ok, 256, np.random.default_rng(0), -9.0, -9.0, 0.45)
    assert np.array_equal(starts, again[0]) and np.array_equal(goals, again[1])
    assert starts.dtype == goals.dtype == np.int32 and starts.shape == goals.shape == (256,)
    # the fleet of seed 0 on the default store, as the store examples drew it before the function moved here
    assert starts[:5].tolist() == [1468, 360, 1317, 1086, 1465] and goals[:5].tolist() == [1191, 1439, 86, 110, 360]
    assert ok.ravel()[starts].all() and ok.ravel()[goals].all()
    a, b = cell_xy(starts, 41, -9.0, -9.0, 0.45), cell_xy(goals, 41, -9.0, -9.0, 0.45)
    assert np.array_equal(a[:, 0], -9.0 + (starts % 41) * 0.45) and np.array_equal(a[:, 1], -9.0 + (starts // 41) * 0.45)
    d = np.linalg.norm(a - b, axis=1)
    assert d.min() >= 10.0 and d.max() <= 20.0
    for p, q in zip(a, b):
        cc = np.rint((p + np.linspace(0.0, 1.0, 200)[:, None] * (q - p) + 9.0) / 0.45).astype(int)
        assert (raw[cc[:, 1], cc[:, 0]] > 0.5).any()


def test_png_values_reproduce_the_reference_png_round_trip(tmp_path):
    """plt.imsave -> OccupancyGridMap.from_png (what get_occupancy_map / get_enlarged_obstacles of the reference go
    through) yields png_values with the rows reversed; free cells 68/256, occupied 253/256."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from robot_mpcs_amd.global_planner import OccupancyGridMap, png_values
    rng = np.random.default_rng(2)
    for m in (np.clip(rng.uniform(-0.1, 0.4, (9, 13)), 0, 0.29), (rng.uniform(size=(11, 11)) < 0.3) * 0.29, np.zeros((4, 4))):
        plt.imsave(tmp_path / "m.png", m)
        assert np.array_equal(OccupancyGridMap.from_png(str(tmp_path / "m.png"), 0.1).data, png_values(m)[::-1])
    assert np.array_equal(png_values(np.array([[0.0, 0.29]])) * 256, [[68.0, 253.0]])


def test_reference_enlargement_is_a_full_dilation():
    """On the values of the PNG round trip, 3 x 3 mean > 0.29 blocks every cell next to an obstacle (one occupied cell in
    the window: (8 * 68 + 253) / (9 * 256) = 0.346) -- also beside the two-cell ends of a shelf."""
    from robot_mpcs_amd.global_planner import png_values, shelf_map
    raw = shelf_map(41, 41, seed=0)
    out, _ = inflate_ref(png_values(raw), 0.45, 0.45, 0.29)
    occ = raw > 0.5
    dil = occ.copy()
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            dil[1:-1, 1:-1] |= occ[1 + dr:40 + dr, 1 + dc:40 + dc]
    assert np.array_equal(out > 0.5, dil)


def test_grid_entries_refuse_negative_prices_on_the_host():
    """A negative (or non-finite) cost_factor would make the field sweeps diverge: refused before any launch."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    L = _lib.load_library()
    p = C.c_void_p(64)          # never dereferenced: the argument checks come first
    for f in (-3.0, float("nan"), float("inf")):
        assert L.rmpc_grid_fields_device(41, 41, p, 1, p, 8, 0.8, f, p, p, None, None) != 0
        assert b"cost_factor" in L.rmpc_last_error()
        assert L.rmpc_grid_paths_device(41, 41, p, 1, p, p, 1, p, p, 8, 0.8, f, 10, p, p, None) != 0
        assert b"cost_factor" in L.rmpc_last_error()
