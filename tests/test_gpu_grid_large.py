"""Cost-to-go fields on large maps on the device (rmpc_grid_fields_large_device, rmpc_grid_fields_seeded_large_device;
DESIGN.md 22): bit for bit the fields of the entries of rmpc.h on the maps those accept, the heap Dijkstras of
tests/global_planner_reference.py and tests/exploration_reference.py beyond, the visit counts of the numpy restatement
of the work-list rule (tests/grid_large_reference.py), and the planner's entries that now take such maps.  Every launch
writes into outputs poisoned with NaN / 0xA5."""
import numpy as np
import pytest

from exploration_reference import field_seeded_ref
from global_planner_reference import S2, descend_ref, field_ref, path_cost
from gpu_support import DEV, _t
from grid_large_reference import serpentine, tiled_field_ref

pytestmark = pytest.mark.gpu
POISON = int(np.frombuffer(b"\xa5" * 4, np.int32)[0])
INF = float("inf")


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib, T=_lib.GRID_TILE)


def _launch(rt, entry, data, src, movement, count=True, stream=None):
    """one launch of a fields entry into poisoned outputs -> (fields, status, sweeps or visits or None)"""
    torch, lib = rt["torch"], rt["lib"]
    seeded = "seeded" in entry
    src_t = _t(torch, src) if seeded else _t(torch, src, torch.int32)
    G = int(src_t.shape[0])
    H, W = data.shape
    f = torch.full((G, H, W), float("nan"), dtype=torch.float64, device=DEV)
    st = torch.full((G,), POISON, dtype=torch.int32, device=DEV)
    n = torch.full((G,), POISON, dtype=torch.int32, device=DEV) if count else None
    kw = {("visits" if "large" in entry else "sweeps"): n}
    grid = _t(torch, data)
    torch.cuda.synchronize()                               # (the launch may go to a side stream)
    getattr(lib, entry)(grid, src_t, f, st, movement, 0.8, 3.0, stream=stream, **kw)
    torch.cuda.synchronize()
    return f.cpu().numpy(), st.cpu().numpy(), None if n is None else n.cpu().numpy()


def _large(rt, data, goals, movement, **kw):
    return _launch(rt, "grid_fields_large_device", data, np.asarray(goals, np.int32), movement, **kw)


def _graded(H, W, seed, wall=0.2):
    rng = np.random.default_rng(seed)
    d = np.where(rng.uniform(size=(H, W)) < wall, 1.0, rng.uniform(0.0, 0.7, size=(H, W)))
    d[0, 0] = 0.1
    return d


def _store41():
    from robot_mpcs_amd.global_planner import shelf_map
    return shelf_map(41, 41)


# ---- maps both entries accept: bit for bit the old entries' fields and status ------------------------------------------
SMALL = {"1x1": lambda: np.zeros((1, 1)), "7x5": lambda: _graded(7, 5, 1, wall=0.1), "store41": _store41,
         "graded128": lambda: _graded(128, 128, 2)}


@pytest.mark.parametrize("movement", [8, 4])
@pytest.mark.parametrize("name", list(SMALL))
def test_goal_fields_equal_the_lds_entry(rt, name, movement):
    data = SMALL[name]()
    H, W = data.shape
    free, occ = np.flatnonzero(data.ravel() < 0.8), np.flatnonzero(data.ravel() >= 0.8)
    # G = 3: a free goal, then an occupied one (or the last free one), a goal at -1; G = 1; goals H W and the last cell
    three = [int(free[0]), int(occ[0]) if len(occ) else int(free[-1]), -1]
    for goals in (three, [int(free[len(free) // 2])], [H * W, int(free[-1]), int(free[0])]):
        want_f, want_st, _ = _launch(rt, "grid_fields_device", data, np.asarray(goals, np.int32), movement)
        f, st, visits = _large(rt, data, goals, movement)
        assert np.array_equal(st, want_st), (goals, st, want_st)
        assert np.array_equal(f, want_f), goals
        assert np.array_equal(visits > 0, st == 0) and np.all(visits[st != 0] == 0)
    assert list(_large(rt, data, three, movement)[1])[2] == rt["lib"].GRID_OUTSIDE
    if len(occ):
        assert _large(rt, data, three, movement)[1][1] == rt["lib"].GRID_GOAL_OCCUPIED


@pytest.mark.parametrize("movement", [8, 4])
@pytest.mark.parametrize("name", list(SMALL))
def test_seeded_fields_equal_the_lds_entry(rt, name, movement):
    lib = rt["lib"]
    data = SMALL[name]()
    H, W = data.shape
    rng = np.random.default_rng(H * W + movement)
    free = np.flatnonzero(data.ravel() < 0.8)
    n = min(len(free), 5)
    good = np.full((H, W), INF)
    good.ravel()[rng.choice(free, n, replace=False)] = rng.uniform(0.0, 9.0, n)
    good.ravel()[np.flatnonzero(data.ravel() >= 0.8)[:2]] = 1.0          # seeds on occupied cells are ignored
    neg, nan = good.copy(), good.copy()
    neg.ravel()[free[-1]], nan.ravel()[free[0]] = -1.0, float("nan")
    for seeds in (np.stack([neg, good, nan]), good[None]):
        want_f, want_st, _ = _launch(rt, "grid_fields_seeded_device", data, seeds, movement)
        f, st, visits = _launch(rt, "grid_fields_seeded_large_device", data, seeds, movement)
        assert np.array_equal(st, want_st) and np.array_equal(f, want_f)
        assert np.array_equal(visits > 0, st == 0) and np.all(visits[st != 0] == 0)
    assert list(st) == [0] and list(_launch(rt, "grid_fields_seeded_large_device", data, np.stack([neg, good, nan]),
                                            movement)[1]) == [lib.GRID_BAD_SEED, 0, lib.GRID_BAD_SEED]
    ref, _ = field_seeded_ref(data, good, movement)
    assert np.array_equal(f[0], ref)


def test_a_negative_free_cell_is_a_bad_map_in_both_entries(rt):
    lib = rt["lib"]
    data = _graded(41, 37, 3)
    free = np.flatnonzero(data.ravel() < 0.8)
    data.ravel()[free[7]] = -0.25
    goals = [int(free[0]), int(free[-1])]
    for entry, src in (("grid_fields", np.asarray(goals, np.int32)),
                       ("grid_fields_seeded", np.where(np.arange(41 * 37).reshape(41, 37) == goals[0], 0.0, INF)[None])):
        want_f, want_st, _ = _launch(rt, entry + "_device", data, src, 8)
        f, st, visits = _launch(rt, entry + "_large_device", data, src, 8)
        assert np.all(st == lib.GRID_BAD_MAP) and np.array_equal(st, want_st)
        assert np.all(np.isinf(f)) and np.array_equal(f, want_f) and np.all(visits == 0)


# ---- beyond the old cap: the Dijkstra exactly ---------------------------------------------------------------------------
def test_the_first_size_the_lds_entry_refuses(rt):
    torch, lib = rt["torch"], rt["lib"]
    data = _graded(129, 128, 4)
    free = np.flatnonzero(data.ravel() < 0.8)
    goals = [int(free[0]), int(free[len(free) // 2])]
    for movement in (8, 4):
        f, st, visits = _large(rt, data, goals, movement)
        assert list(st) == [0, 0] and np.all(visits > 0)
        for k, g in enumerate(goals):
            assert np.array_equal(f[k], field_ref(data, g, movement))
    # the old entry on this map is refused as before
    with pytest.raises(lib.RmpcError, match="129x128 map exceeds RMPC_GRID_MAX_CELLS = 16384"):
        lib.grid_fields_device(_t(torch, data), _t(torch, goals, torch.int32),
                               torch.empty((2, 129, 128), dtype=torch.float64, device=DEV),
                               torch.empty(2, dtype=torch.int32, device=DEV))
    with pytest.raises(lib.RmpcError, match="RMPC_GRID_MAX_CELLS"):
        lib.grid_fields_seeded_device(_t(torch, data), _t(torch, np.zeros((1, 129, 128))),
                                      torch.empty((1, 129, 128), dtype=torch.float64, device=DEV),
                                      torch.empty(1, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("shape", ["T,T", "T+1,T-1", "2*T+1,T+3", "1,3*T+2", "3*T+2,1"])
def test_tile_edges(rt, shape):
    T = rt["T"]
    H, W = eval(shape, {"T": T})
    data = _graded(H, W, H + W)
    free = np.flatnonzero(data.ravel() < 0.8)
    goals = [int(free[0]), int(free[-1]), int(free[len(free) // 2])]
    for movement in (8, 4):
        f, st, visits = _large(rt, data, goals, movement)
        assert list(st) == [0, 0, 0]
        for k, g in enumerate(goals):
            assert np.array_equal(f[k], field_ref(data, g, movement)), (shape, movement, g)
            assert visits[k] == tiled_field_ref(data, g, T, movement, "zigzag")[1]


def test_a_goal_walled_in_on_its_tile_but_open_to_the_next(rt):
    """Nothing of the goal's own tile is ever lowered: the source itself has to wake the tile beside it."""
    T = rt["T"]
    data = np.zeros((T + 9, T + 9))
    data[T - 1, T - 2] = data[T - 2, T - 1] = data[T - 2, T - 2] = 1.0
    goal = (T - 1) * (T + 9) + T - 1
    for movement in (8, 4):
        f, st, visits = _large(rt, data, [goal], movement)
        ref = field_ref(data, goal, movement)
        assert st[0] == 0 and np.isfinite(ref[0, 0]) and np.array_equal(f[0], ref)
        assert visits[0] == tiled_field_ref(data, goal, T, movement, "zigzag")[1]


@pytest.mark.parametrize("movement", [8, 4])
def test_serpentine_fields_and_visits(rt, movement):
    T = rt["T"]
    data = serpentine(2 * T + 3, 2 * T + 5)
    f, st, visits = _large(rt, data, [0], movement)
    ref, want = tiled_field_ref(data, 0, T, movement, "zigzag")
    assert st[0] == 0 and np.array_equal(f[0], field_ref(data, 0, movement)) and np.array_equal(f[0], ref)
    assert visits[0] == want


def test_graded_150x131_goal_and_seeded_with_potentials(rt):
    T = rt["T"]
    data = _graded(150, 131, 6)
    free = np.flatnonzero(data.ravel() < 0.8)
    goal = int(free[len(free) // 3])
    f, st, visits = _large(rt, data, [goal], 8)
    assert st[0] == 0 and np.array_equal(f[0], field_ref(data, goal, 8))
    assert visits[0] == tiled_field_ref(data, goal, T, 8, "zigzag")[1]
    rng = np.random.default_rng(60)
    seeds = np.full((150, 131), INF)
    seeds.ravel()[rng.choice(150 * 131, 60, replace=False)] = rng.uniform(0.0, 20.0, 60)
    ref, status = field_seeded_ref(data, seeds, 8)
    f, st, visits = _launch(rt, "grid_fields_seeded_large_device", data, seeds[None], 8)
    assert status == 0 and st[0] == 0 and np.array_equal(f[0], ref)
    assert visits[0] == tiled_field_ref(data, seeds, T, 8, "zigzag")[1]
    f2, st2, none = _launch(rt, "grid_fields_seeded_large_device", data, seeds[None], 8, count=False)    # d_visits = NULL
    assert none is None and st2[0] == 0 and np.array_equal(f2, f)
    f3, st3, _ = _large(rt, data, [goal], 8, count=False)
    assert st3[0] == 0 and np.array_equal(f3[0], field_ref(data, goal, 8))


def test_store_300x300_run_to_run_and_on_a_side_stream(rt):
    from robot_mpcs_amd.global_planner import shelf_map
    torch = rt["torch"]
    data = shelf_map(300, 300, seed=3)
    free = np.flatnonzero(data.ravel() < 0.8)
    goals = [int(free[0]), int(free[len(free) // 3]), int(free[2 * len(free) // 3]), int(free[-1])]
    f, st, visits = _large(rt, data, goals, 8)
    assert list(st) == [0] * 4 and np.all(visits > 0)
    for k, g in enumerate(goals):
        assert np.array_equal(f[k], field_ref(data, g, 8)), g
    f2, st2, visits2 = _large(rt, data, goals, 8)
    assert np.array_equal(f2, f) and np.array_equal(st2, st) and np.array_equal(visits2, visits)
    side = torch.cuda.Stream(device=DEV)
    f3, st3, visits3 = _large(rt, data, goals, 8, stream=side.cuda_stream)
    assert np.array_equal(f3, f) and np.array_equal(st3, st) and np.array_equal(visits3, visits)


# ---- the planner's entries on a map beyond the old cap ------------------------------------------------------------------
def test_plan_batch_on_a_200x180_store(rt):
    from robot_mpcs_amd.global_planner import plan_batch, shelf_map
    torch, lib = rt["torch"], rt["lib"]
    H, W = 200, 180
    data = shelf_map(H, W, seed=5)
    data[150:153, 100:103] = 1.0
    data[151, 101] = 0.0                                   # a free cell no route reaches
    rng = np.random.default_rng(8)
    free = np.setdiff1d(np.flatnonzero(data.ravel() < 0.8), [151 * W + 101])
    goal_set = rng.choice(free, 4, replace=False)
    B = 32
    starts = rng.choice(free, B, replace=False).astype(np.int32)
    goals = goal_set[rng.integers(0, 4, B)].astype(np.int32)
    starts[0] = 0                                          # the outer wall: an occupied start
    goals[1] = 151 * W + 101                               # unreachable
    starts[2] = H * W                                      # outside the map
    paths, lens, (fields, status, gi) = plan_batch(_t(torch, data), starts, goals, return_fields=True)
    torch.cuda.synchronize()
    paths, lens, fields, gi = paths.cpu().numpy(), lens.cpu().numpy(), fields.cpu().numpy(), gi.cpu().numpy()
    assert np.all(status.cpu().numpy() == 0)
    assert list(lens[:3]) == [lib.GRID_START_OCCUPIED, 0, lib.GRID_OUTSIDE]
    refs = {int(g): field_ref(data, int(g)) for g in np.unique(goals)}
    for b in range(B):
        assert np.array_equal(fields[gi[b]], refs[int(goals[b])])
        if b >= 3:
            want = descend_ref(data, refs[int(goals[b])], int(starts[b]), int(goals[b]))
            assert lens[b] == len(want) and list(paths[b, :lens[b]]) == want


def _cost_from_the_goal(data, cells, f=3.0):
    """The route's cost delta + f data over the entered cells, summed as the field sums it: from the goal backwards,
    D(u) = delta + (f data[v] + D(v)).  (path_cost adds the same terms from the start, which rounds otherwise: on this
    route 260.8822509939088 against the field's 260.88225099390877.)"""
    W = data.shape[1]
    cost = 0.0
    for u, v in zip(cells[-2::-1], cells[:0:-1]):
        (ur, uc), (vr, vc) = divmod(u, W), divmod(v, W)
        cost = (1.0 if abs(ur - vr) + abs(uc - vc) == 1 else S2) + (f * data[vr, vc] + cost)
    return cost


def test_a_star_on_a_150x150_map(rt):
    """a_star with the reference's signature on a map beyond the old cap: the route's cost is the field's value at the
    start, exactly when summed in the field's order and to rounding when summed by path_cost."""
    from robot_mpcs_amd.global_planner import OccupancyGridMap, a_star, shelf_map
    cell = 0.375
    data = shelf_map(150, 150, seed=9)
    gmap = OccupancyGridMap(data.copy(), cell)
    free = np.flatnonzero(data.ravel() < 0.8)
    s, g = int(free[3]), int(free[-5])
    path, path_idx = a_star(((s % 150) * cell, (s // 150) * cell), ((g % 150) * cell, (g // 150) * cell), gmap)
    assert isinstance(path, list) and path_idx[0] == (s % 150, s // 150) and path_idx[-1] == (g % 150, g // 150)
    cells = [y * 150 + x for x, y in path_idx]
    want = field_ref(data, g)[s // 150, s % 150]
    assert _cost_from_the_goal(data, cells) == want
    assert path_cost(data, cells) == pytest.approx(want, rel=1e-12)
