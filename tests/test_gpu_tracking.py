"""The moving-obstacle tracker on the device (rmpc_lidar_tracks_device, ObstacleTracker) against the
numpy restatement of tests/tracking_reference.py, bit for bit: every launch reads the arrays the restatement reads and
writes into poisoned outputs with poisoned memory behind them.  And the closed loop of
examples/fleet_moving_obstacles.py with the walkers' truth, with the tracker and blind."""
import json
import math
import os

import numpy as np
import pytest

from example_loader import load_example
from gpu_support import DEV
from tracking_cases import CASES
from tracking_reference import MAX_DET, params, tracks_ref

pytestmark = pytest.mark.gpu

POISON = -559038737          # 0xDEADBEEF as an int32
GUARD = 32                   # poisoned words behind every output
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "moving_loops.json")


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd import _lib
    return dict(torch=torch, lib=_lib)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Call:
    """The device side of calls with one set of shapes: inputs uploaded per call, the state carried on the device, the
    outputs poisoned before every launch, each buffer with GUARD poisoned words behind it."""

    def __init__(self, rt, B, R, T, n_out, p, static, with_det=True):
        torch = self.torch = rt["torch"]
        self.lib, self.B, self.p = rt["lib"], B, p
        self.buf = {}
        f = lambda name, shape: self._alloc(name, shape, torch.float64)
        i = lambda name, shape: self._alloc(name, shape, torch.int32)
        self.points, self.ranges, self.origin = f("points", (B, R, 3)), f("ranges", (B, R)), f("origin", (B, 3))
        self.static = f("static", (B, R)) if static else None
        self.track, self.age, self.miss = f("track", (B, T, 4)), i("age", (B, T)), i("miss", (B, T))
        self.obst, self.det, self.counts = f("obst", (B, n_out, 9)), f("det", (B, MAX_DET, 2)), i("counts", (B, 4))
        self.with_det = with_det

    def _alloc(self, name, shape, dtype):
        n = int(np.prod(shape))
        fill = math.nan if dtype == self.torch.float64 else POISON
        self.buf[name] = self.torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
        return self.buf[name][:n].view(*shape)

    def set_state(self, track, age, miss):
        t = self.torch
        self.track.copy_(t.from_numpy(track)); self.age.copy_(t.from_numpy(age)); self.miss.copy_(t.from_numpy(miss))

    def run(self, points, ranges, static, origin):
        t, p = self.torch, self.p
        self.points.copy_(t.from_numpy(points)); self.ranges.copy_(t.from_numpy(ranges)); self.origin.copy_(t.from_numpy(origin))
        if self.static is not None:
            self.static.copy_(t.from_numpy(static))
        self.obst.fill_(math.nan); self.det.fill_(math.nan); self.counts.fill_(POISON)
        a = self.lib.tracks_args(self.points, self.ranges, self.origin, self.track, self.age, self.miss, self.obst,
                                 p["radius"], p["dt"], static_ranges=self.static, closed=bool(p["closed"]),
                                 max_range=p["range"], margin=p["margin"], gap=p["gap"], min_rays=p["min_rays"],
                                 max_extent=p["max_extent"], gate=p["gate"], alpha=p["alpha"], beta=p["beta"],
                                 v_max=p["v_max"], confirm=p["confirm"], max_miss=p["max_miss"],
                                 park=(p["park_x"], p["park_y"]), det=self.det if self.with_det else None,
                                 counts=self.counts if self.with_det else None)
        self.lib.lidar_tracks_device(a, self.B)
        t.cuda.synchronize()
        for name, b in self.buf.items():                        # nothing behind any buffer was written
            g = b[-GUARD:].cpu().numpy()
            assert np.all(np.isnan(g)) if g.dtype == np.float64 else np.all(g == POISON), name
        host = lambda x: x.cpu().numpy()
        return host(self.obst), host(self.det), host(self.counts), host(self.track), host(self.age), host(self.miss)


def check(got, want, with_det=True):
    names = ("obst_dyn", "det", "counts", "track", "age", "miss")
    for n, g, w in zip(names, got, want):
        if not with_det and n in ("det", "counts"):
            continue
        assert same(g, w), (n, np.argwhere(bits(g) != bits(w))[:5])


def ref(c_points, c_ranges, c_static, c_origin, p, track, age, miss, n_out):
    ob, det, cnt = tracks_ref(c_points, c_ranges, c_static, c_origin, p, track, age, miss, n_out)
    return ob, det, cnt, track, age, miss


# ---- the constructed cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_constructed_case_is_the_restatement(rt, name):
    c = CASES[name]()
    T = c["track"].shape[1]
    dev = Call(rt, 1, c["points"].shape[1], T, c["n_out"], c["p"], c["static"] is not None)
    dev.set_state(c["track"], c["age"], c["miss"])
    got = dev.run(c["points"], c["ranges"], c["static"], c["origin"])
    want = ref(c["points"], c["ranges"], c["static"], c["origin"], c["p"], c["track"].copy(), c["age"].copy(),
               c["miss"].copy(), c["n_out"])
    check(got, want)
    assert want[2][0, 0] > 0 or name in ("static_exact", "deletion")


# ---- random clouds -------------------------------------------------------------------------------------------------------
def cloud(rng, B, R, T, static, dense):
    """Random clouds built as arrays: runs of 1 .. 7 rays on circles of radius 0.3 around random centres, between them
    rays that are not moving; the state holds tracks near some of the centres.  Returns (points, ranges, static, origin,
    track, age, miss)."""
    ang = 2.0 * math.pi * np.arange(R) / R
    pts = np.zeros((B, R, 3))
    rngs = np.zeros((B, R))
    st = np.full((B, R), 9.0) if static else None
    origin = np.concatenate([rng.uniform(-0.5, 0.5, (B, 2)), np.full((B, 1), 0.02)], axis=1)
    track, age, miss = np.zeros((B, T, 4)), np.zeros((B, T), np.int32), np.zeros((B, T), np.int32)
    for b in range(B):
        pts[b] = np.stack([origin[b, 0] + 8.0 * np.cos(ang), origin[b, 1] + 8.0 * np.sin(ang), np.full(R, 0.02)], axis=1)
        rngs[b] = 9.0 if static else 10.0
        centres = []
        i = int(rng.integers(0, 3))
        while i < R:
            n = int(rng.integers(1, 8))
            c = rng.uniform(-6, 6, 2)
            a0 = math.atan2(origin[b, 1] - c[1], origin[b, 0] - c[0])
            for t in range(min(n, R - i)):
                a = a0 + rng.uniform(-0.8, 0.8)
                pts[b, i + t, :2] = (c[0] + 0.3 * math.cos(a), c[1] + 0.3 * math.sin(a))
                rngs[b, i + t] = math.hypot(pts[b, i + t, 0] - origin[b, 0], pts[b, i + t, 1] - origin[b, 1])
            centres.append(c)
            i += n + (int(rng.integers(0, 3)) if dense else int(rng.integers(R // 8 + 1, R // 3 + 2)))
        if static:
            st[b, ::5] = rngs[b, ::5] + rng.choice([0.0, 0.04, 0.05, 0.06, 1.0], size=len(rngs[b, ::5]))
        for j in range(T):
            if rng.uniform() < 0.7:
                c = centres[int(rng.integers(len(centres)))] if rng.uniform() < 0.8 else rng.uniform(-6, 6, 2)
                track[b, j] = (c[0] + rng.normal(0, 0.2), c[1] + rng.normal(0, 0.2), rng.uniform(-1, 1), rng.uniform(-1, 1))
                age[b, j], miss[b, j] = rng.integers(1, 6), rng.integers(0, 7)
            else:
                track[b, j] = rng.uniform(-1, 1, 4)              # a free slot's stale words stay as they are
    return pts, rngs, st, origin, track, age, miss


CLOUDS = [
    # B, R, T, n_out, closed, static, dense
    (1, 5, 1, 1, 1, False, True), (3, 5, 8, 5, 0, True, False),
    (3, 64, 16, 20, 1, False, True), (37, 64, 8, 5, 0, False, False), (1, 64, 1, 1, 1, True, True),
    (3, 257, 8, 1, 1, True, True), (37, 257, 16, 5, 0, False, True), (1, 257, 16, 20, 1, False, False),
    (1, 2048, 16, 20, 1, False, True), (3, 2048, 8, 5, 0, True, True), (37, 2048, 1, 1, 1, True, False),
]


@pytest.mark.parametrize("B,R,T,n_out,closed,static,dense", CLOUDS)
def test_random_clouds_are_the_restatement(rt, B, R, T, n_out, closed, static, dense):
    rng = np.random.default_rng(1000 * R + 10 * B + T)
    p = params(closed=closed, gap=0.5, min_rays=2, max_extent=0.62, gate=0.8, confirm=2, max_miss=5, v_max=0.9,
               range=10.0, margin=0.05, park_x=-40.0, park_y=55.0)
    pts, rngs, st, origin, track, age, miss = cloud(rng, B, R, T, static, dense)
    with_det = (B + R) % 2 == 0                                   # det and counts may be NULL
    dev = Call(rt, B, R, T, n_out, p, static, with_det)
    dev.set_state(track, age, miss)
    got = dev.run(pts, rngs, st, origin)
    want = ref(pts, rngs, st, origin, p, track.copy(), age.copy(), miss.copy(), n_out)
    check(got, want, with_det)
    if dense and R >= 257:
        assert want[2][:, 0].max() > MAX_DET                     # more segments than detections
    # only robot b's inputs change: the rows of the others do not
    if B > 1:
        b = B // 2
        pts2, rngs2 = pts.copy(), rngs.copy()
        pts2[b, :, :2] = pts[b, ::-1, :2]
        rngs2[b] = rngs[b, ::-1]
        dev.set_state(track, age, miss)
        got2 = dev.run(pts2, rngs2, st, origin)
        others = np.arange(B) != b
        for g, g2 in zip(got, got2):
            assert same(g[others], g2[others])


# ---- a scripted sequence that carries the state ------------------------------------------------------------------------------
def test_forty_calls_carry_the_state(rt):
    rng = np.random.default_rng(7)
    B, R, T, n_out, steps = 3, 64, 8, 5, 40
    p = params(closed=1, gap=0.45, min_rays=2, max_extent=0.7, gate=1.0, confirm=3, max_miss=3, v_max=1.5)
    dev = Call(rt, B, R, T, n_out, p, False)
    track, age, miss = np.zeros((B, T, 4)), np.zeros((B, T), np.int32), np.zeros((B, T), np.int32)
    dev.set_state(track, age, miss)
    P = 6
    w = np.concatenate([rng.uniform(-5, 5, (B, P, 2)), rng.uniform(-1.0, 1.0, (B, P, 2))], axis=2)
    ang = 2.0 * math.pi * np.arange(R) / R
    seen = set()
    for k in range(steps):
        pts = np.stack([8.0 * np.cos(ang), 8.0 * np.sin(ang), np.full(R, 0.02)], axis=1)[None].repeat(B, axis=0)
        rngs = np.full((B, R), 10.0)
        origin = np.zeros((B, 3))
        for b in range(B):
            for q in range(P):
                if (k + 3 * q + b) % 11 < 3:                     # a walker goes unseen for three calls in eleven
                    continue
                i0 = (10 * q + k // 2) % R                       # its rays drift around the sweep, over the seam too
                a0 = math.atan2(-w[b, q, 1], -w[b, q, 0])
                for t in range(3):
                    a = a0 + 0.5 * (t - 1)
                    i = (i0 + t) % R
                    pts[b, i, :2] = (w[b, q, 0] + 0.3 * math.cos(a), w[b, q, 1] + 0.3 * math.sin(a))
                    rngs[b, i] = math.hypot(pts[b, i, 0], pts[b, i, 1])
        got = dev.run(pts, rngs, None, origin)
        want = ref(pts, rngs, None, origin, p, track, age, miss, n_out)      # (in place: the host's state)
        check(got, want)
        seen |= {int(v) for v in want[2][:, 3]}
        w[:, :, :2] += 0.1 * w[:, :, 2:]
    assert max(seen) >= 3 and int(miss.max()) >= 1 and int(age.max()) >= 8       # tracks were confirmed, coasted, kept


# ---- the chain: scan on the device, tracker on the device, against the restatement on the device's scan -----------------------
def test_the_chain_from_the_scan_is_the_restatement(rt):
    torch = rt["torch"]
    from robot_mpcs_amd.utils.tracking import ObstacleTracker
    rng = np.random.default_rng(3)
    B, R, T, n_out, steps, P = 5, 256, 8, 5, 20, 7
    boxes = np.array([(0.0, 4.0, 3.0, 0.5), (-4.0, -1.0, 0.5, 4.0), (3.0, -3.0, 1.0, 1.0)])
    pose = np.zeros((B, 8))
    pose[:, :3] = np.stack([rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(-math.pi, math.pi, B)], axis=1)
    w = np.concatenate([rng.uniform(-6, 6, (P, 2)), rng.uniform(-0.5, 0.5, (P, 2))], axis=1)
    w[0, :2], w[1, :2] = (0.0, 5.0), (-5.0, -1.0)               # two walkers start behind a box
    trk = ObstacleTracker(B, n_out, boxes=boxes, rays=R, n_tracks=T, radius=0.3, dt=0.1, confirm=2, device=DEV)
    p = params(closed=1, range=10.0, margin=0.05, gap=trk.gap, radius=0.3, max_extent=trk.max_extent, min_rays=2,
               gate=1.0, dt=0.1, alpha=0.4, beta=0.1, v_max=0.0, confirm=2, max_miss=5)
    track, age, miss = np.zeros((B, T, 4)), np.zeros((B, T), np.int32), np.zeros((B, T), np.int32)
    d_pose = torch.from_numpy(pose).to(DEV)
    occluded = 0
    for k in range(steps):
        circles = np.concatenate([w[:, :2], np.full((P, 1), 0.3)], axis=1)
        trk.obst_dyn.fill_(math.nan); trk.det.fill_(math.nan); trk.counts.fill_(POISON)
        ob = trk.step(d_pose, torch.from_numpy(circles).to(DEV))
        torch.cuda.synchronize()
        host = lambda x: x.cpu().numpy()
        pts, rngs, st, origin = host(trk.points), host(trk.ranges), host(trk.static_ranges), host(trk.origin)[:, 0]
        want = ref(pts, rngs, st, origin, p, track, age, miss, n_out)
        check((host(ob), host(trk.det), host(trk.counts), host(trk.track), host(trk.age), host(trk.miss)), want)
        occluded += int((want[2][:, 1] < P).sum())
        w[:, :2] += 0.1 * w[:, 2:]
        pose[:, 2] += 0.05
        d_pose.copy_(torch.from_numpy(pose))
    assert occluded > 0 and int(age.max()) >= 10 and int((age >= 2).sum()) >= B


# ---- the closed loop -----------------------------------------------------------------------------------------------------------
# tests/golden/moving_loops.json holds the three runs below as measured on one MI355X (they repeat themselves there key
# for key).  The gates are fixed from those recorded values ("Closed loop"):
#   contact    tracked <= truth + 1.5 x (the recorded tracked - truth): the difference is the confirm-step latency of a
#              new track and the walkers hidden behind other walkers; half as much again may come on top;
#   blind      strictly above tracked, by at least half the recorded factor blind / tracked;
#   failed     tracked <= truth + max(1.5 x the recorded difference, 1e-3): the recorded shares are 0 and 0, one failed
#              solve in the 9600 is 1e-4, ten of them are allowed.
LOOP = dict(B=64, P=24, steps=150, seed=0)


def test_the_closed_loop_tracked_against_truth_and_blind(rt):
    with open(GOLDEN) as fh:
        rec = json.load(fh)
    ex = load_example("fleet_moving_obstacles")
    r = {mode: json.loads(json.dumps(ex.run(obstacles=mode, **LOOP))) for mode in ("truth", "tracked", "blind")}
    for mode in r:
        print(mode, r[mode])
        assert r[mode]["fused"] and {k for k in r[mode] if not k.startswith("ms_")} == set(rec[mode])
    c = {m: r[m]["contact_share"] for m in r}
    c0 = {m: rec[m]["contact_share"] for m in rec}
    assert c0["blind"] > c0["tracked"] > c0["truth"]
    assert c["tracked"] <= c["truth"] + 1.5 * (c0["tracked"] - c0["truth"])
    assert c["blind"] > c["tracked"] and c["blind"] >= 0.5 * (c0["blind"] / c0["tracked"]) * c["tracked"]
    f, f0 = {m: r[m]["failed_share"] for m in r}, {m: rec[m]["failed_share"] for m in rec}
    assert f["tracked"] <= f["truth"] + max(1.5 * (f0["tracked"] - f0["truth"]), 1e-3)
    # the tracker did its work: most rows hold a track, and the rows are where walkers are
    assert r["tracked"]["rows_tracked_share"] >= 0.5 and r["tracked"]["pos_err_p50"] < 1e-3
