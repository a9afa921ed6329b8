"""The random maps the timed planners' GPU modules draw (test_gpu_timed*.py), seeded per test."""
import numpy as np


def _map_and_starts(rng, H, W, B, density, sep2):
    """a random map, its free cells in random order and B starts among them pairwise sep2 apart, the first that fit"""
    g = (rng.uniform(size=(H, W)) < density).astype(float)
    free = rng.permutation(np.flatnonzero(g.ravel() < 0.5))
    starts = []
    for c in free:
        if len(starts) < B and all((c // W - q // W) ** 2 + (c % W - q % W) ** 2 >= sep2 for q in starts):
            starts.append(int(c))
    assert len(starts) == B
    return g, free, np.array(starts, np.int32)


def random_case(H, W, B, seed, density=0.15, sep2=4):
    """(grid, starts, goals, rng) for the timed routes: the goals are the last B free cells"""
    rng = np.random.default_rng(seed)
    g, free, starts = _map_and_starts(rng, H, W, B, density, sep2)
    return g, starts, free[-B:].astype(np.int32), rng


def random_tours_case(H, W, B, K, seed, density=0.15, sep2=4, Gf=None, lens=None):
    """a random map, B starts pairwise sep2 apart, Gf = 3 B free cells to stop at; a robot's stops are the K cells nearest
    to its start, the nearest first, so that short windows serve some and miss some; tours of mixed length"""
    rng = np.random.default_rng(seed)
    g, free, starts = _map_and_starts(rng, H, W, B, density, sep2)
    Gf = 3 * B if Gf is None else Gf
    cells = free[-Gf:].astype(np.int32)
    near = lambda s: np.argsort(np.maximum(abs(cells // W - s // W), abs(cells % W - s % W)), kind="stable")
    stops = np.stack([np.resize(near(s), K) for s in starts]).astype(np.int32)
    lens = (np.arange(B) % (K + 1) if lens is None else np.full(B, lens)).astype(np.int32)
    park = rng.integers(0, Gf, B).astype(np.int32)
    return dict(grid=g, starts=starts, cells=cells, stops=stops, lens=lens, park=park), rng


def walkers(rng, H, W, T, n):
    """n random walks of T + 1 cells, a tenth of them -1"""
    out = []
    for _ in range(n):
        r, c, path = int(rng.integers(0, H)), int(rng.integers(0, W)), []
        for t in range(T + 1):
            r, c = min(max(r + int(rng.integers(-1, 2)), 0), H - 1), min(max(c + int(rng.integers(-1, 2)), 0), W - 1)
            path.append(-1 if rng.uniform() < 0.1 else r * W + c)
        out.append(path)
    return np.array(out, np.int32)
