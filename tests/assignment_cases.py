"""Constructed inputs that the assignment tests share (tests/test_assignment_cpu.py, tests/test_gpu_assignment.py)."""
import math

INF = math.inf


def random_costs(rng, B, T, ties):
    """uniform doubles, or {0, 1, 2, 3} so that ties dominate; then NaN, negative, -0.0 and +inf entries mixed in, and
    last whole rows and columns of +inf"""
    cost = rng.integers(0, 4, (B, T)).astype(float) if ties else rng.uniform(0.0, 100.0, (B, T))
    if B * T >= 16:
        for v in (math.nan, -1.0, -INF, INF, -0.0):
            cost[rng.integers(0, B, max(1, B * T // 50)), rng.integers(0, T, max(1, B * T // 50))] = v
        cost[rng.integers(0, B, max(1, B // 16))] = INF
        cost[:, rng.integers(0, T, max(1, T // 16))] = INF
    return cost
