"""The three store examples in small, pinned to the run recorded before their shared parts moved into
robot_mpcs_amd/store.py (tests/golden/store_loops.json: the same five calls on the commit before, which reproduced
themselves there in every key kept).  The shapes are the smallest that pass through every piece that moved: step 0
without a previous plan, a re-plan at step 0 and later ones, the lidar on and off, the map's statistics, the known-map
loop and the early-exit bookkeeping of the frontier loop.  No margin on anything but the times: the device code is the
same, the solver is deterministic under its launch-order tests, the map's atomics are integer adds."""
import json
import os

import pytest

from example_loader import load_example

pytestmark = pytest.mark.gpu

RUNS = {
    "lidar": ("fleet_store_lidar", dict(B=8, steps=80)),
    "lidar_off": ("fleet_store_lidar", dict(B=8, steps=80, lidar=False)),
    "explore": ("fleet_store_explore", dict(B=8, steps=80, replan_every=10)),
    "explore_known": ("fleet_store_explore", dict(B=8, steps=20, known_map=True)),
    "frontier": ("fleet_store_frontier", dict(B=4, steps=40, replan_every=10)),
}
# the keys a recording may never lose
NEVER_DROPPED = {"robots", "steps", "routes", "replans", "control_steps", "failed_solves", "map_seen_cells",
                 "map_wrong_cells"}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "store_loops.json")) as _f:
    GOLDEN = json.load(_f)


def is_time(key):
    return key in ("ms_per_step", "plan_ms") or key.endswith("_ms")


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()


@pytest.mark.parametrize("name", list(RUNS))
def test_store_loop_reproduces_the_recorded_run(rt, name):
    example, kw = RUNS[name]
    r = json.loads(json.dumps(load_example(example).run(seed=0, K=4, rays=64, **kw)))
    print(r)
    want = GOLDEN[name]
    assert {k for k in r if not is_time(k)} == set(want) and NEVER_DROPPED & set(r) <= set(want)
    for k in want:
        assert r[k] == want[k], (k, r[k], want[k])
