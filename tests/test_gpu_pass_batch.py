"""Whole solves on the pass kernels (k_sweep / k_riccati[_lane] / k_compact[_wave] / k_step under the host loop of
solve_device) at the batch sizes where that loop changes regime: the grouped recursion blocks and their hand-over to the
one-wave blocks, the block list builder k_compact, the lane-per-instance recursion by default and the migration out of
it.  Cases and the sizes they sit at: pass_batch_cases.py.  Every test asserts the regime it names through
``Solver.last_solve_path()`` (rmpc_last_solve_path), so that it cannot pass outside it when a default or a threshold
moves; the bars against the oracle are check_plan's (gpu_support.py, stated in test_gpu_parity.py)."""
import numpy as np
import pytest

from gpu_support import check_plan
from pass_batch_cases import (B_COMPACT_BLOCK, B_LANE, CHUNK, GROUPED_CASES, NO_FUSED, ORACLE_SAMPLE, solve_in_chunks,
                              strided_sample, take)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    import __graft_entry__ as g
    g.build()
    from oracle.oracle import Oracle
    from robot_mpcs_amd._lib import Solver
    from robot_mpcs_amd.scenarios import make_scenario
    return dict(Oracle=Oracle, Solver=Solver, make_scenario=make_scenario)


def _pass_kernel_env(monkeypatch):
    """The pass kernels with every other switch as shipped (all of them are read once, at rmpc_create)."""
    for k in ("RMPC_NO_MIGRATE", "RMPC_RIC_LANE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in NO_FUSED.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name,B,seed,kw,ric_first", GROUPED_CASES)
def test_grouped_blocks_and_their_hand_over_match_oracle(rt, name, B, seed, kw, ric_first, monkeypatch):
    """A list of at least kGroupedMin = 512 columns runs k_riccati's grouped blocks (half a wavefront per instance for
    the small models), and once the list has shrunk below that the same solve goes on in the one-wave blocks: both
    regimes and the hand-over between them inside one solve, against the oracle.  The list is the whole batch while more
    than an eighth of it iterates, so at these sizes the hand-over comes when at most B / 8 instances are left -- the
    cases are such that the host loop then still finds instances iterating and enqueues further passes.  The arm (cfg4)
    has no grouped blocks: its 530 one-wave blocks of the first pass are what its case pins."""
    _pass_kernel_env(monkeypatch)
    sc = rt["make_scenario"](name, B=B, seed=seed, **kw)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert not s.is_fused()
    gpu = s.solve(sc.xinit, sc.x0, sc.params)
    path = s.last_solve_path()
    s.close()
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit, sc.x0, sc.params)
    print("grouped %s B %d: %s | iters max %d | iteration counts equal to the oracle's %.4f"
          % (name, B, path, gpu["iters"].max(), (gpu["iters"] == cpu["iters"]).mean()))
    assert not path["fused"] and path["migrated_at"] == -1 and path["compact"] == "wave", path
    assert path["ric_first"] == ric_first and path["ric_last"] == "wave", path
    check_plan(gpu, cpu, sc.desc["nx"] + sc.desc["ns"])
    np.testing.assert_allclose(gpu["obj"], cpu["obj"], rtol=1e-9, atol=1e-9)


def _large_batch(rt, monkeypatch, name, B, seed):
    """One solve of B instances on the pass kernels, the same instances in chunks of CHUNK through a handle of that size
    (pass kernels too: k_compact_wave, the grouped blocks, a migration per chunk), and the oracle on a strided sample."""
    _pass_kernel_env(monkeypatch)
    sc = rt["make_scenario"](name, B=B, seed=seed)
    nxs = sc.desc["nx"] + sc.desc["ns"]
    big = rt["Solver"](sc.desc, max_batch=B)
    assert not big.is_fused()
    gpu = big.solve(sc.xinit, sc.x0, sc.params)
    path = big.last_solve_path()
    big.close()
    small = rt["Solver"](sc.desc, max_batch=CHUNK)
    assert not small.is_fused()
    chunks, cpaths = solve_in_chunks(small, sc.xinit, sc.x0, sc.params, CHUNK)
    small.close()
    cpath = cpaths[0]
    assert len(cpaths) == B // CHUNK + 1     # (full chunks and a short one)
    for c in cpaths[:-1]:
        assert not c["fused"] and c["compact"] == "wave" and c["ric_first"] == "grouped" and c["migrated_at"] >= 8, c
    assert not cpaths[-1]["fused"] and cpaths[-1]["ric_first"] == "wave" and cpaths[-1]["migrated_at"] == -1, cpaths[-1]
    idx = strided_sample(B, ORACLE_SAMPLE)
    cpu = rt["Oracle"](sc.desc).solve_batch(sc.xinit[idx], sc.x0[idx], sc.params[idx])
    print("large %s B %d: %s | first chunk %s | iters max %d | iteration counts equal: oracle sample %.4f, chunks %.4f | plans equal to the chunks' bit for bit %.4f"
          % (name, B, path, cpath, gpu["iters"].max(), (gpu["iters"][idx] == cpu["iters"]).mean(),
             (gpu["iters"] == chunks["iters"]).mean(), (gpu["z"] == chunks["z"]).all(axis=(1, 2)).mean()))
    return sc, gpu, path, chunks, cpu, idx, nxs


def _check_large(gpu, chunks, cpu, idx, nxs):
    # the oracle on its sample; the chunked run in the oracle's place on everything (same bars, no bit-identity: the
    # regimes differ); and every instance usable
    check_plan(take(gpu, idx), cpu, nxs)
    check_plan(gpu, chunks, nxs)
    assert np.all(gpu["exitflag"] >= 0)
    assert gpu["kkt"][gpu["exitflag"] == 1].max() <= 1e-6


def test_block_list_builder_matches_oracle_and_chunks(rt, monkeypatch):
    """B = 8192 + 65 > kCompactWaveMax: the list of iterating instances is built by k_compact (one block of 1024
    threads, a scan over nine columns per thread with a ragged last thread) instead of k_compact_wave -- every pass of the
    solve until the survivors migrate."""
    sc, gpu, path, chunks, cpu, idx, nxs = _large_batch(rt, monkeypatch, "cfg2", B_COMPACT_BLOCK, 57)
    assert not path["fused"] and path["compact"] == "block", path
    assert path["ric_first"] == "grouped" and path["migrated_at"] >= 8 and path["survivors"] >= 8, path
    _check_large(gpu, chunks, cpu, idx, nxs)


@pytest.mark.parametrize("name,seed", [("cfg2", 58), ("chain2", 59)])
def test_lane_recursion_by_default_matches_oracle_and_chunks(rt, name, seed, monkeypatch):
    """B = 16384 + 37 >= kLaneMin with no RMPC_RIC_LANE: the chains with at most 3 joints start on k_riccati_lane (one
    lane per instance, 257 wavefronts, the last with 37 lanes in use), and when the survivors migrate the list falls
    below the threshold and the same instances go on in k_riccati -- another recursion in the middle of a solve."""
    sc, gpu, path, chunks, cpu, idx, nxs = _large_batch(rt, monkeypatch, name, B_LANE, seed)
    assert not path["fused"] and path["compact"] == "block" and path["ric_first"] == "lane", path
    assert path["migrated_at"] >= 8 and 8 <= path["survivors"] <= B_LANE // 8, path
    assert path["ric_last"] in ("wave", "grouped"), path
    _check_large(gpu, chunks, cpu, idx, nxs)


def test_large_batch_does_not_depend_on_stale_workspace(rt, monkeypatch):
    """test_solve_does_not_depend_on_stale_lds at a size where the compact workspace is used in earnest: B = 8192 + 65
    twice through one handle, LDS, scratch and the whole workspace (the compact one included) filled with NaN patterns in
    between -- bit for bit the same results, with a migration of hundreds of survivors in both."""
    _pass_kernel_env(monkeypatch)
    B = B_COMPACT_BLOCK
    sc = rt["make_scenario"]("cfg2", B=B, seed=57)
    s = rt["Solver"](sc.desc, max_batch=B)
    assert not s.is_fused()
    clean = s.solve(sc.xinit, sc.x0, sc.params)
    p1 = s.last_solve_path()
    s.poison_lds()
    dirty = s.solve(sc.xinit, sc.x0, sc.params)
    p2 = s.last_solve_path()
    s.close()
    print("poison twin cfg2 B %d: %s" % (B, p1))
    assert p1 == p2 and p1["compact"] == "block" and p1["migrated_at"] >= 8 and p1["survivors"] >= 64, (p1, p2)
    for key in ("z", "exitflag", "iters", "obj", "kkt"):
        assert np.array_equal(clean[key], dirty[key]), key
    assert np.isin(clean["exitflag"], (1, 2)).mean() > 0.95
