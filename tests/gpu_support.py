"""What the GPU test modules share: the device, the one host-to-device copy, and check_plan, the bars of a plan against
the CPU oracle's (the tolerance is stated in tests/test_gpu_parity.py; the fused-kernel tests apply the same bars)."""
import numpy as np

DEV = "cuda:0"
TOL = 1e-6


def _t(torch, a, dtype=None, dev=DEV):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype if dtype is not None else torch.float64).to(dev)    # (a copy)


def check_plan(gpu, cpu, nxs, tol_stat=1e-6):
    # equal exit flags; a converged <-> acceptable flip is tolerated only when the KKT residual sits within
    # 2x the tolerance (rounding decides which stop fires first there; fleet.flags_consistent)
    from robot_mpcs_amd.fleet import flags_consistent
    assert flags_consistent(gpu["exitflag"], cpu["exitflag"], gpu["kkt"], tol_stat), \
        np.flatnonzero(gpu["exitflag"] != cpu["exitflag"])
    conv = np.isin(cpu["exitflag"], (1, 2))  # converged or acceptable level
    zs = np.maximum(1.0, np.abs(cpu["z"]).reshape(len(conv), -1).max(axis=1))
    dz = np.abs(gpu["z"] - cpu["z"]).reshape(len(conv), -1).max(axis=1)
    du = np.abs(gpu["z"][:, 0, nxs:] - cpu["z"][:, 0, nxs:]).max(axis=1)
    us = np.maximum(1.0, np.abs(cpu["z"][:, 0, nxs:]).max(axis=1))
    assert np.all(du[conv] <= TOL * us[conv]), du[conv].max()
    assert np.all(dz[conv] <= TOL * zs[conv]), dz[conv].max()
    # same algorithm, same arithmetic: iteration counts agree (allow rare borderline flips)
    assert (gpu["iters"] == cpu["iters"]).mean() >= 0.98
