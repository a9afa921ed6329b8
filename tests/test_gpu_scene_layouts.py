"""The scene packer k_scene (csrc/rmpc_batch.hpp) in its three output layouts, on every parameter row, against the plain
restatement scene_reference.pack_scene_ref (which test_scene_cpu.py holds to the host packer and to the reference's
loops).  Cases: scene_cases.py -- every field differs by instance, by joint and by stage.

  layout 0   rmpc_pack_scene_device, [b][k][npar]: the output array itself, bit for bit, NaN-poisoned beforehand and
             with 32 poisoned words behind it that must come back untouched
  layout 1   the pass kernels' [off][k][Bp], written into the workspace   } seen through the solve: the scene solve and
  layout 2   the fused kernels' [b][off][32 stages]                       } the packed solve equal, bit for bit, the plain
             solve of the SAME handle type fed pack_scene_ref (z, kkt_res, obj as uint64; exit flags and iteration counts
             exact), the workspace filled with 0xff bytes immediately before each pack (a slot the packer skipped and
             the solver reads is then a NaN, not yesterday's value).  What makes this a check of every word: scaling one
             entry of one instance by 1 + 1e-3 changes the bits of that instance's plan and of no other, for every
             parameter group (asserted of the oracle for every row in test_scene_cpu.py, and of the plain device solve
             for one row per layout here), and the plain solves are ordinary ones (>= 90 % flag 1, >= 2 iterations).

Every row asserts ``is_fused()``, so that it cannot silently test the other layout; the migration row asserts through
``last_solve_path()`` that the SCENE solve moved survivors to the compact workspace (k_migrate carries the parameters)."""
import numpy as np
import pytest

from scene_cases import (NO_FUSED, ROWS, VARIANTS, field_tensors, make_case_scene, perturbed_instance_params, reference_params,
                         row_case, row_id, scene_case, sensitivity_groups)
from scene_reference import pack_scene_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x7ff8dead0000beef      # a NaN pattern no packer writes
TAIL = 32


@pytest.fixture(scope="module")
def rt():
    import torch
    import __graft_entry__ as g
    g.build()
    from robot_mpcs_amd._lib import RmpcError, Solver
    return dict(torch=torch, Solver=Solver, RmpcError=RmpcError)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _handle(rt, monkeypatch, desc, max_batch, env=None):
    """A handle with the switches that rmpc_create reads set as the row says and every other one as shipped."""
    for k in ("RMPC_NO_FUSED", "RMPC_NO_MIGRATE", "RMPC_RIC_LANE", "RMPC_NO_SPEC", "RMPC_FUSED_GRID", "RMPC_NO_ORDER",
              "RMPC_NO_COLD_ORDER", "RMPC_ARM_TWO_PARTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return rt["Solver"](desc, max_batch=max_batch)


# ---- layout 0 ------------------------------------------------------------------------------------------------------------
LAYOUT0_CONFIGS = ["cfg2", "cfg3", "cfg4", "wc_point", "wc_boxer", "wc_boxer_slack", "chain8"]
LAYOUT0 = [(n, B, B, "all", {}) for n in LAYOUT0_CONFIGS for B in (1, 63, 65, 130)]
LAYOUT0 += [(n, 65, 65, v, {}) for n in LAYOUT0_CONFIGS for v in VARIANTS if v != "all"]
LAYOUT0 += [("cfg3", 65, 130, "all", {}), ("wc_boxer", 65, 130, "all", {})]          # one handle of 130 called with 65
LAYOUT0 += [("cfg2", 65, 65, "all", {"time_horizon": 1}), ("cfg2", 65, 65, "all", {"time_horizon": 40})]


def _layout0_id(c):
    name, B, max_batch, variant, kw = c
    return "-".join([name, "B%d" % B] + (["max%d" % max_batch] if max_batch != B else []) + ([variant] if variant != "all" else [])
                    + ["N%d" % v for v in kw.values()])


@pytest.mark.parametrize("c", LAYOUT0, ids=_layout0_id)
def test_abi_layout_equals_restatement(rt, monkeypatch, c):
    torch = rt["torch"]
    name, B, max_batch, variant, kw = c
    case = scene_case(name, B, 1, **kw)
    ref = reference_params(case, variant)
    s = _handle(rt, monkeypatch, case.desc, max_batch)
    scene, _keep = make_case_scene(torch, s, case, variant)
    words = B * case.N * case.desc["npar"]
    out = torch.full((words + TAIL,), POISON, dtype=torch.int64, device=DEV).view(torch.float64)
    s.pack_scene_device(B, scene, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    s.close()
    assert np.all(got[words:] == POISON), "words behind the array were written"
    diff = np.flatnonzero(got[:words] != _bits(ref).reshape(-1))
    assert diff.size == 0, (diff.size, [np.unravel_index(i, ref.shape) for i in diff[:8]])


# ---- layouts 1 and 2, through the solve -----------------------------------------------------------------------------------
def _outputs(torch, B, N, nv):
    f64, i32 = dict(dtype=torch.float64, device=DEV), dict(dtype=torch.int32, device=DEV)
    return dict(z=torch.full((B, N, nv), float("nan"), **f64), ef=torch.full((B,), -77, **i32), it=torch.full((B,), -77, **i32),
                kkt=torch.full((B,), float("nan"), **f64), obj=torch.full((B,), float("nan"), **f64))


def _fetch(torch, o):
    torch.cuda.synchronize()
    return dict(z=o["z"].cpu().numpy(), exitflag=o["ef"].cpu().numpy(), iters=o["it"].cpu().numpy(), kkt=o["kkt"].cpu().numpy(),
                obj=o["obj"].cpu().numpy())


def _scene_solve(rt, s, case, scene, halves, poison=True):
    """One solve from a scene (``halves``: pack_scene_workspace + solve_packed_device instead of solve_scene_device), the
    workspace filled with 0xff bytes immediately before the pack."""
    torch = rt["torch"]
    B = case.B
    tx = torch.from_numpy(np.ascontiguousarray(case.xinit)).to(DEV)
    t0 = torch.from_numpy(np.ascontiguousarray(case.x0)).to(DEV)
    o = _outputs(torch, B, case.N, s.nvar)
    torch.cuda.synchronize()
    if poison:
        s.poison_lds()
    if halves:
        s.pack_scene_workspace(B, scene)
        s.solve_packed_device(B, tx, t0, o["z"], o["ef"], o["it"], o["kkt"], o["obj"])
    else:
        s.solve_scene_device(B, scene, tx, t0, o["z"], o["ef"], o["it"], o["kkt"], o["obj"])
    return _fetch(torch, o)


def _assert_same_solve(got, want, what):
    for key in ("z", "kkt", "obj"):
        bad = np.flatnonzero((_bits(got[key]) != _bits(want[key])).reshape(len(want["exitflag"]), -1).any(axis=1))
        assert bad.size == 0, (what, key, bad[:16])
    assert np.array_equal(got["exitflag"], want["exitflag"]), (what, np.flatnonzero(got["exitflag"] != want["exitflag"])[:16])
    assert np.array_equal(got["iters"], want["iters"]), (what, np.flatnonzero(got["iters"] != want["iters"])[:16])


def _assert_ordinary(plain):
    """the conditions that keep a row from passing vacuously, on the reference side"""
    assert (plain["exitflag"] == 1).mean() >= 0.9, (plain["exitflag"] == 1).mean()
    assert plain["iters"].min() >= 2, plain["iters"].min()
    assert np.all(np.isfinite(plain["z"][plain["exitflag"] == 1]))


@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_scene_solve_equals_plain_solve(rt, monkeypatch, r):
    torch = rt["torch"]
    case = row_case(r)
    params = reference_params(case)
    s = _handle(rt, monkeypatch, case.desc, r.max_batch, r.env)
    assert s.is_fused() == r.fused
    plain = s.solve(case.xinit, case.x0, params)
    plain_path = s.last_solve_path()
    _assert_ordinary(plain)
    scene, _keep = make_case_scene(torch, s, case)
    one = _scene_solve(rt, s, case, scene, halves=False)
    one_path = s.last_solve_path()
    two = _scene_solve(rt, s, case, scene, halves=True)
    two_path = s.last_solve_path()
    s.close()
    print("%s: fused %s | plain %s | scene %s | iters %d .. %d" % (row_id(r), r.fused, plain_path, one_path, plain["iters"].min(),
                                                                plain["iters"].max()))
    if r.migrates:
        for path in (plain_path, one_path, two_path):
            assert not path["fused"] and path["migrated_at"] >= 8 and path["survivors"] >= 1, path
    _assert_same_solve(one, plain, "solve_scene_device")
    _assert_same_solve(two, plain, "pack_scene_workspace + solve_packed_device")


SENSITIVITY_ROWS = [r for r in ROWS if (r.name, r.B, r.fused, bool(r.env), r.max_batch, bool(r.overrides)) in (
    ("cfg2", 65, True, False, 65, False), ("cfg4", 33, True, False, 33, False), ("chain4", 65, False, False, 65, False),
    ("wc_boxer", 65, False, True, 65, False))]


@pytest.mark.parametrize("r", SENSITIVITY_ROWS, ids=row_id)
def test_plain_device_solve_sees_every_parameter_group(rt, monkeypatch, r):
    """test_scene_cpu.py::test_every_parameter_group_moves_the_oracle_plan with the plain device solve, one row per kernel
    family (k_fused, k_fused_arm, the pass kernels by themselves and forced): one entry of instance B // 2 scaled by
    1 + 1e-3 changes that instance's plan and no other instance's."""
    case = row_case(r)
    b = case.B // 2
    ref = reference_params(case)
    s = _handle(rt, monkeypatch, case.desc, r.max_batch, r.env)
    assert s.is_fused() == r.fused
    base = s.solve(case.xinit, case.x0, ref)
    others = np.arange(case.B) != b
    unmoved, leaked = [], []
    for label, apply in sensitivity_groups(case):
        params = np.array(ref)
        params[b] = perturbed_instance_params(case, b, apply)
        got = s.solve(case.xinit, case.x0, params)
        if np.array_equal(_bits(got["z"][b]), _bits(base["z"][b])):
            unmoved.append(label)
        if not (np.array_equal(_bits(got["z"][others]), _bits(base["z"][others])) and
                np.array_equal(got["iters"][others], base["iters"][others])):
            leaked.append(label)
    s.close()
    assert len(SENSITIVITY_ROWS) == 4
    assert not unmoved and not leaked, (unmoved, leaked)


# ---- re-packing on one handle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,fused", [({}, True), (NO_FUSED, False)], ids=["fused", "nofused"])
def test_repacking_leaves_nothing_of_the_previous_scene(rt, monkeypatch, env, fused):
    """A loop packs into the same handle every control step.  wc_boxer (planes per stage, velocity limits, no obstacle
    slots): scene A with every field, then scenes with fewer fields and a smaller batch into the same handle -- each solve
    equals the same scene's on a fresh handle bit for bit (no 0xff fill in between: what A left is what would leak)."""
    torch = rt["torch"]
    big, small = scene_case("wc_boxer", 65, 1), scene_case("wc_boxer", 33, 2)

    def solve(s, case, variant):
        scene, _keep = make_case_scene(torch, s, case, variant)
        return _scene_solve(rt, s, case, scene, halves=False, poison=False)

    def fresh(case, variant):
        s = _handle(rt, monkeypatch, case.desc, case.B, env)
        out = solve(s, case, variant)
        s.close()
        return out

    s = _handle(rt, monkeypatch, big.desc, 65, env)
    assert s.is_fused() == fused
    first = solve(s, big, "all")
    _assert_ordinary(first)
    _assert_same_solve(first, s.solve(big.xinit, big.x0, reference_params(big)), "scene A")
    for variant in ("bare", "no_obstacles", "all"):
        _assert_same_solve(solve(s, big, variant), fresh(big, variant), "%s after A" % variant)
    # (the last pack above was A at B = 65)
    _assert_same_solve(solve(s, small, "all"), fresh(small, "all"), "B = 33 after B = 65")
    _assert_same_solve(solve(s, small, "bare"), fresh(small, "bare"), "bare at B = 33 after B = 65")
    s.close()


@pytest.mark.parametrize("env,fused", [({}, True), (NO_FUSED, False)], ids=["fused", "nofused"])
def test_packed_solve_is_refused_without_a_pack_of_its_size(rt, monkeypatch, env, fused):
    torch = rt["torch"]
    case = scene_case("wc_boxer", 65, 1)
    s = _handle(rt, monkeypatch, case.desc, 65, env)
    assert s.is_fused() == fused
    tx = torch.from_numpy(np.ascontiguousarray(case.xinit)).to(DEV)
    t0 = torch.from_numpy(np.ascontiguousarray(case.x0)).to(DEV)
    o = _outputs(torch, 65, case.N, s.nvar)
    packed = lambda B: s.solve_packed_device(B, tx, t0, o["z"], o["ef"], o["it"], o["kkt"], o["obj"])
    with pytest.raises(rt["RmpcError"]):     # a new handle: nothing packed
        packed(65)
    scene, _keep = make_case_scene(torch, s, case)
    s.pack_scene_workspace(65, scene)
    with pytest.raises(rt["RmpcError"]):     # another batch size than the packed one
        packed(33)
    packed(65)
    packed(65)                               # (the parameters stay: a packed solve does not consume them)
    s.solve(case.xinit, case.x0, reference_params(case))
    with pytest.raises(rt["RmpcError"]):     # a plain solve has overwritten the workspace parameters
        packed(65)
    s.pack_scene_workspace(33, scene)
    with pytest.raises(rt["RmpcError"]):
        packed(65)
    packed(33)
    torch.cuda.synchronize()
    s.close()


# ---- one control step of the real chain ------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,fused", [({}, True), (NO_FUSED, False)], ids=["fused", "nofused"])
def test_scene_is_read_at_solve_time(rt, monkeypatch, env, fused):
    """fleet.make_block + step_block(flags=True), wc_boxer at B = 65, two control steps with the warm start on; the goal
    and plane tensors change IN PLACE between the steps, the way k_retarget and LidarPlanes change them.  After each
    step the plan equals the plain warm-started solve of a second handle fed pack_scene_ref of the tensors as they stood."""
    torch = rt["torch"]
    from robot_mpcs_amd.fleet import make_block, step_block
    for k in ("RMPC_NO_FUSED", "RMPC_NO_MIGRATE", "RMPC_RIC_LANE", "RMPC_NO_SPEC", "RMPC_FUSED_GRID", "RMPC_NO_ORDER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = scene_case("wc_boxer", 65, 1)
    B = case.B
    ten = field_tensors(torch, case.fields)
    f = make_block(case.desc, case.weights, B, case.xinit, DEV, x0=case.x0, **ten)
    ref = rt["Solver"](case.desc, max_batch=B)
    assert f["s"].is_fused() == fused and ref.is_fused() == fused
    f["s"].set_warm_start(True)
    ref.set_warm_start(True)
    rng = np.random.default_rng(5)
    fields = {k: (None if v is None else np.array(v)) for k, v in case.fields.items()}
    for step in range(2):
        if step == 1:
            dgoal = rng.uniform(-0.3, 0.3, size=(B, 3)) * np.array([1.0, 1.0, 0.0])
            dplane = rng.uniform(0.0, 0.05, size=(B, case.N, case.desc["nobst"]))
            ten["goal"].add_(torch.from_numpy(dgoal).to(DEV))
            ten["lin_constrs"][:, :, :, 3].add_(torch.from_numpy(dplane).to(DEV))
            torch.cuda.synchronize()
            # (the restatement packs what the tensors hold now, fetched from the device: the sums are the device's)
            fields["goal"], fields["lin_constrs"] = ten["goal"].cpu().numpy(), ten["lin_constrs"].cpu().numpy()
            assert not np.array_equal(fields["goal"], case.fields["goal"])
        xin, x0 = f["x"].cpu().numpy(), f["x0"].cpu().numpy()
        step_block(f, previous_plan=True, flags=True)
        torch.cuda.synchronize()
        want = ref.solve(xin, x0, pack_scene_ref(case.desc, case.N, case.weights, case.dyn_radius, fields))
        got = dict(z=f["z"].cpu().numpy(), exitflag=f["ef"].cpu().numpy(), iters=f["it"].cpu().numpy(), kkt=f["kkt"].cpu().numpy(),
                   obj=f["obj"].cpu().numpy())
        if step == 0:
            _assert_ordinary(want)
        _assert_same_solve(got, want, "control step %d" % step)
        if step == 1:
            stale = ref.solve(xin, x0, reference_params(case))
            assert not np.array_equal(_bits(stale["z"]), _bits(want["z"]))     # (the change of the scene is visible in the plan)
    f["s"].close()
    ref.close()
