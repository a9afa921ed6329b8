"""Kinematics and curvature on chains that mix revolute and prismatic joints (chain_cases.py): the
URDF parser, the oracle's model functions, kinematics and curvature terms, its Newton step and the rule that switches
the curvature terms of a chain of three or fewer joints.  The shipped chains reach none of: a prismatic joint among
more than three, a revolute joint before a prismatic one, a revolute axis off local z, an origin rotation with pitch or
yaw, three joints whose frames are not affine in q.  No GPU needed.

Anchors: chain_reference.py (scipy rotations, 4 x 4 products, differences with Richardson extrapolation) shares neither
the parser nor a walk of the chain with the package, the oracle or oracle/nlp_numpy.py; the oracle's values, derivatives
and Gauss-Newton block run through test_oracle_model.py's checks (its CASES hold the new classes); the curvature terms
and the step through exact_hessian_cases.py and newton_step_cases.py with their bounds as they stand.

Measured (the tests print the figures):
  parser                |fk_positions - reference| at most 1.3e-15 (bound 1e-13 max(1, |p|))
  oracle kinematics     against chain_reference: positions 6.7e-16, Jacobians 6.0e-14, second derivatives 1.4e-11,
                        distance rows 4.4e-16, their Jg rows 5.2e-14
  |C - C_ref| / scale   (oracle, B = 4, worst stage and instance; bound of (b): u + 9.0e-10)
                        N = 4: cold at most 1.6e-12 (mix8), conv 1.2e-11 (mix5); own N: cold at most 3.4e-12 (mix7),
                        conv 3.6e-11 (mix4).  The reference's own uncertainty u is larger here than on the shipped
                        chains: up to 2.0e-6 (mix5, N = 4) against 2.4e-9 -- still four orders below a missing term
  mix2, mix3, aff3      C == 0 exactly, the step at cw = 1 is the step at cw = 0 bit for bit
  aff3 before the rule asked for an affine goal frame: |C - C_ref| / scale 2.5e-2 .. 1.5e-1 (the goal cost's kinematic
                        term, absent for n <= 3; C[1][1] = 0 where the reference has -0.11 .. -0.59), all 16 instances
                        (four per horizon and mode) outside the bound
  step error over the textbook recursion's: at most 1.87 cold, 1.02 late; on the exact Hessian 1.89 cold, 2.04 conv
                        (bound 16).  8 of the 64 cold instances of (c) are not positive definite: ok = 0 for each
"""
import functools

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import chain_cases as cc
import chain_reference as cref
import exact_hessian_cases as ehc
import kkt_reference as ref
import newton_step_cases as nsc

EPS = np.finfo(np.float64).eps
POS_TOL = 1e-13          # positions: the project's bound, times max(1, |p|)
JAC_FLOOR = 1e-10        # first differences at h / 4 = 5e-3 round at eps |p| / h = 5e-14, Richardson's weights double it:
                         # 1e-10 is far above that and eight orders below a wrong column (1e-2 .. 1)
CURV_FLOOR = 1e-8        # second differences at h / 4 = 1.25e-2 round at 4 eps |p| / h^2 = 6e-12: the same margins
H4 = {"time_horizon": 4}


@pytest.fixture(scope="module")
def rt(oracle_lib):
    @functools.lru_cache(maxsize=None)
    def prepared(name, mode, kw):
        sc, o, xinit, x0, params, duals = ehc.make_inputs(cc.make_chain_scenario, oracle_lib.Oracle, name, mode, kw)
        refs = [ehc.instance_reference(o, mode, xinit, x0, params, duals, b) for b in range(ehc.B)]
        return sc, o, xinit, x0, params, duals, refs

    return dict(Oracle=oracle_lib.Oracle, prepared=prepared)


# ---- parser ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mix8", "aff3"])
def test_parser_and_fk_match_the_chain_reference(name):
    """parse_chain, rpy_to_matrix and fk_positions against the 4 x 4 product of chain_reference, every frame."""
    from robot_mpcs_amd.utils.urdf_chain import fk_positions, parse_chain
    n = cc.CLASSES[name]["n"]
    with open(cc.urdf_file(name)) as f:
        chain = parse_chain(f.read(), "l0", "l%d" % n)
    rchain = cc.reference_chain(name)
    assert chain.n() == n == len(rchain)
    assert [j.child for j in chain.joints] == [j["child"] for j in rchain]
    rng = np.random.default_rng(11)
    q = rng.uniform(-1.0, 1.0, size=(8, n))
    got = fk_positions(chain.joints, q, range(n))
    worst = 0.0
    for b in range(q.shape[0]):
        for f in range(n):
            want = cref.position(rchain, q[b], f)
            err = float(np.abs(got[f][b] - want).max())
            worst = max(worst, err)
            assert err <= POS_TOL * max(1.0, float(np.abs(want).max())), (b, f, err)
    print("chain %s: |fk_positions - reference| at most %.2e" % (name, worst))


@pytest.mark.parametrize("rpy", [(0.3, -0.2, 0.5), (-0.4, 0.6, 0.2), (1.1, -0.5, 0.4), (-0.9, 0.4, 1.2), (2.5, -1.3, -2.8),
                                 (0.0, 0.7, 0.0), (0.0, 0.0, -1.9), (0.2, 1.5607, -0.3)])
def test_rpy_with_roll_pitch_and_yaw(rpy):
    """R = Rz(yaw) Ry(pitch) Rx(roll): URDF's fixed-axis angles are scipy's extrinsic "xyz".  An entry is a sum of at
    most two products of three sines and cosines, each within an ulp: 8 eps per side."""
    from robot_mpcs_amd.utils.urdf_chain import rpy_to_matrix
    R = np.array(rpy_to_matrix(rpy)).reshape(3, 3)
    np.testing.assert_allclose(R, Rotation.from_euler("xyz", rpy).as_matrix(), rtol=0, atol=16 * EPS)
    if rpy[1] != 0.0 and rpy[2] != 0.0 and rpy[1] != rpy[2]:   # the order matters at these angles: the swap is far away
        swapped = Rotation.from_euler("xyz", (rpy[0], rpy[2], rpy[1])).as_matrix()
        assert np.abs(R - swapped).max() > 1e-2


EDGE_URDF = """<?xml version="1.0"?>
<robot name="edge">
  <link name="a"/><link name="b"/><link name="c"/><link name="d"/><link name="e"/>
  <joint name="unnormalised" type="revolute">
    <parent link="a"/><child link="b"/><origin xyz="0.1 0.2 0.3" rpy="0.4 0.5 0.6"/><axis xyz="3 0 -4"/>
  </joint>
  <joint name="no_axis" type="prismatic">
    <parent link="b"/><child link="c"/><origin xyz="0.2 -0.1 0.1" rpy="-0.3 0.2 0.9"/>
  </joint>
  <joint name="no_origin" type="revolute">
    <parent link="c"/><child link="d"/><axis xyz="0 2 0"/>
  </joint>
  <joint name="turns_on" type="continuous">
    <parent link="d"/><child link="e"/><origin xyz="0.3 0.1 -0.2"/><axis xyz="1 1 1"/>
  </joint>
</robot>
"""


def test_parser_defaults_and_unnormalised_axes(tmp_path):
    """An axis the URDF does not give normalised, no <axis> (1 0 0), no <origin> and no rpy (identity), `continuous`."""
    from robot_mpcs_amd.utils.urdf_chain import JOINT_PRISMATIC, JOINT_REVOLUTE, fk_positions, parse_chain
    chain = parse_chain(EDGE_URDF, "a", "e")
    j = chain.joints
    assert [x.type for x in j] == [JOINT_REVOLUTE, JOINT_PRISMATIC, JOINT_REVOLUTE, JOINT_REVOLUTE]
    assert [x.dof for x in j] == [0, 1, 2, 3]
    np.testing.assert_allclose(j[0].axis, [0.6, 0.0, -0.8], rtol=0, atol=2 * EPS)
    assert j[1].axis == [1.0, 0.0, 0.0]
    assert j[2].xyz == [0.0, 0.0, 0.0] and j[2].rot == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0] and j[2].axis == [0.0, 1.0, 0.0]
    assert j[3].rot == j[2].rot
    np.testing.assert_allclose(j[3].axis, np.ones(3) / np.sqrt(3.0), rtol=0, atol=2 * EPS)
    path = tmp_path / "edge.urdf"
    path.write_text(EDGE_URDF)
    rchain = cref.read_chain(str(path), "e")
    rng = np.random.default_rng(12)
    q = rng.uniform(-2.0, 2.0, size=(6, 4))     # (a continuous joint has no limits: beyond +- 1 too)
    got = fk_positions(j, q, range(4))
    for b in range(6):
        for f in range(4):
            want = cref.position(rchain, q[b], f)
            np.testing.assert_allclose(got[f][b], want, rtol=0, atol=POS_TOL * max(1.0, float(np.abs(want).max())))


@pytest.mark.parametrize("name", cc.NAMES)
def test_descriptors_pass_the_library_checks(name):
    """build_model and build_tables of the library (host code, reached through the view generator's entry) accept every
    class -- four distinct collision points at the most, 24 variables for mix8 -- and no class has a generated view."""
    from robot_mpcs_amd._lib import spec_for, spec_source
    sc = cc.make_chain_scenario(name, B=1)
    assert "struct ChainView" in spec_source(sc.desc, "ChainView")
    assert spec_for(sc.desc) == ""
    assert sc.desc["n"] == cc.CLASSES[name]["n"] and sc.desc["N"] == cc.CLASSES[name]["N"]


# ---- the oracle's kinematics --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_kinematics_match_the_chain_reference(rt, name):
    """Positions, Jacobians and second derivatives (orc_fk, orc_fk_curv) of every frame, and the values and Jg rows of
    the distance rows of eval_stage, against chain_reference directly."""
    sc = cc.make_chain_scenario(name, B=3, seed=21)
    o = rt["Oracle"](sc.desc)
    d, n = sc.desc, o.n
    rchain = cc.reference_chain(name)
    rng = np.random.default_rng(22)
    worst = dict(p=0.0, J=0.0, D=0.0, g=0.0, Jg=0.0)
    for b in range(sc.B):
        q = sc.xinit[b, :n] + rng.uniform(-0.3, 0.3, size=n)
        P, J, U = {}, {}, {}
        for f in range(n):
            P[f] = cref.position(rchain, q, f)
            J[f], U[f] = cref.jacobian(rchain, q, f)
            pos, Jo = o.fk(q, f)
            ep, eJ = float(np.abs(pos - P[f]).max()), float(np.abs(Jo - J[f]).max())
            worst["p"] = max(worst["p"], ep); worst["J"] = max(worst["J"], eJ)
            assert ep <= POS_TOL * max(1.0, float(np.abs(P[f]).max())), (f, ep)
            assert eJ <= U[f] + JAC_FLOOR, (f, eJ, U[f])
            D, uD = cref.second_derivatives(rchain, q, f)
            F = rng.normal(size=3)
            eD = float(np.abs(o.fk_curv(q, f, F) - np.einsum("c,cab->ab", F, D)).max())
            worst["D"] = max(worst["D"], eD)
            assert eD <= np.abs(F).sum() * uD + CURV_FLOOR, (f, eD, uD)
        # the distance rows of a stage whose state is free: sphere rows link by link, then the pairs
        z = np.concatenate([q, rng.normal(0, 0.3, n), rng.normal(0, 0.5, o.nu)])
        p = sc.params[b].reshape(o.N, o.npar)[1]
        e = o.eval_stage(z, p)
        rb = p[d["off_r_body"]]
        ob = p[d["off_obst"]: d["off_obst"] + 4]
        rows = []
        for f in d["link_frame"]:
            dv = P[f] - ob[:3]
            rows.append((np.linalg.norm(dv) - ob[3] - rb, dv / np.linalg.norm(dv) @ J[f], U[f]))
        for a, c in d["pair_frame"]:
            dv = P[a] - P[c]
            rows.append((np.linalg.norm(dv) - 2.0 * rb, dv / np.linalg.norm(dv) @ (J[a] - J[c]), U[a] + U[c]))
        assert d["module_kind"][:2] == [0, 2] and len(rows) == len(d["link_frame"]) + len(d["pair_frame"])
        for r, (g, Jg, u) in enumerate(rows):
            eg, eJg = abs(e["g"][r] - g), float(np.abs(e["Jg"][r, :n] - Jg).max())
            worst["g"] = max(worst["g"], eg); worst["Jg"] = max(worst["Jg"], eJg)
            assert eg <= POS_TOL * 4.0, (r, eg)                      # (a norm of a difference of two positions)
            assert eJg <= np.sqrt(3.0) * u + JAC_FLOOR, (r, eJg, u)
            assert not np.any(e["Jg"][r, n:])
    print("chain %s: oracle against chain_reference: p %.1e J %.1e D %.1e g %.1e Jg %.1e" % (
        name, worst["p"], worst["J"], worst["D"], worst["g"], worst["Jg"]))


def test_the_mixed_chain_has_the_terms_the_shipped_chains_lack(rt):
    """What the classes are for: d2 p / dq_a dq_c of a revolute joint a before a prismatic joint c is axis_a x axis_c,
    not zero -- in the point robot the prismatic joints come first and every such term vanishes."""
    rchain = cc.reference_chain("mix8")
    D, u = cref.second_derivatives(rchain, np.full(8, 0.2), 7)
    for a, c in ((0, 1), (2, 4), (3, 4), (6, 7), (0, 7)):   # (revolute, prismatic behind it)
        assert np.abs(D[:, a, c]).max() > 0.1, (a, c)
    assert np.abs(D[:, 1, 4]).max() <= u + CURV_FLOOR and np.abs(D[:, 4, 4]).max() <= u + CURV_FLOOR   # two prismatic joints


# ---- the curvature terms and the rule ---------------------------------------------------------------------------------

CURV_CLASSES = [(n, kw) for n in cc.NAMES for kw in (H4, {})]


def _cid(c):
    return ehc.class_id(c[0], c[1])


@pytest.mark.parametrize("mode", ehc.MODES)
@pytest.mark.parametrize("cls", CURV_CLASSES, ids=_cid)
def test_oracle_exact_hessian_step_on_the_chains(rt, cls, mode):
    """Checks (b) and (c) of exact_hessian_cases.py on the oracle, at N = 4 and at the class's own N.  The classes without
    terms (mix2, mix3, aff3): C == 0 exactly and the step at cw = 1 equals the step at cw = 0 bit for bit."""
    name, kw = cls
    sc, o, xinit, x0, params, duals, refs = rt["prepared"](name, mode, tuple(sorted(kw.items())))
    label = "oracle %s %s" % (_cid(cls), mode)
    noterms = not cc.CLASSES[name]["use_curv"]
    insts, worst = [], 0.0
    for b, r in enumerate(refs):
        dl = None if duals is None else (duals[0][b], duals[1][b], duals[2][b])
        d = o.debug_step(xinit[b], x0[b], params[b], dl, curv=1.0)
        g = r["orc"]
        for key in ("Q", "C", "q", "A", "B", "rc", "t", "lam"):
            assert np.array_equal(d[key], g[key]), key
        assert np.array_equal(d["C"], np.transpose(d["C"], (0, 2, 1)))
        if noterms:
            assert not np.any(d["C"])
            assert np.array_equal(d["dz"], g["dz"]) and np.array_equal(d["nu"], g["nu"]) and d["ok"] == g["ok"]
        else:
            assert np.any(d["C"])
            worst = max(worst, ehc.check_against_reference("%s inst %d" % (label, b), d["C"], r))   # (b)
        insts.append(dict(Q=d["Q"], C=d["C"], q=d["q"], A=d["A"], B=d["B"], rc=d["rc"], t=d["t"], mu=d["mu"], dz=d["dz"],
                          nu=d["nu"], ok=d["ok"], evals=r["evals"], z=r["z"]))
    print("exact-hessian %s: |C - C_ref| / scale %.3e (u up to %.1e)" % (label, worst, max(r["u"].max() for r in refs)))
    ehc.check_steps(label, mode, o, 1.0, insts, nu_from=0)                                          # (c)


@pytest.mark.parametrize("name", cc.NAMES)
def test_use_curv_follows_the_rule(rt, name):
    """use_curv of every class as chain_cases tabulates it from the rule, read through the oracle's hook: with the
    multipliers of a converged plan the terms of a model that carries any are not zero (the distance rows' own
    curvature alone is (lam + c N / h^2) (I - n n^T) / d per row)."""
    sc, o, xinit, x0, params, duals, refs = rt["prepared"](name, "conv", ())
    got = [int(np.any(r["orc"]["C"])) for r in refs]
    assert got == [cc.CLASSES[name]["use_curv"]] * len(refs), (name, got)


def test_the_goal_on_a_turning_frame_is_what_switches_aff3_off(rt):
    """aff3's distance rows sit on affine frames: without the goal cost the rule keeps the terms and they are exact
    (check (b) on the same inputs); aff3g, whose goal sits on an affine frame, keeps them with the goal.  With the goal
    on l3 the exact Hessian has a kinematic term of the goal cost that a chain of three joints does not carry: the
    reference's C over the q block is not zero there, so Gauss-Newton is the honest choice."""
    sc, o, xinit, x0, params, duals, refs = rt["prepared"]("aff3", "conv", ())
    assert int(sc.desc["end_frame"]) == 2 and sc.desc["has_goal"]
    nogoal = dict(sc.desc, has_goal=0)
    o2 = rt["Oracle"](nogoal)
    big = 0.0
    for b, r in enumerate(refs):
        d = o2.debug_step(xinit[b], x0[b], params[b], (duals[0][b], duals[1][b], duals[2][b]), curv=0.0)
        assert np.any(d["C"])
        r2 = ehc.instance_reference(o2, "conv", xinit, x0, params, duals, b)
        ehc.check_against_reference("aff3 without goal inst %d" % b, d["C"], r2)
        # the goal's own second-order term: what the two references differ by
        big = max(big, float(np.abs(r["Cref"] - r2["Cref"]).max()))
    assert big > 1e-3, big


# ---- the Newton step ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", nsc.MODES)
@pytest.mark.parametrize("name", cc.NAMES)
def test_oracle_step_matches_dense_kkt_on_the_chains(rt, name, mode):
    """test_newton_step_cpu.py's check on the new classes: B = 6, the 16 x textbook bound as it stands."""
    B = 6
    sc, o, xinit, x0, params, duals = nsc.make_inputs(cc.make_chain_scenario, rt["Oracle"], name, mode, B)
    errs, yard = [], []
    for b in range(B):
        d = o.debug_step(xinit[b], x0[b], params[b], None if duals is None else (duals[0][b], duals[1][b], duals[2][b]))
        assert d["ok"]
        assert d["mu"] == (sc.desc["options"]["mu0"] if mode == "cold" else nsc.WARM_MU_MIN)
        dz_ref, nu_ref, e_text, rel = nsc.reference_and_yardstick(d["Q"], d["q"], d["A"], d["B"], d["rc"])
        assert rel < ref.REFINE_TOL
        errs.append(ref.block_errors(d["dz"], d["nu"], dz_ref, nu_ref, o.nx))
        yard.append(e_text)
        if mode == "cold":
            evals, z = nsc.stage_evals(o, xinit[b], x0[b], params[b])
            nsc.check_descent(ref.merit_slope(evals, z, d["t"], d["mu"], d["dz"], dz_ref), d["dz"])
    nsc.check_class("oracle %s %s" % (name, mode), errs, yard)
