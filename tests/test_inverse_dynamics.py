"""The no-GPU half of the inverse-dynamics tests (inputs, references, metric and tolerances: inverse_dynamics_cases.py; the kernel
on the GPU: test_gpu_inverse_dynamics.py).

 * the entry is exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states its contract, the
   wrapper has the accessors;
 1 the reference is right: tau_ref against the independent numpy fp64 Newton-Euler of test_oracle_kat.py <= 1e-8, and forward
   dynamics under tau_ref gives qdd back <= 1e-9;
 2 the device function inverse_dynamics (csrc/mppi_device.hpp) itself, compiled for the host, meets the GPU half's tolerance for
   every robot at every base pose, for all combinations of terms, with qdd given and left out;
 3 gravity off in the model: the gravity-only result is exactly 0; nothing asked for: exactly 0;
 4 a pass means something, on the reference alone: leaving out any part, an env's neighbour's q, qd or qdd, a neighbouring joint's
   qdd, gravity along the base's axes instead of the world's - each moves some entry by >= 100 tolerances; the fp32 restatement the
   tolerance comes from is re-measured here and sits within a tenth of it;
 5 the host build refuses a moving base without writing;
 9 / 10 the oracle side of the two closed-loop rows of the GPU half: under g_ref the effort-driven arm stays at rest and under a zero
   command every env sags by more than 100 bounds; the computed-torque identity qd' - qd = h qdd holds on the oracle to 1e-9 with no
   limit of the model in reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import inverse_dynamics_cases as ic
import jacobian_cases as jc
from mppiisaac.backend import capi

ROBOT_IDS = list(ic.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def test_the_entry_is_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_inverse_dynamics"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    assert (capi.ID_GRAVITY, capi.ID_VELOCITY) == (ic.ID_GRAVITY, ic.ID_VELOCITY) == (1, 2)
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    assert "mppi_sim_inverse_dynamics" in capi.EXPORTED_SYMBOLS
    getattr(lib, "mppi_sim_inverse_dynamics")
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    assert "int mppi_sim_inverse_dynamics(" in header
    for said in ("#define MPPI_ID_GRAVITY   1", "#define MPPI_ID_VELOCITY  2", "free of contact", "must not overlap", "MOVING base", "exact zeros"):
        assert said in header, said
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("acquire_bias_force_tensor", "refresh_bias_force_tensors", "inverse_dynamics"):
        assert callable(getattr(IsaacGymWrapper, name))


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_the_reference_is_right(robot, oracle64):
    from test_oracle_kat import rnea
    for pose in ic.POSES[robot]:
        scene, model, root, parts, D, _ = ic.references(robot, pose)
        dof, qdd = ic.inputs(robot, pose)
        q, qd, a = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64), qdd.astype(np.float64)
        gb = ic.gravity_in_base(model, root)
        assert np.abs(gb).max() > 9.0
        tau_ref = ic.combine(parts, *ic.FULL)
        worst_ne = worst_fd = 0.0
        for k in range(len(q)):
            worst_ne = max(worst_ne, np.abs(rnea(scene.robot_model, q[k], qd[k], a[k], gb) - tau_ref[k]).max())
            worst_fd = max(worst_fd, np.abs(oracle64.forward_dynamics(model, root, q[k], qd[k], tau_ref[k]) - a[k]).max())
        # the parts, against the same independent pass with the other inputs zeroed
        zero = np.zeros(q.shape[1])
        worst_part = 0.0
        for k in range(0, len(q), 8):
            worst_part = max(worst_part, np.abs(rnea(scene.robot_model, q[k], zero, zero, gb) - parts["g"][k]).max(),
                             np.abs(rnea(scene.robot_model, q[k], qd[k], zero, np.zeros(3)) - parts["C"][k]).max(),
                             np.abs(rnea(scene.robot_model, q[k], zero, a[k], np.zeros(3)) - parts["M"][k]).max())
        print(f"\n[{robot} {pose}] K {len(q)}: tau_ref against the numpy Newton-Euler {worst_ne:.1e} (1e-8), its parts {worst_part:.1e} (1e-8), "
              f"FD(tau_ref) - qdd {worst_fd:.1e} (1e-9); D_j {np.array2string(D, precision=3)}")
        assert np.isfinite(tau_ref).all() and (D > 0.0).all()
        assert worst_ne <= 1e-8 and worst_part <= 1e-8 and worst_fd <= 1e-9


# ---- 2., 3., 5. the host build ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu_id():
    d = os.path.join(HERE, "hostemu_inverse_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libinverse_dynamics_hostemu.so"))


def host_call(lib, model, root, dof, qdd, terms, with_qdd):
    K, n = qdd.shape
    root32 = np.ascontiguousarray(root, np.float32)
    tau = np.full((K, n), np.nan, np.float32)
    for k in range(K):
        q, qd, a = (np.ascontiguousarray(x) for x in (dof[k, 0::2], dof[k, 1::2], qdd[k]))
        assert lib.emu_inverse_dynamics(C.byref(model), fp(root32), fp(q), fp(qd), fp(a) if with_qdd else None, terms, fp(tau[k])) == 0
    assert np.isfinite(tau).all()
    return tau


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_function_on_the_host_meets_the_tolerance(robot, hostemu_id):
    tol = ic.tolerance(robot)
    for pose in ic.POSES[robot]:
        scene, model, root, parts, D, _ = ic.references(robot, pose)
        dof, qdd = ic.inputs(robot, pose)
        got = {call: host_call(hostemu_id, model, root, dof, qdd, *call) for call in ic.ALL_CALLS}
        e = {call: ic.e_tau(got[call], ic.combine(parts, *call), D) for call in ic.ALL_CALLS}
        print(f"\n[{robot} {pose}] host build, e_tau per (terms, qdd given) (tol {tol:.0e}): " + ", ".join(f"{c}: {v:.1e}" for c, v in e.items()))
        assert max(e.values()) <= tol
        assert not got[(0, False)].any()                               # nothing asked for: exact zeros
        # the partial calls sum to the full one
        parts_sum = got[(ic.ID_GRAVITY, False)].astype(np.float64) + got[(ic.ID_VELOCITY, False)] + got[(0, True)]
        assert ic.e_tau(parts_sum, got[ic.FULL].astype(np.float64), D) <= 2.0 * tol


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_gravity_off_in_the_model_is_exactly_zero(robot, hostemu_id):
    scene = ic.scene_of(robot, "tilted", gravity=False)
    model = scene.to_c()
    _, root = scene.initial_state()
    dof, qdd = ic.inputs(robot)
    assert not host_call(hostemu_id, model, root, dof, qdd, ic.ID_GRAVITY, False).any()
    assert not host_call(hostemu_id, model, root, dof, qdd, 0, False).any()
    # ... and the other parts are what they are with gravity on
    _, model_on, _, _, _, _ = ic.references(robot, "tilted")
    for call in ((ic.ID_VELOCITY, True), (ic.ID_VELOCITY, False), (0, True)):
        assert np.array_equal(host_call(hostemu_id, model, root, dof, qdd, *call), host_call(hostemu_id, model_on, root, dof, qdd, *call))
    assert np.array_equal(host_call(hostemu_id, model, root, dof, qdd, *ic.FULL), host_call(hostemu_id, model, root, dof, qdd, ic.ID_VELOCITY, True))


def test_host_build_refuses_a_moving_base_and_unknown_terms(hostemu_id):
    from scenes import boxer_push
    _, model, _, _, dof, root = boxer_push(K=8, H=2)
    out = np.zeros(64, np.float32)
    q, qd = np.ascontiguousarray(np.asarray(dof, np.float32)[0::2]), np.ascontiguousarray(np.asarray(dof, np.float32)[1::2])
    root32 = np.ascontiguousarray(root, np.float32)
    assert hostemu_id.emu_inverse_dynamics(C.byref(model), fp(root32), fp(q), fp(qd), fp(q), 3, fp(out)) == -2
    assert not out.any()
    scene, model, root, _, _, _ = ic.references("franka_panda")
    dof, qdd = ic.inputs("franka_panda")
    q, qd, a = (np.ascontiguousarray(x) for x in (dof[0, 0::2], dof[0, 1::2], qdd[0]))
    assert hostemu_id.emu_inverse_dynamics(C.byref(model), fp(np.ascontiguousarray(root, np.float32)), fp(q), fp(qd), fp(a), 4, fp(out)) == -4
    assert not out.any()


# ---- 4. a pass means something ------------------------------------------------------------------------------------------------------
# the velocity term of heijn (a planar base: x, y, yaw) is what a centre of mass 0.4 mm off the yaw axis makes of rates of 1 rad/s:
# 74 tolerances at the most, whatever the draw - it cannot reach the 100 asked of every part, and since that term is all that heijn's
# joint forces take from the rates, neither can a neighbour's rates (70).  Asserted there: 50.
PART_FLOOR = {("heijn", "C"): 50.0, ("heijn", "env k+1's qd"): 50.0, ("heijn", "env k-1's qd"): 50.0}


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_are_well_posed(robot, oracle64):
    """in tolerances: what SOME entry moves by (the worst entry over the robot's envs, joints and base poses) - and, printed next to
    it, what the least-moved env's worst entry moves by"""
    tol = ic.tolerance(robot)
    assert 0.0 < tol <= ic.CAP
    some = {}
    for pose in ic.POSES[robot]:
        scene, model, root, parts, D, w32 = ic.references(robot, pose)
        dof, qdd = ic.inputs(robot, pose)
        K, n = qdd.shape
        assert K == ic.ROBOTS[robot][3]
        full = ic.combine(parts, *ic.FULL)
        # the restatement, re-measured: the full call in fp32 (the cached figure is the worst over all calls)
        gb = ic.gravity_in_base(model, root)
        again = ic.e_tau(ic.restated(scene.robot_model, gb, dof, qdd, *ic.FULL), full, D)
        per_env = lambda other: (np.abs(other - full) / D[None, :]).max(1) / tol          # [K]: every env's worst entry, in tolerances
        moved = {f"without {p}": per_env(full - parts[p]) for p in ("M", "C", "g")}
        q, qd, a = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64), qdd.astype(np.float64)
        for name in ("q", "qd", "qdd"):          # env k +- 1's q, qd or qdd in place of env k's
            for shift in (1, -1):
                q2, qd2, a2 = (np.roll(x, shift, axis=0) if nm == name else x for nm, x in (("q", q), ("qd", qd), ("qdd", a)))
                moved[f"env k{shift:+d}'s {name}"] = per_env(ic.combine(ic.reference_parts(oracle64, model, root, q2, qd2, a2), *ic.FULL))
        M = jc.oracle_M(oracle64, model, root, q)
        for s in (1, -1):                        # a neighbouring joint's qdd
            moved[f"joint j{s:+d}'s qdd"] = per_env(full + np.einsum("kij,kj->ki", M, np.roll(a, s, axis=1) - a))
        near = min(float((np.abs(full[k] - full[k + 1]) / D).max()) for k in range(K - 1)) / tol
        print(f"\n[{robot} {pose}] K {K}: fp32 restatement e_tau {w32:.1e} over all calls, {again:.1e} full (tol {tol:.0e}); neighbouring envs differ by "
              f">= {near:.0f} tolerances; moved by, in tolerances (some entry / the least-moved env): "
              + ", ".join(f"{k} {v.max():.0f} / {v.min():.0f}" for k, v in moved.items()))
        assert again <= w32 <= 0.1 * tol
        assert near >= 100.0
        for k, v in moved.items():
            some[k] = max(some.get(k, 0.0), float(v.max()))
        if pose == "tilted":      # gravity along the BASE's axes instead of the world's
            wrong = ic.restated(scene.robot_model, np.array([model.gravity[j] for j in range(3)]), dof, qdd, ic.ID_GRAVITY, False, np.float64)
            off = float((np.abs(wrong - parts["g"]) / D[None, :]).max(1).min()) / tol
            print(f"[{robot} tilted] gravity along the base's axes: every env off by >= {off:.0f} tolerances")
            assert off >= 100.0
    for k, v in some.items():
        floor = PART_FLOOR.get((robot, k.replace("without ", "")), 100.0)
        assert v >= floor, f"{robot}: {k} moves no entry by {floor:.0f} tolerances ({v:.0f})"


def test_the_tilted_base_is_tilted():
    _, model, root, _, _, _ = ic.references("franka_panda", "tilted")
    R = ic.quat_to_R(np.asarray(root)[model.robot_actor, 3:7])
    cz, sz, cx, sx = np.cos(ic.TILT_YAW), np.sin(ic.TILT_YAW), np.cos(ic.TILT_ROLL), np.sin(ic.TILT_ROLL)
    want = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    assert np.abs(R - want).max() < 2e-7 and np.allclose(np.asarray(root)[model.robot_actor, 0:3], jc.OFFSET_POS)
    assert np.abs((R.T @ [0.0, 0.0, 1.0])[1:]).min() > 0.3      # rolled: gravity has a y and a z part in the base's axes
    dof, _ = ic.inputs("omnipanda", "far")
    assert (np.abs(dof[:, 0]) == ic.FAR).all() and (np.abs(dof[:, 2]) == ic.FAR).all()


# ---- 9., 10. the oracle side of the closed-loop rows --------------------------------------------------------------------------------
def test_the_arm_is_held_up_on_the_oracle_and_sags_without():
    scene, model, root, dof, g_ref, bound, sag, drift64, drift32 = ic.hold_case()
    assert model.drive_mode == capi.DRIVE_EFFORT and model.actors[model.robot_actor].gravity == 1
    print(f"\n[hold] K {len(dof)}, {ic.HOLD_STEPS} steps: fp64 oracle under g_ref drifts {drift64:.1e}, fp32 oracle {drift32:.1e} -> bound {bound:.0e}; "
          f"under a zero command the envs sag by {sag.min():.2e} .. {sag.max():.2e} rad")
    assert drift64 <= 1e-9                         # the reference stays at rest
    assert 0.0 < bound <= 1e-3
    assert sag.min() > 100.0 * bound               # every env: the row cannot pass without the gravity term


def test_computed_torque_identity_on_the_oracle():
    scene, model, root, dof, qdd, tau_ref, cmd, after = ic.torque_case()
    assert model.substeps == 1 and model.drive_mode == capi.DRIVE_EFFORT
    kd, h = float(model.drive_kd), float(model.dt)
    assert kd > 0.0
    q, qd = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64)
    err = np.abs(after[:, 1::2] - qd - h * qdd.astype(np.float64)).max()
    bodies = scene.robot_model["bodies"]
    effort = np.array([b["effort"] for b in bodies])
    vmax = np.array([b["velocity"] for b in bodies])
    lo, hi = np.array([b["lower"] for b in bodies]), np.array([b["upper"] for b in bodies])
    assert np.allclose([model.bodies[i].effort for i in range(len(bodies))], effort) and (effort > 0.0).all()
    load = (np.abs(tau_ref) / effort[None, :]).max()
    rate = (np.abs(after[:, 1::2]) / vmax[None, :]).max()
    reach = h * np.abs(after[:, 1::2])
    room = np.minimum(after[:, 0::2] - lo[None, :], hi[None, :] - after[:, 0::2]) - reach
    print(f"\n[computed torque] qd' - qd - h qdd on the oracle {err:.1e} (1e-9); |tau_ref| / effort limit {load:.2f} (0.9), |qd'| / rate limit {rate:.2f}, "
          f"least room to a joint limit beyond one step {room.min():.3f} rad")
    assert err <= 1e-9
    assert load <= 0.9 and rate < 1.0 and room.min() > 0.0
    assert np.abs(after[:, 0::2] - q - h * after[:, 1::2]).max() <= 1e-12
