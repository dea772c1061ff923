"""The no-GPU half of the link-Jacobian / mass-matrix tests (inputs, references and tolerances: jacobian_cases.py; the kernels on
the GPU: test_gpu_jacobian_mass.py).

 * both entries are exported by the cross-compiled libmppi_hip.so and declared by the binding; the wrapper has the accessors;
 * the inputs are well posed, on the oracle alone: everything finite, the fp32 oracle's route within a TENTH of each tolerance,
   neighbouring envs more than 100 tolerances apart in both tensors (an index mix-up cannot pass); the numbers are printed;
 * the DEFINITION of J is the oracle's: J_ref qd reproduces the rigid-body velocity columns for a full joint-rate vector (they
   are linear in qd), and the linear rows are the central difference of the rigid-body positions.
   Finite-difference bound: step 1e-4 rad (m) per joint -> truncation h^2 / 6 x |third derivative| <= 1.7e-9 x 3 m of lever, rounding
   2^-53 x 400 m / 2e-4 = 2e-10 (the mobile manipulator's fixture carries the arm 394 m from the origin): asserted at 5e-8;
 * the device functions link_jacobian / mass_matrix (csrc/mppi_device.hpp) themselves, compiled for the host, meet the GPU half's
   tolerances against the same references, base at the origin and away from it, with M == M^T bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jacobian_cases as jc
from mppiisaac.backend import capi

ROBOT_IDS = list(jc.ROBOTS)


def test_both_entries_are_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_jacobian"] == (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p])
    assert capi._SIGNATURES["mppi_sim_mass_matrix"] == (C.c_int, [C.c_void_p, C.c_void_p])
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    for name in ("mppi_sim_jacobian", "mppi_sim_mass_matrix"):
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mppi_hip.h")).read()
    for name, replaces in (("mppi_sim_jacobian", "gym.acquire_jacobian_tensor"), ("mppi_sim_mass_matrix", "gym.acquire_mass_matrix_tensor")):
        assert f"int {name}(" in header and replaces in header
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("acquire_jacobian_tensor", "acquire_mass_matrix_tensor", "refresh_jacobian_tensors", "refresh_mass_matrix_tensors",
                 "get_actor_link_jacobian_by_name"):
        assert callable(getattr(IsaacGymWrapper, name))


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_are_well_posed(robot):
    for offset in (False, True) if robot == "franka_panda" else (False,):
        scene, model, root, J_ref, M_ref, w32_J, w32_M = jc.references(robot, offset)
        tol_J, tol_M = jc.tolerances(robot)
        K = len(J_ref)
        assert K == jc.ROBOTS[robot][3] and J_ref.shape == (K, model.n_rb, 6, scene.n_dof) and M_ref.shape == (K, scene.n_dof, scene.n_dof)
        assert np.isfinite(J_ref).all() and np.isfinite(M_ref).all()
        assert 0.0 < tol_J <= jc.CAP and 0.0 < tol_M <= jc.CAP
        near_J = min(jc.e_J(J_ref[k:k + 1], J_ref[k + 1:k + 2]) for k in range(K - 1))
        near_M = min(jc.e_M(M_ref[k:k + 1], M_ref[k + 1:k + 2]) for k in range(K - 1))
        print(f"\n[{robot}{' offset' if offset else ''}] K {K}: fp32 route e_J {w32_J:.1e} (tol {tol_J:.0e}) e_M {w32_M:.1e} (tol {tol_M:.0e}); "
              f"nearest neighbours {near_J / tol_J:.0f} tol(J), {near_M / tol_M:.0f} tol(M)")
        assert w32_J <= 0.1 * tol_J and w32_M <= 0.1 * tol_M
        assert near_J > 100.0 * tol_J and near_M > 100.0 * tol_M
        for k in range(K):      # what the GPU half asserts of every M holds of the reference
            assert np.abs(M_ref[k] - M_ref[k].T).max() <= 1e-9 * np.abs(M_ref[k]).max()
            np.linalg.cholesky(M_ref[k])


def test_the_offset_root_moves_the_panda():
    """the base pose of the `away from the origin` row differs: the rigid-body positions move by the offset, the Jacobians turn"""
    _, _, root0, J0, M0, _, _ = jc.references("franka_panda")
    _, _, root1, J1, M1, _, _ = jc.references("franka_panda", True)
    assert np.allclose(root1[0, 0:3] - root0[0, 0:3], jc.OFFSET_POS) and np.allclose(root1[0, 3:7], jc.OFFSET_ORI)
    assert jc.e_J(J1, J0) > 0.1               # (yawed by 0.7 rad: the columns turn with the base)
    assert jc.e_M(M1[3:], M0[3:]) < 1e-9      # ... and the mass matrix does not care where the base stands


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_the_jacobian_is_the_oracles(robot, oracle64):
    scene, model, root, J_ref, _, _, _ = jc.references(robot)
    dof, _ = jc.inputs(robot)
    n = scene.n_dof
    h = 1e-4
    worst_lin, worst_fd = 0.0, 0.0
    for k in range(8):
        q, qd = dof[k, 0::2].astype(np.float64), dof[k, 1::2].astype(np.float64)
        rb = oracle64.rigid_body_state(model, root, q, qd)[0]
        worst_lin = max(worst_lin, np.abs(J_ref[k] @ qd - rb[:, 7:13]).max() / max(1.0, np.abs(rb[:, 7:13]).max()))
        for i in range(n):
            e = np.eye(n)[i] * h
            fd = (oracle64.rigid_body_state(model, root, q + e, qd)[0][:, 0:3] - oracle64.rigid_body_state(model, root, q - e, qd)[0][:, 0:3]) / (2 * h)
            worst_fd = max(worst_fd, np.abs(J_ref[k, :, 0:3, i] - fd).max())
    print(f"\n[{robot}] J_ref qd against the rb velocity columns {worst_lin:.1e}, linear rows against the central difference {worst_fd:.1e}")
    assert worst_lin < 1e-13 and worst_fd < 5e-8
    # zero blocks: links welded to the fixed base (the root link among them) do not move
    fixed = [l for l, link in enumerate(scene.robot_model["links"]) if link["body"] < 0]
    assert 0 in fixed and not J_ref[:, [scene.first_rb[scene.robot_idx] + l for l in fixed]].any()


@pytest.fixture(scope="module")
def hostemu_jacobian():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostemu_jacobian")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libjacobian_hostemu.so"))


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_functions_on_the_host_meet_the_tolerances(robot, hostemu_jacobian):
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    tol_J, tol_M = jc.tolerances(robot)
    dof, _ = jc.inputs(robot)
    for offset in (False, True) if robot == "franka_panda" else (False,):
        scene, model, root, J_ref, M_ref, _, _ = jc.references(robot, offset)
        K, n = len(J_ref), scene.n_dof
        J, M = np.zeros((K, model.n_rb, 6, n), np.float32), np.zeros((K, n, n), np.float32)
        root32 = np.ascontiguousarray(root, np.float32)
        for k in range(K):
            q = np.ascontiguousarray(dof[k, 0::2])
            assert hostemu_jacobian.emu_jacobian(C.byref(model), fp(root32), fp(q), fp(J[k])) == 0
            assert hostemu_jacobian.emu_mass_matrix(C.byref(model), fp(root32), fp(q), fp(M[k])) == 0
        eJ, eM = jc.e_J(J, J_ref), jc.e_M(M, M_ref)
        print(f"\n[{robot}{' offset' if offset else ''}] host build: e_J {eJ:.1e} (tol {tol_J:.0e}), e_M {eM:.1e} (tol {tol_M:.0e})")
        assert eJ <= tol_J and eM <= tol_M
        assert (M == M.transpose(0, 2, 1)).all()
        for k in range(K):
            np.linalg.cholesky(M[k].astype(np.float64))


def test_host_build_refuses_a_moving_base(hostemu_jacobian):
    from scenes import boxer_push
    _, model, _, _, dof, root = boxer_push(K=8, H=2)
    out = np.zeros(4096, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    q = np.ascontiguousarray(np.asarray(dof, np.float32)[0::2])
    assert hostemu_jacobian.emu_jacobian(C.byref(model), fp(np.asarray(root, np.float32)), fp(q), fp(out)) == -2
    assert not out.any()
