"""Inputs, references, metrics and tolerances of the forward-dynamics tests (test_forward_dynamics.py, no GPU;
test_gpu_forward_dynamics.py): mppi_sim_forward_dynamics (csrc/mppi_kernels.hpp k_sim_forward_dynamics, csrc/mppi_device.hpp
forward_dynamics) against the fp64 oracle, every env, every joint, every combination of terms.

INPUTS per robot: the robots, base poses and envs of inverse_dynamics_cases (ROBOTS, POSES, STORE_EDGES), its joint positions, its
rates (+-1) and its accelerations qdd* (+-3), gravity on.  tau is the fp64 tau_ref of those qdd* (reference_parts / combine there),
rounded to fp32 - so qdd_ref is O(1) in every joint (D_j = 2.7 to 3.0 for every robot).  An env's inputs do not depend on how many
envs there are.
REFERENCE, always fp64, from the oracle as it stands:  Oracle("f64").forward_dynamics(model, root, q, qd, tau_fp32); the parts
come with qd = 0 (no velocity part) and / or gravity off on the scene (no gravity part), tau = 0 when tau is left out.
METRICS - forward dynamics amplifies by cond(M) (1e4 on the arms), so two:
  (a) e_qdd = max |qdd - qdd_ref|[k, j] / D_j,  D_j = max_k |qdd_ref[k, j]| of the FULL call;
  (b) e_res = max |M_ref (qdd - qdd_ref)|[k, j] / Dtau_j, the torque-space residual: M_ref = jacobian_cases.oracle_M, Dtau_j the
      torque scale of inverse_dynamics_cases.  The backward error: it does not grow with the conditioning, and a wrong shift
      formula shows there first.
Calls with fewer terms are measured against the same D_j / Dtau_j.
TOLERANCES, per robot and metric, by the project's rule: 10 x the worst deviation of Oracle("f32").forward_dynamics from qdd_ref -
over the robot's base poses and the eight (terms, tau given or left out) combinations -, rounded up to 1-2-5; at most CAP_QDD =
1e-3 for (a): a pass means three digits (rounding tau to fp32 alone moves qdd by 2.4e-5 on the Panda); at most the CAP of
inverse_dynamics_cases for (b)."""
import functools

import numpy as np

import inverse_dynamics_cases as ic
import jacobian_cases as jc
from test_gpu_step_matrix import round_up_125

CAP_QDD = 1e-3
CAP_RES = ic.CAP
ID_GRAVITY, ID_VELOCITY = ic.ID_GRAVITY, ic.ID_VELOCITY
# (terms, tau given): the full call, tau NULL with both terms, gravity only, velocity only, tau only; then the remaining combinations
FULL = ic.FULL
CALLS = ic.CALLS
ALL_CALLS = ic.ALL_CALLS
ROBOTS = ic.ROBOTS
STORE_EDGES = ic.STORE_EDGES
POSES = ic.POSES


@functools.lru_cache(maxsize=None)
def inputs(robot, pose="origin"):
    """-> (dof [KMAX][2n] fp32 interleaved q, qd; tau [KMAX][n] fp32: the joint forces of inverse_dynamics_cases' qdd*), read-only"""
    dof, _ = ic.inputs(robot, pose)
    parts = ic.references(robot, pose)[3]
    tau = ic.combine(parts, *ic.FULL).astype(np.float32)
    tau.setflags(write=False)
    return dof, tau


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def oracle_qdd(o, model_on, model_off, root, q, qd, tau, terms, with_tau):
    """[K][n] in fp64 from the oracle of either precision for one call: a part that is not asked for has its input zeroed (qd = 0,
    the scene's gravity off, tau = 0)"""
    K, n = q.shape
    zero = np.zeros(n)
    model = model_on if terms & ID_GRAVITY else model_off
    return np.stack([o.forward_dynamics(model, root, q[k], qd[k] if terms & ID_VELOCITY else zero, tau[k] if with_tau else zero).astype(np.float64)
                     for k in range(K)])


def reference_calls(o, model_on, model_off, root, q, qd, tau, calls=ALL_CALLS):
    return {call: oracle_qdd(o, model_on, model_off, root, np.asarray(q, np.float64), np.asarray(qd, np.float64), np.asarray(tau, np.float64), *call)
            for call in calls}


def scale(ref):
    """D_j: the per-joint acceleration scale of the full call's reference"""
    return np.abs(ref[FULL]).max(0)


def e_qdd(qdd, qdd_ref, D):
    return float((np.abs(np.asarray(qdd, np.float64) - qdd_ref) / D[None, :]).max())


def e_res(qdd, qdd_ref, M_ref, Dtau):
    r = np.einsum("kij,kj->ki", M_ref, np.asarray(qdd, np.float64) - qdd_ref)
    return float((np.abs(r) / Dtau[None, :]).max())


def models_of(robot, pose="origin"):
    """the robot's scene with gravity on and off -> (scene, model_on, model_off, root)"""
    scene = ic.scene_of(robot, pose)
    _, root = scene.initial_state()
    return scene, scene.to_c(), ic.scene_of(robot, pose, gravity=False).to_c(), root


# ---- references and tolerances ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def references(robot, pose="origin"):
    """-> (scene, model, model with gravity off, root, qdd_ref {call: [K][n]}, D, M_ref, Dtau, worst fp32-oracle e_qdd over ALL_CALLS,
    worst fp32-oracle e_res over ALL_CALLS, fp32-oracle e_qdd of the full call) at the robot's inputs and base pose"""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    scene, model, model_off, root = models_of(robot, pose)
    dof, tau = inputs(robot, pose)
    q, qd = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64)
    ref = reference_calls(o64, model, model_off, root, q, qd, tau)
    M_ref = jc.oracle_M(o64, model, root, q)
    Dtau = ic.references(robot, pose)[4]
    D = scale(ref)
    for a in list(ref.values()) + [M_ref]:
        a.setflags(write=False)
    r32 = reference_calls(o32, model, model_off, root, q, qd, tau)
    wq = max(e_qdd(r32[c], ref[c], D) for c in ALL_CALLS)
    wr = max(e_res(r32[c], ref[c], M_ref, Dtau) for c in ALL_CALLS)
    return scene, model, model_off, root, ref, D, M_ref, Dtau, wq, wr, e_qdd(r32[FULL], ref[FULL], D)


@functools.lru_cache(maxsize=None)
def oracle32_worst(robot):
    """worst fp32-oracle deviation (e_qdd, e_res) over the robot's base poses and all calls"""
    runs = [references(robot, pose) for pose in POSES[robot]]
    return max(r[8] for r in runs), max(r[9] for r in runs)


def tolerances_from(worst_qdd, worst_res):
    return min(round_up_125(10.0 * worst_qdd), CAP_QDD), min(round_up_125(10.0 * worst_res), CAP_RES)


def tolerances(robot):
    """-> (tol_qdd, tol_res)"""
    return tolerances_from(*oracle32_worst(robot))


def measure(got, ref, D, M_ref, Dtau):
    """{call: (e_qdd, e_res)} of the results `got` {call: [K][n]}"""
    return {c: (e_qdd(got[c], ref[c], D), e_res(got[c], ref[c], M_ref, Dtau)) for c in got}


# ---- M^-1 (inverse_mass_matrix) -----------------------------------------------------------------------------------------------------
def oracle_Minv(o, model_off, root, q):
    """[K][n][n] in fp64 from the oracle of either precision: column i = forward dynamics of the unit torque e_i at qd = 0, gravity off"""
    K, n = q.shape
    zero, eye = np.zeros(n), np.eye(n)
    return np.stack([np.stack([o.forward_dynamics(model_off, root, q[k], zero, eye[i]).astype(np.float64) for i in range(n)], axis=1) for k in range(K)])


def e_X(X, X_ref):
    """max |X - X_ref|_ij / sqrt(X_ref,ii X_ref,jj)"""
    s = np.sqrt(np.einsum("kii->ki", X_ref))
    return float((np.abs(np.asarray(X, np.float64) - X_ref) / (s[:, :, None] * s[:, None, :])).max())


@functools.lru_cache(maxsize=None)
def Minv_reference(robot, K):
    """-> (X_ref [K][n][n], tolerance: 10 x the fp32 oracle's e_X rounded up to 1-2-5, at most CAP_QDD, the fp32 oracle's e_X)"""
    from oracle.oracle import Oracle
    _, _, model_off, root = models_of(robot)
    q = inputs(robot)[0][:K, 0::2].astype(np.float64)
    X_ref = oracle_Minv(Oracle("f64"), model_off, root, q)
    X_ref.setflags(write=False)
    w32 = e_X(oracle_Minv(Oracle("f32"), model_off, root, q), X_ref)
    return X_ref, min(round_up_125(10.0 * w32), CAP_QDD), w32
