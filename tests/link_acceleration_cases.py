"""Inputs, references, metrics and tolerances of the link-acceleration / wrench-force tests (test_link_acceleration.py, no GPU;
test_gpu_link_acceleration.py): mppi_sim_link_acceleration and mppi_sim_wrench_forces (csrc/mppi_kernels.hpp k_sim_link_acceleration,
k_sim_wrench_forces; csrc/mppi_device.hpp link_accelerations, link_acceleration, gather_link_wrench, wrench_joint_forces) against the
fp64 oracle, every env, every rigid body, every entry.

INPUTS per robot: those of inverse_dynamics_cases.inputs(robot, pose) - the robots of jacobian_cases.ROBOTS, the base poses `origin`,
`tilted` and, for the mobile manipulator, `far` (its prismatic base joints +-420 m out), joint rates +-1 and accelerations +-3 - and
wrenches from default_rng(SEED = 22): forces uniform in +-10 N and moments uniform in +-1 N m on every rigid body.  An env's inputs
do not depend on how many envs there are.
REFERENCES, always fp64, from the oracle as it stands:
  a_ref   = J_ref qdd + (Jdot qd)_ref,  J_ref = jacobian_cases.oracle_J(Oracle("f64"), ...);  (Jdot qd)_ref the Richardson-extrapolated
            central difference of the oracle's rigid-body velocity columns along the motion:  c(h) = [v(q + h qd, qd) - v(q - h qd, qd)] / 2h
            with v = rigid_body_state(...)[0][:, 7:13],  (Jdot qd)_ref = (4 c(h) - c(2h)) / 3,  h = 1e-3.  The same value one level up,
            (4 c(2h) - c(4h)) / 3, must agree with it within RICHARDSON_AGREE = 1e-8 on every input (asserted where it is computed).
  tau_ref = sum_b J_ref,b^T w_b.
METRICS  e_lin = max |a - a_ref|[k, b, 0:3] / D_lin, D_lin the largest |a_ref| linear entry of the FULL call (qdd given, velocity on) over
the robot's inputs at that pose; e_ang the same for rows 3-5; calls with fewer parts are measured against the same D.
e_tau = max |tau - tau_ref|[k, j] / D_j, D_j = max_k |tau_ref[k, j]|, as in the inverse-dynamics tests.  Rows that the reference has
exactly zero (links welded to the fixed base, bodies of box or sphere actors) must be exact zeros.
TOLERANCES, per robot and metric, by the project's rule: 10 x the worst deviation from the reference of an fp32 RESTATEMENT - over the
robot's base poses and calls -, rounded up to 1-2-5, at most CAP = 1e-4 (the cap of the inverse-dynamics tests).  The restatement
(body_frame_accelerations, body_frame_wrench_forces) is a body-frame 3-vector pass over the robot's JSON model in numpy float32 on
fp32-rounded inputs, in the style of inverse_dynamics_cases.newton_euler - deliberately not the kernel's world-axes formulation, and
never the code under test."""
import functools
from types import SimpleNamespace

import numpy as np

import inverse_dynamics_cases as ic
import jacobian_cases as jc
from test_gpu_step_matrix import round_up_125

SEED = 22
FORCE_AMP, MOMENT_AMP = 10.0, 1.0
H_STEP = 1e-3
RICHARDSON_AGREE = 1e-8
CAP = ic.CAP
ID_GRAVITY, ID_VELOCITY = ic.ID_GRAVITY, ic.ID_VELOCITY
# (terms, qdd given): the full call, Jdot qd alone, J qdd alone, nothing
FULL = (ID_VELOCITY, True)
ACC_CALLS = [FULL, (ID_VELOCITY, False), (0, True), (0, False)]
ROBOTS = jc.ROBOTS
STORE_EDGES = jc.STORE_EDGES
POSES = ic.POSES


def scene_of(robot, pose="origin"):
    return ic.scene_of(robot, pose)


@functools.lru_cache(maxsize=None)
def wrenches(kmax, n_rb):
    """[kmax][n_rb][6] fp32, read-only: (force, moment) on every rigid body of every env"""
    w = np.random.default_rng(SEED).uniform(-1.0, 1.0, size=(kmax, n_rb, 6)) * np.array([FORCE_AMP] * 3 + [MOMENT_AMP] * 3)
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def inputs(robot, pose="origin"):
    """-> (dof [KMAX][2n] fp32 interleaved q, qd; qdd [KMAX][n] fp32; wrenches [KMAX][n_rb][6] fp32 of the robot's own scene), read-only"""
    dof, qdd = ic.inputs(robot, pose)
    return dof, qdd, wrenches(len(dof), int(scene_of(robot, pose).to_c().n_rb))


# ---- the references -----------------------------------------------------------------------------------------------------------------
def velocity_columns(o64, model, root, q, qd):
    return o64.rigid_body_state(model, root, q, qd)[0][:, 7:13].astype(np.float64)


def oracle_Jdot_qd(o64, model, root, q, qd, h=H_STEP):
    """-> ((Jdot qd)_ref [K][n_rb][6], the largest difference from the same extrapolation one level up) in fp64"""
    q, qd = np.asarray(q, np.float64), np.asarray(qd, np.float64)
    out = np.zeros((len(q), model.n_rb, 6))
    gap = 0.0
    for k in range(len(q)):
        c = [(velocity_columns(o64, model, root, q[k] + s * qd[k], qd[k]) - velocity_columns(o64, model, root, q[k] - s * qd[k], qd[k])) / (2.0 * s)
             for s in (h, 2.0 * h, 4.0 * h)]
        out[k] = (4.0 * c[0] - c[1]) / 3.0
        gap = max(gap, float(np.abs(out[k] - (4.0 * c[1] - c[2]) / 3.0).max()))
    return out, gap


def reference_parts(o64, model, root, q, qd, qdd):
    """-> (J_ref [K][n_rb][6][n], {'A': J qdd, 'V': Jdot qd} each [K][n_rb][6]) in fp64; asserts the agreement of the two Richardson levels"""
    q, qd, qdd = (np.asarray(a, np.float64) for a in (q, qd, qdd))
    J = jc.oracle_J(o64, model, root, q)
    V, gap = oracle_Jdot_qd(o64, model, root, q, qd)
    assert gap <= RICHARDSON_AGREE, f"the two Richardson levels of (Jdot qd)_ref differ by {gap:.2e}"
    return J, {"A": np.einsum("kbri,ki->kbr", J, qdd), "V": V, "gap": gap}


def combine(parts, terms, with_qdd):
    out = np.zeros_like(parts["V"])
    if with_qdd:
        out = out + parts["A"]
    if terms & ID_VELOCITY:
        out = out + parts["V"]
    return out


def wrench_reference(J, w):
    """tau_ref [K][n] = sum_b J_b^T w_b in fp64"""
    return np.einsum("kbri,kbr->ki", J, np.asarray(w, np.float64))


def scales(parts):
    """(D_lin, D_ang) of the full call's reference"""
    full = np.abs(combine(parts, *FULL))
    return float(full[:, :, 0:3].max()), float(full[:, :, 3:6].max())


def e_acc(a, a_ref, D):
    """-> (e_lin, e_ang)"""
    d = np.abs(np.asarray(a, np.float64) - a_ref)
    return float(d[:, :, 0:3].max() / D[0]), float(d[:, :, 3:6].max() / D[1])


def e_tau(tau, tau_ref, Dj):
    return float((np.abs(np.asarray(tau, np.float64) - tau_ref) / Dj[None, :]).max())


def zero_bodies(J):
    """[n_rb] bool: the bodies whose reference Jacobian is exactly zero in every env"""
    return ~np.abs(J).max((0, 2, 3)).astype(bool)


# ---- the fp32 restatement -----------------------------------------------------------------------------------------------------------
def _body_frames(model_json, R_base, q, f):
    """joint rotations R[i] (child in parent), offsets p[i] (in the parent's frame) and world rotations Rw[i] of every body in precision f"""
    bodies = model_json["bodies"]
    n = len(bodies)
    R, p, Rw = [None] * n, [None] * n, [None] * n
    for i, b in enumerate(bodies):
        ax, Rt, pt = np.asarray(b["axis"], f), np.asarray(b["R_tree"], f), np.asarray(b["p_tree"], f)
        R[i], p[i] = (Rt @ ic._rot_axis(ax, q[i], f), pt) if b["jtype"] == "revolute" else (Rt, pt + (Rt @ ax) * q[i])
        Rw[i] = (np.asarray(R_base, f) if b["parent"] < 0 else Rw[b["parent"]]) @ R[i]
    return R, p, Rw


def body_frame_accelerations(model_json, R_base, q, qd, qdd, f=np.float32):
    """[L][6] of every link of the model: the outward half of the classic body-frame Newton-Euler recursion (Luh-Walker-Paul) without
    gravity, every operation in precision f on inputs rounded to f; a link's row is turned into world axes at the very end"""
    bodies, links = model_json["bodies"], model_json["links"]
    n = len(bodies)
    q, qd, qdd = (np.asarray(a, f) for a in (q, qd, qdd))
    R, p, Rw = _body_frames(model_json, R_base, q, f)
    w, wd, a = [None] * n, [None] * n, [None] * n
    zero = np.zeros(3, f)
    for i, b in enumerate(bodies):
        ax, par = np.asarray(b["axis"], f), b["parent"]
        wp, wdp, ap = (zero, zero, zero) if par < 0 else (w[par], wd[par], a[par])
        E = R[i].T
        carried = E @ (ap + np.cross(wdp, p[i]) + np.cross(wp, np.cross(wp, p[i])))
        if b["jtype"] == "revolute":
            w[i] = E @ wp + ax * qd[i]
            wd[i] = E @ wdp + ax * qdd[i] + np.cross(E @ wp, ax * qd[i])
            a[i] = carried
        else:
            w[i], wd[i] = E @ wp, E @ wdp
            a[i] = carried + f(2) * np.cross(w[i], ax * qd[i]) + ax * qdd[i]
        assert all(v.dtype == f for v in (R[i], p[i], Rw[i], w[i], wd[i], a[i]))
    out = np.zeros((len(links), 6), f)
    for l, L in enumerate(links):
        i = L["body"]
        if i < 0:
            continue
        r = np.asarray(L["p"], f)
        out[l, 0:3] = Rw[i] @ (a[i] + np.cross(wd[i], r) + np.cross(w[i], np.cross(w[i], r)))
        out[l, 3:6] = Rw[i] @ wd[i]
    return out


def body_frame_wrench_forces(model_json, R_base, q, w, f=np.float32):
    """tau [n] of the wrenches w [L][6] (world axes, about the link frame origins) on the model's links: each wrench turned into its body's
    frame and moved to the body's origin, then the inward half of the body-frame recursion, every operation in precision f"""
    bodies, links = model_json["bodies"], model_json["links"]
    n = len(bodies)
    q, w = np.asarray(q, f), np.asarray(w, f)
    R, p, Rw = _body_frames(model_json, R_base, q, f)
    F, N = [np.zeros(3, f) for _ in range(n)], [np.zeros(3, f) for _ in range(n)]
    for l, L in enumerate(links):
        i = L["body"]
        if i < 0:
            continue
        fb = Rw[i].T @ w[l, 0:3]
        F[i] = F[i] + fb
        N[i] = N[i] + Rw[i].T @ w[l, 3:6] + np.cross(np.asarray(L["p"], f), fb)
    tau = np.zeros(n, f)
    for i in reversed(range(n)):
        b = bodies[i]
        tau[i] = (N[i] if b["jtype"] == "revolute" else F[i]) @ np.asarray(b["axis"], f)
        if b["parent"] >= 0:
            fp = R[i] @ F[i]
            F[b["parent"]] = F[b["parent"]] + fp
            N[b["parent"]] = N[b["parent"]] + R[i] @ N[i] + np.cross(p[i], fp)
        assert F[i].dtype == f and N[i].dtype == f
    return tau


def base_rotation(model, root):
    return ic.quat_to_R(np.asarray(root, np.float64).reshape(-1, 13)[model.robot_actor, 3:7])


def restated_acc(model_json, R_base, dof, qdd, terms, with_qdd, f=np.float32):
    """[K][L][6]: body_frame_accelerations of every env for one call (a part that is not asked for has its input zeroed)"""
    q, qd = dof[:, 0::2], dof[:, 1::2]
    zero = np.zeros(q.shape[1])
    return np.stack([body_frame_accelerations(model_json, R_base, q[k], qd[k] if terms & ID_VELOCITY else zero, qdd[k] if with_qdd else zero, f)
                     for k in range(len(q))])


def restated_tau(model_json, R_base, dof, w, f=np.float32):
    return np.stack([body_frame_wrench_forces(model_json, R_base, dof[k, 0::2], w[k], f) for k in range(len(dof))])


# ---- references and tolerances ------------------------------------------------------------------------------------------------------
def references_of(scene, dof, qdd, w):
    """the references and the restatement's worst deviations of a robot-only scene at the given inputs -> a namespace: scene, model, root,
    J, parts, D (D_lin, D_ang), tau_ref, Dj, zero (bodies with an exactly zero reference), w32 (worst restatement e_lin, e_ang, e_tau)"""
    from oracle.oracle import Oracle
    o64 = Oracle("f64")
    model = scene.to_c()
    _, root = scene.initial_state()
    first, L = int(model.actors[model.robot_actor].first_rb), len(scene.robot_model["links"])
    J, parts = reference_parts(o64, model, root, dof[:, 0::2], dof[:, 1::2], qdd)
    tau_ref = wrench_reference(J, w)
    D, Dj = scales(parts), np.abs(tau_ref).max(0)
    Rb = base_rotation(model, root)
    worst = [0.0, 0.0, 0.0]
    for call in ACC_CALLS:
        r = restated_acc(scene.robot_model, Rb, dof, qdd, *call)
        el, ea = e_acc(r, combine(parts, *call)[:, first:first + L], D)
        worst[0], worst[1] = max(worst[0], el), max(worst[1], ea)
    worst[2] = e_tau(restated_tau(scene.robot_model, Rb, dof, w[:, first:first + L]), wrench_reference(J[:, first:first + L], w[:, first:first + L]), Dj)
    for a in (J, parts["A"], parts["V"], tau_ref):
        a.setflags(write=False)
    return SimpleNamespace(scene=scene, model=model, root=root, J=J, parts=parts, D=D, tau_ref=tau_ref, Dj=Dj, zero=zero_bodies(J), w32=tuple(worst),
                           first=first, L=L)


@functools.lru_cache(maxsize=None)
def references(robot, pose="origin"):
    return references_of(scene_of(robot, pose), *inputs(robot, pose))


@functools.lru_cache(maxsize=None)
def restatement_worst(robot):
    """worst fp32-restatement deviation (e_lin, e_ang, e_tau) over the robot's base poses and calls"""
    runs = [references(robot, pose).w32 for pose in POSES[robot]]
    return tuple(max(r[j] for r in runs) for j in range(3))


def tolerances_from(worst):
    return tuple(min(round_up_125(10.0 * x), CAP) for x in worst)


def tolerances(robot):
    """-> (tol_lin, tol_ang, tol_tau)"""
    return tolerances_from(restatement_worst(robot))
