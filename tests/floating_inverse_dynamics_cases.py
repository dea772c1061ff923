"""Inputs, references, metric and tolerances of the moving-base inverse-dynamics tests (test_floating_inverse_dynamics.py, no GPU;
test_gpu_floating_inverse_dynamics.py): mppi_sim_floating_inverse_dynamics (csrc/mppi_kernels.hpp k_sim_floating_inverse_dynamics,
csrc/mppi_device.hpp floating_inverse_dynamics) against an fp64 reference built from what the oracle exports, every env, every row,
every combination of terms.

GENERALISED VELOCITY  v = (root linvel, root angvel, qd) of floating_jacobian_cases; vd its time derivative (the acceleration of the
root frame origin, the angular acceleration, qdd); tau the force dual to v: rows 0:3 the force on the base (N), rows 3:6 the moment
about the base origin (N m), world axes, then the joints (N for a prismatic joint, N m for a revolute one).
REFERENCE, always fp64, at the state the simulator holds, per env the sum over the BODY frames (floating_jacobian_cases.
body_frame_model: the n_bodies body frames and the base frame):
    tau_ref = sum_i J_i^T ( I6_i (J_i vd + (Jdot_i v) - (g, 0)) + (w_i x (w_i x h_w), w_i x (I_o w_i)) )
  J_i      floating_jacobian_cases.oracle_J of the body-frame model;
  I6_i     [[m 1, -[h_w]x], [[h_w]x, R Io R^T]], the block of floating_jacobian_cases.congruence_M;
  w_i      columns 10:13 of the oracle's rigid-body row at the env's own twist and rates;
  Jdot_i v the Richardson-extrapolated central difference (h = 1e-3, two levels, as link_acceleration_cases.oracle_Jdot_qd) of the
           oracle's velocity columns along the flow of constant v: q +- s qd, the base position +- s v_lin, the base quaternion
           exp(+- s w / 2) (x) quat.  The two levels must agree within link_acceleration_cases.RICHARDSON_AGREE.
  The three parts are kept apart: 'M' = sum J^T I6 J vd, 'C' = sum J^T (I6 Jdot v + velocity products), 'g' = -sum J^T I6 (g, 0).
  On fixed-base robots the same route (fixed_parts) reproduces inverse_dynamics_cases.reference_parts - asserted in the no-GPU half
  before anything else, with the power balance v^T (C v) = v^T Mdot v / 2 and the Richardson agreement.
INPUTS per robot: the robots, env counts, joint positions and base poses of floating_jacobian_cases.inputs; the robot's gravity on;
fresh rates from default_rng(SEED): qd uniform +-1, base twist +-1 m/s and +-1 rad/s, vd uniform +-3 (at +-0.1 the velocity part
is too small to tell apart: 27 N against 2685 N of weight for boxer), all rounded to fp32 before the references are taken.  An env's
inputs do not depend on how many envs there are.
METRIC  e = max |tau - ref|[k, j] / D_j with D_j = max_k |ref[k, j]| OF THE CALL'S OWN reference over the robot's envs (each part on
its own scale - the weight would swamp C v in the base-force rows -, the full call as the sum against the sum's D), floored at
FLOOR = 1e-3 of the largest D among rows of the same unit (balanced wheels and the x / y rows of the weight have a zero reference).
A call whose reference is zero everywhere (terms = 0 without vd) must give exact zeros.
TOLERANCE, per robot, by the project's rule: 10 x the worst e of an fp32 RESTATEMENT from the reference over the eight call
combinations, rounded up to 1-2-5, at most CAP = 1e-4.  The restatement (floating_newton_euler) is a body-frame Luh-Walker-Paul
recursion with a moving root in np.float32 on fp32-rounded inputs - deliberately not the kernel's world-axes formulation, and never
the code under test."""
import functools
from types import SimpleNamespace

import numpy as np

import floating_jacobian_cases as fc
import inverse_dynamics_cases as ic
import link_acceleration_cases as lc
from test_gpu_step_matrix import round_up_125

SEED = 24
QD_AMP, TWIST_AMP, VD_AMP = 1.0, 1.0, 3.0
CAP = 1e-4
FLOOR = 1e-3
H_STEP = lc.H_STEP
RICHARDSON_AGREE = lc.RICHARDSON_AGREE
ID_GRAVITY, ID_VELOCITY = ic.ID_GRAVITY, ic.ID_VELOCITY
FULL, CALLS, ALL_CALLS = ic.FULL, ic.CALLS, ic.ALL_CALLS
ROBOTS = fc.ROBOTS
STORE_EDGES = fc.STORE_EDGES
PUSH_SCENE = fc.PUSH_SCENE
FAR_SHIFT = fc.FAR_SHIFT
combine = ic.combine


def scene_of(robot):
    scene = fc.scene_of(robot)
    scene.robot.gravity = True
    return scene


def draw_rates(dof0, roots0, robot_actor, seed=SEED):
    """the poses of (dof0, roots0) with fresh rates -> (dof [K][2n], roots [K][A][13], vd [K][6 + n]) fp32; one row of draws per env"""
    K, n = dof0.shape[0], dof0.shape[1] // 2
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(K, 2 * n + 12))
    dof, roots = np.array(dof0, np.float32), np.array(roots0, np.float32)
    dof[:, 1::2] = QD_AMP * u[:, 0:n]
    roots[:, robot_actor, 7:13] = TWIST_AMP * u[:, n:n + 6]
    vd = (VD_AMP * u[:, n + 6:2 * n + 12]).astype(np.float32)
    return dof, roots, vd


@functools.lru_cache(maxsize=None)
def inputs(robot):
    """-> (dof [KMAX][2n], roots [KMAX][A][13], vd [KMAX][6 + n]) fp32, read-only"""
    dof0, roots0 = fc.inputs(robot)
    out = draw_rates(dof0, roots0, scene_of(robot).robot_idx)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def quat_mul(a, b):
    """a (x) b, xyzw"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_exp(phi):
    """the unit quaternion (xyzw) of the rotation vector phi"""
    a = float(np.linalg.norm(phi))
    s = 0.5 if a < 1e-12 else np.sin(a / 2) / a
    return np.array([s * phi[0], s * phi[1], s * phi[2], np.cos(a / 2)])


def gravity_of(model):
    on = bool(model.actors[model.robot_actor].gravity)
    return np.array([model.gravity[j] for j in range(3)], np.float64) if on else np.zeros(3)


def body_inertias(model, moving, dtype=np.float64):
    """(m, h, Io) of the body frames of body_frame_model, the base's last"""
    sym = lambda Io: np.array([[Io[0], Io[1], Io[2]], [Io[1], Io[3], Io[4]], [Io[2], Io[4], Io[5]]], dtype)
    out = [(dtype(model.bodies[i].mass), np.array(list(model.bodies[i].h), dtype), sym(list(model.bodies[i].Io))) for i in range(int(model.n_bodies))]
    if moving:
        out.append((dtype(model.base_mass), np.array(list(model.base_h), dtype), sym(list(model.base_Io))))
    return out


def _flow(root, q, v, r, s):
    """the state a time s along the flow of constant v = (linvel, angvel, qd): (root, q)"""
    out = np.array(root, np.float64)
    out[r, 0:3] = out[r, 0:3] + s * v[0:3]
    out[r, 3:7] = quat_mul(quat_exp(s * v[3:6]), out[r, 3:7])
    return out, q + s * v[6:]


def env_parts(o64, model, root, q, v, vd, moving=True):
    """one env -> (M vd, C v, g, gap of the two Richardson levels, J [nf][6][N], I6 [nf][6][6]) in fp64.  moving: root [A][13] with the
    env's own pose (its twist columns are set from v), v and vd [6 + n]; fixed: the base rows are left out, v and vd [n]"""
    bm, first = fc.body_frame_model(model)
    n = len(q)
    r = int(model.robot_actor)
    inert = body_inertias(model, moving)
    nf, C0 = len(inert), 6 if moving else 0
    root = np.array(root, np.float64)
    root[:, 7:13] = 0.0
    vfull = v if moving else np.concatenate([np.zeros(6), v])

    def rows_at(s):
        rt, qs = _flow(root, q, vfull, r, s) if moving else (root, q + s * v)
        rt = np.array(rt)
        if moving:
            rt[r, 7:13] = v[0:6]
        return o64.rigid_body_state(bm, rt, qs, vfull[6:])[0][first:first + nf].astype(np.float64)

    J = (fc.oracle_J(o64, bm, root[None], q[None])[0] if moving else fc.fixed_oracle_J(o64, bm, root, q[None])[0][:, :, 6:])[first:first + nf]
    rows = rows_at(0.0)
    c = [(rows_at(s)[:, 7:13] - rows_at(-s)[:, 7:13]) / (2.0 * s) for s in (H_STEP, 2.0 * H_STEP, 4.0 * H_STEP)]
    Jdv = (4.0 * c[0] - c[1]) / 3.0
    gap = float(np.abs(Jdv - (4.0 * c[1] - c[2]) / 3.0).max())
    g6 = np.concatenate([gravity_of(model), np.zeros(3)])
    N = n + C0
    pM, pC, pg = np.zeros(N), np.zeros(N), np.zeros(N)
    I6s = np.zeros((nf, 6, 6))
    for i, (m_i, h, Io) in enumerate(inert):
        R = fc.quat_R(rows[i, 3:7], np.float64)
        hw, Iw = R @ h, R @ Io @ R.T
        I6 = np.zeros((6, 6))
        I6[0:3, 0:3] = m_i * np.eye(3)
        I6[0:3, 3:6] = -fc.skew(hw)
        I6[3:6, 0:3] = fc.skew(hw)
        I6[3:6, 3:6] = Iw
        I6s[i] = I6
        w = rows[i, 10:13]
        vel = np.concatenate([np.cross(w, np.cross(w, hw)), np.cross(w, Iw @ w)])
        pM += J[i].T @ (I6 @ (J[i] @ vd))
        pC += J[i].T @ (I6 @ Jdv[i] + vel)
        pg += J[i].T @ (I6 @ (-g6))
    return pM, pC, pg, gap, J, I6s


def reference_parts(o64, model, roots, q, v, vd):
    """-> ({'M', 'C', 'g'} each [K][6 + n], the largest Richardson gap) in fp64 for a moving base; roots [K][A][13]"""
    roots, q, v, vd = (np.asarray(a, np.float64) for a in (roots, q, v, vd))
    out = [env_parts(o64, model, roots[k], q[k], v[k], vd[k])[:4] for k in range(len(q))]
    return {"M": np.stack([o[0] for o in out]), "C": np.stack([o[1] for o in out]), "g": np.stack([o[2] for o in out])}, max(o[3] for o in out)


def fixed_parts(o64, model, root, q, qd, qdd):
    """the same route on a FIXED-base robot -> ({'M', 'C', 'g'} each [K][n], gap): comparable to inverse_dynamics_cases.reference_parts"""
    q, qd, qdd = (np.asarray(a, np.float64) for a in (q, qd, qdd))
    out = [env_parts(o64, model, root, q[k], qd[k], qdd[k], moving=False)[:4] for k in range(len(q))]
    return {"M": np.stack([o[0] for o in out]), "C": np.stack([o[1] for o in out]), "g": np.stack([o[2] for o in out])}, max(o[3] for o in out)


def mass_matrix_along_flow(o64, model, root, q, v, s):
    """congruence_M of a moving base a time s along the flow of constant v"""
    rt, qs = _flow(np.asarray(root, np.float64), np.asarray(q, np.float64), v, int(model.robot_actor), s)
    return fc.congruence_M(o64, model, rt[None], qs[None], True)[0]


def power_gap(o64, model, root, q, v, Cv, h=H_STEP):
    """v^T (C v) - v^T Mdot v / 2 with Mdot the central difference of congruence_M along the flow, Richardson-extrapolated like
    Jdot v (the plain difference at h = 1e-3 is itself off by 1e-7 of the power) -> (gap, v^T C v)"""
    c = [(mass_matrix_along_flow(o64, model, root, q, v, s) - mass_matrix_along_flow(o64, model, root, q, v, -s)) / (2.0 * s) for s in (h, 2.0 * h)]
    Md = (4.0 * c[0] - c[1]) / 3.0
    return float(v @ Cv - 0.5 * v @ Md @ v), float(v @ Cv)


# ---- the metric ---------------------------------------------------------------------------------------------------------------------
def row_units(model_json):
    """True where the row of tau is a force (N): the base force and the prismatic joints; False: moments (N m)"""
    return np.array([True] * 3 + [False] * 3 + [b["jtype"] != "revolute" for b in model_json["bodies"]])


def scale(ref, force_rows):
    """D_j of one call's reference, floored at FLOOR of the largest D among rows of the same unit"""
    D = np.abs(ref).max(0)
    out = D.copy()
    for unit in (force_rows, ~force_rows):
        if unit.any():
            out[unit] = np.maximum(D[unit], FLOOR * D[unit].max())
    return out


def e_tau(tau, ref, force_rows):
    """the metric of one call against its own reference; a reference that is zero everywhere asks for exact zeros"""
    tau = np.asarray(tau, np.float64)
    if not ref.any():
        return 0.0 if not tau.any() else float("inf")
    return float((np.abs(tau - ref) / scale(ref, force_rows)[None, :]).max())


# ---- the fp32 restatement -----------------------------------------------------------------------------------------------------------
def floating_newton_euler(model_json, base_inertia, quat, wb, q, qd, vd, g_world, f=np.float32):
    """tau [6 + n] by the Luh-Walker-Paul recursion with 3-vectors in BODY frames and a MOVING root, every operation in precision f on
    inputs rounded to f.  base_inertia: (m, h, Io [3][3]) of the base in its own axes about its origin; quat: the base orientation
    (xyzw); wb: the base angular velocity, vd[0:6]: the acceleration of the base origin and the angular acceleration, world axes."""
    bodies = model_json["bodies"]
    n = len(bodies)
    q, qd, vd, wb, g_world = (np.asarray(a, f) for a in (q, qd, vd, wb, g_world))
    Rb = fc.quat_R(np.asarray(quat, f) / np.sqrt(np.sum(np.asarray(quat, f) ** 2, dtype=f)), f)
    Eb = Rb.T
    zero = np.zeros(3, f)
    w0, wd0, a0 = Eb @ wb, Eb @ vd[3:6], Eb @ (vd[0:3] - g_world)      # the base's motion in its own axes; gravity as an acceleration
    qdd = vd[6:]

    def rigid(m, h, Io, w, wd, a):
        m = f(m)
        h = np.asarray(h, f)
        c = h / m if m > 0 else zero
        Ic = np.asarray(Io, f) - m * ((c @ c) * np.eye(3, dtype=f) - np.outer(c, c))
        F = m * (a + np.cross(wd, c) + np.cross(w, np.cross(w, c)))
        return F, Ic @ wd + np.cross(w, Ic @ w) + np.cross(c, F)

    Fb, Nb = rigid(base_inertia[0], base_inertia[1], base_inertia[2], w0, wd0, a0)
    R, p, w, wd, a, F, N = ([None] * n for _ in range(7))
    for i, b in enumerate(bodies):
        ax, Rt, pt = np.asarray(b["axis"], f), np.asarray(b["R_tree"], f), np.asarray(b["p_tree"], f)
        par = b["parent"]
        rev = b["jtype"] == "revolute"
        R[i], p[i] = (Rt @ ic._rot_axis(ax, q[i], f), pt) if rev else (Rt, pt + (Rt @ ax) * q[i])
        wp, wdp, ap = (w0, wd0, a0) if par < 0 else (w[par], wd[par], a[par])
        E = R[i].T
        carried = E @ (ap + np.cross(wdp, p[i]) + np.cross(wp, np.cross(wp, p[i])))
        if rev:
            w[i] = E @ wp + ax * qd[i]
            wd[i] = E @ wdp + ax * qdd[i] + np.cross(E @ wp, ax * qd[i])
            a[i] = carried
        else:
            w[i], wd[i] = E @ wp, E @ wdp
            a[i] = carried + f(2) * np.cross(w[i], ax * qd[i]) + ax * qdd[i]
        I = b["inertia"]
        Io = [[I["Io"][0], I["Io"][1], I["Io"][2]], [I["Io"][1], I["Io"][3], I["Io"][4]], [I["Io"][2], I["Io"][4], I["Io"][5]]]
        F[i], N[i] = rigid(I["mass"], I["h"], Io, w[i], wd[i], a[i])
        assert all(x.dtype == f for x in (R[i], p[i], w[i], wd[i], a[i], F[i], N[i]))
    tau = np.zeros(6 + n, f)
    for i in reversed(range(n)):
        b = bodies[i]
        tau[6 + i] = (N[i] if b["jtype"] == "revolute" else F[i]) @ np.asarray(b["axis"], f)
        fpar = R[i] @ F[i]
        if b["parent"] >= 0:
            F[b["parent"]] = F[b["parent"]] + fpar
            N[b["parent"]] = N[b["parent"]] + R[i] @ N[i] + np.cross(p[i], fpar)
        else:
            Fb = Fb + fpar
            Nb = Nb + R[i] @ N[i] + np.cross(p[i], fpar)
    tau[0:3], tau[3:6] = Rb @ Fb, Rb @ Nb
    assert tau.dtype == f
    return tau


def restated(model_json, model, roots, dof, vd, terms, with_vd, f=np.float32):
    """[K][6 + n]: floating_newton_euler of every env for one call (a part that is not asked for has its input zeroed)"""
    r = int(model.robot_actor)
    q, qd = dof[:, 0::2], dof[:, 1::2]
    n = q.shape[1]
    base = body_inertias(model, True)[-1]
    g = gravity_of(model) if terms & ID_GRAVITY else np.zeros(3)
    vel = bool(terms & ID_VELOCITY)
    return np.stack([floating_newton_euler(model_json, base, roots[k, r, 3:7], roots[k, r, 10:13] if vel else np.zeros(3), q[k],
                                           qd[k] if vel else np.zeros(n), vd[k] if with_vd else np.zeros(6 + n), g, f) for k in range(len(q))])


# ---- references and tolerances ------------------------------------------------------------------------------------------------------
def references_at(scene, model, roots, dof, vd):
    """-> namespace(parts, gap, force_rows, w32 = worst e of the fp32 restatement over ALL_CALLS, v) at the given state, fp64"""
    from oracle.oracle import Oracle
    o64 = Oracle("f64")
    roots32, dof32, vd32 = (np.ascontiguousarray(a, np.float32) for a in (roots, dof, vd))
    v = fc.generalised_velocity(dof32, roots32, int(model.robot_actor))
    parts, gap = reference_parts(o64, model, roots32, dof32[:, 0::2], v, vd32)
    for a in parts.values():
        a.setflags(write=False)
    force_rows = row_units(scene.robot_model)
    w32 = max(e_tau(restated(scene.robot_model, model, roots32, dof32, vd32, t, wv), combine(parts, t, wv), force_rows) for t, wv in ALL_CALLS)
    return SimpleNamespace(scene=scene, model=model, parts=parts, gap=gap, force_rows=force_rows, w32=w32, v=v)


@functools.lru_cache(maxsize=None)
def references(robot):
    scene = scene_of(robot)
    dof, roots, vd = inputs(robot)
    return references_at(scene, scene.to_c(), roots, dof, vd)


def tolerance_from(w32):
    return min(round_up_125(10.0 * w32), CAP)


def tolerance(robot):
    return tolerance_from(references(robot).w32)
