"""Inputs, references, metrics and tolerances of the moving-base link-acceleration / wrench-force tests
(test_floating_link_acceleration.py, no GPU; test_gpu_floating_link_acceleration.py): mppi_sim_floating_link_acceleration and
mppi_sim_floating_wrench_forces (csrc/mppi_kernels.hpp k_sim_floating_link_acceleration, k_sim_floating_wrench_forces;
csrc/mppi_device.hpp floating_link_accelerations, floating_link_acceleration, gather_floating_link_wrench,
floating_wrench_joint_forces) against the fp64 oracle, every env, every rigid body, every entry.

GENERALISED VELOCITY  v = (root linvel, root angvel, qd) of floating_jacobian_cases, read from the env's own root row and rates; vd its
time derivative; tau the force dual to v (rows 0:3 the force on the base, rows 3:6 the moment about the base origin, then the joints).
INPUTS per robot: floating_inverse_dynamics_cases.inputs(robot) - the four robots and env counts of floating_jacobian_cases.ROBOTS,
every env at a base pose of its own, twist +-1, rates +-1, vd +-3 - and link_acceleration_cases.wrenches(K, n_rb): +-10 N, +-1 N m on
every rigid body.
REFERENCES, always fp64, from the oracle as it stands, on the scene's OWN model (not the body-frame model):
  J_ref      floating_jacobian_cases.oracle_J;
  (Jdot v)_ref the two-level Richardson central difference (h = 1e-3) of columns 7:13 of rigid_body_state along
             floating_inverse_dynamics_cases._flow, the flow of constant v (q +- s qd, the base position +- s v_lin, the base quaternion
             exp(+- s w / 2) (x) quat); the two levels must agree within link_acceleration_cases.RICHARDSON_AGREE (asserted here);
  a_ref    = J_ref vd + (Jdot v)_ref;     tau_ref = sum_b J_ref,b^T w_b.
  With moving = False the same route leaves the base rows out (a fixed base: q +- s qd alone, the joint columns alone) and must
  reproduce link_acceleration_cases.reference_parts within FIXED_ROUTE_AGREE - asserted in the no-GPU half before anything else.
METRICS  e_lin, e_ang as link_acceleration_cases.e_acc against D_lin / D_ang of the FULL call (calls with fewer parts use the same
scales); e_tau = max |tau - ref|[k, j] / D_j with D_j = max_k |tau_ref[k, j]|, floored by the rule of
floating_inverse_dynamics_cases.scale (FLOOR of the largest D among rows of the same unit; every scale is O(1), the floor does not
bind).  Rows that the reference has exactly zero (bodies of box or sphere actors) must be exact zeros.
TOLERANCES per robot and metric, by the project's rule: 10 x the worst deviation of an fp32 RESTATEMENT from the reference over the four
acceleration calls and the wrench call, rounded up to 1-2-5, at most link_acceleration_cases.CAP = 1e-4.  The restatement
(moving_root_accelerations, moving_root_wrench_forces) is a body-frame Luh-Walker-Paul pass with a moving root in np.float32 on
fp32-rounded inputs, in the style of link_acceleration_cases.body_frame_accelerations / body_frame_wrench_forces and
floating_inverse_dynamics_cases.floating_newton_euler - deliberately not the kernel's world-axes formulation, never the code under test."""
import functools
from types import SimpleNamespace

import numpy as np

import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
import link_acceleration_cases as lc
from test_gpu_step_matrix import round_up_125

CAP = lc.CAP
H_STEP = lc.H_STEP
RICHARDSON_AGREE = lc.RICHARDSON_AGREE
# the flow-difference route against link_acceleration_cases.reference_parts on fixed bases: measured exactly 0 in J, J qdd and Jdot qd
# over the mobile manipulator and heijn at both poses - with the base rows left out the route makes the very oracle calls of that
# module.  There is no next 1-2-5 step of zero: the bound leaves room for another order of the same fp64 sums (entries up to 40,
# eps 2.2e-16, a difference divided by 2h = 2e-3: 40 * 2.2e-16 / 2e-3 = 4.4e-12 -> 5e-12) and for nothing else.
FIXED_ROUTE_AGREE = 5e-12
ID_VELOCITY = lc.ID_VELOCITY
FULL, ACC_CALLS = lc.FULL, lc.ACC_CALLS
ROBOTS = fc.ROBOTS
STORE_EDGES = fc.STORE_EDGES
PUSH_SCENE = fc.PUSH_SCENE
FAR_SHIFT = fc.FAR_SHIFT
combine = lc.combine
e_acc = lc.e_acc
scene_of = fi.scene_of


@functools.lru_cache(maxsize=None)
def inputs(robot):
    """-> (dof [KMAX][2n], roots [KMAX][A][13], vd [KMAX][6 + n], wrenches [KMAX][n_rb][6]) fp32, read-only"""
    dof, roots, vd = fi.inputs(robot)
    return dof, roots, vd, lc.wrenches(len(dof), int(scene_of(robot).to_c().n_rb))


# ---- the references -----------------------------------------------------------------------------------------------------------------
def env_Jdot_v(o64, model, root, q, v, moving=True):
    """one env -> ((Jdot v)_ref [n_rb][6], the gap of the two Richardson levels).  moving: root [A][13] at the env's own pose, v [6 + n];
    fixed: the base rows are left out, v [n]"""
    r = int(model.robot_actor)
    root = np.array(root, np.float64)
    root[:, 7:13] = 0.0
    vfull = v if moving else np.concatenate([np.zeros(6), v])

    def columns_at(s):
        rt, qs = fi._flow(root, q, vfull, r, s) if moving else (root, q + s * v)
        rt = np.array(rt)
        if moving:
            rt[r, 7:13] = v[0:6]
        return o64.rigid_body_state(model, rt, qs, vfull[6:])[0][:, 7:13].astype(np.float64)

    c = [(columns_at(s) - columns_at(-s)) / (2.0 * s) for s in (H_STEP, 2.0 * H_STEP, 4.0 * H_STEP)]
    out = (4.0 * c[0] - c[1]) / 3.0
    return out, float(np.abs(out - (4.0 * c[1] - c[2]) / 3.0).max())


def route_parts(o64, model, roots, q, v, vd, moving=True):
    """-> (J_ref [K][n_rb][6][N], {'A': J vd, 'V': Jdot v, 'gap'}) in fp64, N = 6 + n (moving; roots [K][A][13]) or n (fixed; roots [A][13]);
    asserts the agreement of the two Richardson levels"""
    q, v, vd = (np.asarray(a, np.float64) for a in (q, v, vd))
    roots = np.asarray(roots, np.float64)
    J = fc.oracle_J(o64, model, roots, q) if moving else fc.fixed_oracle_J(o64, model, roots, q)[:, :, :, 6:]
    out = [env_Jdot_v(o64, model, roots[k] if moving else roots, q[k], v[k], moving) for k in range(len(q))]
    gap = max(o[1] for o in out)
    assert gap <= RICHARDSON_AGREE, f"the two Richardson levels of (Jdot v)_ref differ by {gap:.2e}"
    return J, {"A": np.einsum("kbri,ki->kbr", J, vd), "V": np.stack([o[0] for o in out]), "gap": gap}


wrench_reference = lc.wrench_reference


def e_tau(tau, tau_ref, Dj):
    return float((np.abs(np.asarray(tau, np.float64) - tau_ref) / Dj[None, :]).max())


# ---- the fp32 restatement -----------------------------------------------------------------------------------------------------------
def _base_rotation(quat, f):
    quat = np.asarray(quat, f)
    return fc.quat_R(quat / np.sqrt(np.sum(quat ** 2, dtype=f)), f)


def moving_root_accelerations(model_json, quat, wb, q, qd, vd, f=np.float32):
    """[L][6] of every link: the outward half of the body-frame Luh-Walker-Paul recursion with a MOVING root and without gravity, every
    operation in precision f on inputs rounded to f; the root's motion (wb; vd[0:3], vd[3:6], world axes) is turned into the base's own
    axes first, a link's row into world axes at the very end"""
    bodies, links = model_json["bodies"], model_json["links"]
    n = len(bodies)
    q, qd, vd, wb = (np.asarray(a, f) for a in (q, qd, vd, wb))
    Rb = _base_rotation(quat, f)
    R, p, Rw = lc._body_frames(model_json, Rb, q, f)
    w0, wd0, a0 = Rb.T @ wb, Rb.T @ vd[3:6], Rb.T @ vd[0:3]
    qdd = vd[6:]
    w, wd, a = [None] * n, [None] * n, [None] * n
    for i, b in enumerate(bodies):
        ax, par = np.asarray(b["axis"], f), b["parent"]
        wp, wdp, ap = (w0, wd0, a0) if par < 0 else (w[par], wd[par], a[par])
        E = R[i].T
        carried = E @ (ap + np.cross(wdp, p[i]) + np.cross(wp, np.cross(wp, p[i])))
        if b["jtype"] == "revolute":
            w[i] = E @ wp + ax * qd[i]
            wd[i] = E @ wdp + ax * qdd[i] + np.cross(E @ wp, ax * qd[i])
            a[i] = carried
        else:
            w[i], wd[i] = E @ wp, E @ wdp
            a[i] = carried + f(2) * np.cross(w[i], ax * qd[i]) + ax * qdd[i]
        assert all(x.dtype == f for x in (R[i], p[i], Rw[i], w[i], wd[i], a[i]))
    out = np.zeros((len(links), 6), f)
    for l, L in enumerate(links):
        i = L["body"]
        Rl, wl, wdl, al = (Rb, w0, wd0, a0) if i < 0 else (Rw[i], w[i], wd[i], a[i])
        r = np.asarray(L["p"], f)
        out[l, 0:3] = Rl @ (al + np.cross(wdl, r) + np.cross(wl, np.cross(wl, r)))
        out[l, 3:6] = Rl @ wdl
    assert out.dtype == f
    return out


def moving_root_wrench_forces(model_json, quat, q, w, f=np.float32):
    """tau [6 + n] of the wrenches w [L][6] (world axes, about the link frame origins): each wrench turned into its body's frame (the base's
    for a link welded to it) and moved to that frame's origin, then the inward half of the body-frame recursion down to the root, whose
    sums are turned into world axes at the very end; every operation in precision f"""
    bodies, links = model_json["bodies"], model_json["links"]
    n = len(bodies)
    q, w = np.asarray(q, f), np.asarray(w, f)
    Rb = _base_rotation(quat, f)
    R, p, Rw = lc._body_frames(model_json, Rb, q, f)
    F, N = [np.zeros(3, f) for _ in range(n)], [np.zeros(3, f) for _ in range(n)]
    Fb, Nb = np.zeros(3, f), np.zeros(3, f)
    for l, L in enumerate(links):
        i = L["body"]
        E = (Rb if i < 0 else Rw[i]).T
        fb = E @ w[l, 0:3]
        nb = E @ w[l, 3:6] + np.cross(np.asarray(L["p"], f), fb)
        if i < 0:
            Fb, Nb = Fb + fb, Nb + nb
        else:
            F[i], N[i] = F[i] + fb, N[i] + nb
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
    assert tau.dtype == f and Fb.dtype == f and Nb.dtype == f
    return tau


def restated_acc(model_json, model, roots, dof, vd, terms, with_vd, f=np.float32):
    """[K][L][6]: moving_root_accelerations of every env for one call (a part that is not asked for has its input zeroed)"""
    r = int(model.robot_actor)
    q, qd = dof[:, 0::2], dof[:, 1::2]
    n = q.shape[1]
    vel = bool(terms & ID_VELOCITY)
    return np.stack([moving_root_accelerations(model_json, roots[k, r, 3:7], roots[k, r, 10:13] if vel else np.zeros(3), q[k],
                                               qd[k] if vel else np.zeros(n), vd[k] if with_vd else np.zeros(6 + n), f) for k in range(len(q))])


def restated_tau(model_json, model, roots, dof, w, f=np.float32):
    r = int(model.robot_actor)
    return np.stack([moving_root_wrench_forces(model_json, roots[k, r, 3:7], dof[k, 0::2], w[k], f) for k in range(len(dof))])


# ---- references and tolerances ------------------------------------------------------------------------------------------------------
def references_at(scene, model, roots, dof, vd, w, scales=None):
    """the references and the restatement's worst deviations at the given state -> a namespace: scene, model, J, parts, D (D_lin, D_ang),
    tau_ref, Dj, zero (bodies with an exactly zero reference), w32 (worst restatement e_lin, e_ang, e_tau), first, L, v, force_rows.
    scales: (D, Dj) of the robot's whole input set, for a state that is the first few envs of it (one env alone has scales of its own
    that are no measure of the robot's); None: the scales of the given state"""
    from oracle.oracle import Oracle
    o64 = Oracle("f64")
    roots32, dof32, vd32, w32in = (np.ascontiguousarray(a, np.float32) for a in (roots, dof, vd, w))
    a = int(model.robot_actor)
    first, L = int(model.actors[a].first_rb), len(scene.robot_model["links"])
    assert L == int(model.actors[a].n_rb)
    v = fc.generalised_velocity(dof32, roots32, a)
    J, parts = route_parts(o64, model, roots32, dof32[:, 0::2], v, vd32)
    tau_ref = wrench_reference(J, w32in)
    force_rows = fi.row_units(scene.robot_model)
    D, Dj = (lc.scales(parts), fi.scale(tau_ref, force_rows)) if scales is None else scales
    worst = [0.0, 0.0, 0.0]
    for call in ACC_CALLS:
        got = restated_acc(scene.robot_model, model, roots32, dof32, vd32, *call)
        el, ea = e_acc(got, combine(parts, *call)[:, first:first + L], D)
        worst[0], worst[1] = max(worst[0], el), max(worst[1], ea)
    worst[2] = e_tau(restated_tau(scene.robot_model, model, roots32, dof32, w32in[:, first:first + L]),
                     wrench_reference(J[:, first:first + L], w32in[:, first:first + L]), Dj)
    for x in (J, parts["A"], parts["V"], tau_ref):
        x.setflags(write=False)
    return SimpleNamespace(scene=scene, model=model, J=J, parts=parts, D=D, tau_ref=tau_ref, Dj=Dj, zero=lc.zero_bodies(J), w32=tuple(worst),
                           first=first, L=L, v=v, force_rows=force_rows)


@functools.lru_cache(maxsize=None)
def references(robot):
    scene = scene_of(robot)
    dof, roots, vd, w = inputs(robot)
    return references_at(scene, scene.to_c(), roots, dof, vd, w)


def tolerances_from(worst):
    return tuple(min(round_up_125(10.0 * x), CAP) for x in worst)


def tolerances(robot):
    """-> (tol_lin, tol_ang, tol_tau)"""
    return tolerances_from(references(robot).w32)


def measure(acc, tau, r, rows=None):
    """worst (e_lin, e_ang) per acceleration call and e_tau of results {call: [K][n_rb][6]}, tau [K][6 + n] over the first len(tau) envs"""
    K = len(tau)
    out = {c: e_acc(acc[c], combine(r.parts, *c)[:K], r.D) for c in acc}
    return out, e_tau(tau, r.tau_ref[:K], r.Dj)
