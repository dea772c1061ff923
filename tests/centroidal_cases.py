"""Inputs, references, metrics and tolerances of the whole-robot tests (test_centroidal.py, no GPU; test_gpu_centroidal.py):
mppi_sim_momentum, mppi_sim_centroidal_matrix and mppi_sim_floating_centroidal_matrix (csrc/mppi_kernels.hpp k_sim_momentum,
k_sim_centroidal_matrix, k_sim_floating_centroidal_matrix; csrc/mppi_device.hpp momentum_pass, centroidal_matrix_pass) against an fp64
reference built from what the oracle exports, every env, every entry.

THE ROW  (m, c [3], p [3], L about c [3], T, V) of the bodies the packed model moves - for a moving base the base's own rigid body
too; a link welded to a FIXED base is no part of it.  THE MATRIX  A [6][N] with A v = (p, L): v = qd (N = n) for a fixed base,
v = (root linvel, root angvel, qd) (N = 6 + n) of floating_jacobian_cases for a moving one.
INPUTS, reused: fixed bases - inverse_dynamics_cases.inputs(robot, pose) for franka_panda, panda_gripper (branching, prismatic
fingers), point_robot, heijn and omnipanda at the poses origin and tilted, gravity on; moving bases - floating_inverse_dynamics_cases.
inputs(robot) for boxer, jackal_a, albert and anymal (every env a base pose and twist of its own, gravity on).  STORE_EDGES of those
modules: K = 1, 63, 64, 65, 130 on one robot of each kind and 65 on the others.
REFERENCE, always fp64, never the code under test: Oracle("f64").rigid_body_state on floating_jacobian_cases.body_frame_model(model) at
the simulator's own state gives every body frame's p_i, quaternion (R), v_i, w_i.  With (m_i, h_i, Io_i) of model.bodies[i] (base_*
for a moving base) and hw = R h_i:
    m = sum m_i        m c = sum (m_i p_i + hw)        p = sum (m_i v_i + w_i x hw)
    L = sum [R Io R^T w_i + hw x v_i + (p_i - c) x (m_i v_i + w_i x hw)]
    T = sum [v; w]^T I6 [v; w] / 2   with the I6 = [[m 1, -[hw]x], [[hw]x, R Io R^T]] of congruence_M
    V = -g . (m c)   when the robot's gravity is on, else 0
    A_ref = sum X^T(p_i - c) I6_i J_i,  X^T(r) = [[1, 0], [[r]x, 1]],  J_i = oracle_J / fixed_oracle_J of the body-frame model
METRICS  max absolute error per quantity over envs, made scale-free by the largest norm of that quantity over the robot's envs
(euclidean norm of the 3-vectors and of the 3-vector column halves of A, absolute value of the scalars); the error of c is in
metres against 1 m.  A quantity whose reference is zero everywhere must come out as exact zeros (V with gravity off).
TOLERANCES, per robot and quantity, by the project's rule: 10 x the worst deviation of the fp32 route from the fp64 reference - for
a fixed base over both poses -, rounded up to 1-2-5 (round_up_125), at most CAP = 1e-4.  The fp32 route: Oracle("f32") rows (and
Jacobians) with the same sums wholly in np.float32."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
import inverse_dynamics_cases as ic
from test_gpu_step_matrix import round_up_125

CAP = 1e-4
FIXED_ROBOTS = ("franka_panda", "panda_gripper", "point_robot", "heijn", "omnipanda")
MOVING_ROBOTS = ("boxer", "jackal_a", "albert", "anymal")
FIXED_POSES = ("origin", "tilted")
FIXED_CASES = [(r, p) for r in FIXED_ROBOTS for p in FIXED_POSES]
FIXED_STORE_EDGES, MOVING_STORE_EDGES = ic.STORE_EDGES, fi.STORE_EDGES
GRIPPER_SCENE, PUSH_SCENE, FAR_SHIFT = ic.jc.GRIPPER_SCENE, fi.PUSH_SCENE, fi.FAR_SHIFT
QUANTITIES = ("m", "c", "p", "L", "T", "V", "A_lin", "A_ang")
COLS = {"m": slice(0, 1), "c": slice(1, 4), "p": slice(4, 7), "L": slice(7, 10), "T": slice(10, 11), "V": slice(11, 12)}
# the steps' cases (test_gpu_centroidal.py rows 6 and 7)
ENERGY_K, MOMENTUM_K, STEPS = 8, 8, 50
BOXER_HEIGHT = 1.0


def is_moving(model):
    return not bool(model.actors[int(model.robot_actor)].fixed)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _I6(m_i, hw, Iw, dtype):
    I6 = np.zeros((6, 6), dtype)
    I6[0:3, 0:3] = m_i * np.eye(3, dtype=dtype)
    I6[0:3, 3:6] = -fc.skew(hw)
    I6[3:6, 0:3] = fc.skew(hw)
    I6[3:6, 3:6] = Iw
    return I6


def env_row_and_matrix(rows, J, inert, g, dtype=np.float64):
    """one env: rows [nf][13] of the body frames, J [nf][6][N] their Jacobians (or None), inert [(m, h, Io)] -> (row [12], A [6][N] or None)
    with every product and sum in dtype"""
    rows = np.asarray(rows, dtype)
    m, mc, p, T = dtype(0), np.zeros(3, dtype), np.zeros(3, dtype), dtype(0)
    per = []
    for i, (m_i, h, Io) in enumerate(inert):
        R = fc.quat_R(rows[i, 3:7], dtype)
        hw, Iw = R @ h, R @ Io @ R.T
        v, w = rows[i, 7:10], rows[i, 10:13]
        pl = m_i * v + np.cross(w, hw)
        la = Iw @ w + np.cross(hw, v)
        I6 = _I6(m_i, hw, Iw, dtype)
        vw = np.concatenate([v, w])
        m = m + m_i
        mc = mc + (m_i * rows[i, 0:3] + hw)
        p = p + pl
        T = T + dtype(0.5) * (vw @ (I6 @ vw))
        per.append((rows[i, 0:3], pl, la, I6))
    c = mc / m
    L = np.zeros(3, dtype)
    A = None if J is None else np.zeros((6, J.shape[2]), dtype)
    for i, (p_i, pl, la, I6) in enumerate(per):
        L = L + (la + np.cross(p_i - c, pl))
        if J is not None:
            XT = np.eye(6, dtype=dtype)
            XT[3:6, 0:3] = fc.skew(p_i - c)
            A = A + XT @ (I6 @ np.asarray(J[i], dtype))
    V = -(np.asarray(g, dtype) @ mc)
    out = np.concatenate([[m], c, p, L, [T], [V]]).astype(dtype)
    assert out.dtype == dtype and (A is None or A.dtype == dtype)
    return out, A


def route(o, model, roots, dof, dtype=np.float64, with_A=True):
    """the route of the module docstring with the oracle `o`, every sum in dtype -> (rows [K][12], A [K][6][N] or None) as fp64 arrays.
    roots: [K][A][13] for a moving base (every env its own), [A][13] or [K][A][13] for a fixed one; dof [K][2n]"""
    moving = is_moving(model)
    bm, first = fc.body_frame_model(model)
    dof = np.asarray(dof, np.float64)
    q, qd = dof[:, 0::2], dof[:, 1::2]
    K, n = q.shape
    roots = np.asarray(roots, np.float64)
    if roots.ndim == 2:
        roots = np.tile(roots, (K, 1, 1))
    inert = fi.body_inertias(model, moving, dtype)
    nf = len(inert)
    g = fi.gravity_of(model)
    J = None
    if with_A:
        J = fc.oracle_J(o, bm, roots, q) if moving else np.stack([fc.fixed_oracle_J(o, bm, roots[k], q[k:k + 1])[0][:, :, 6:] for k in range(K)])
        J = J[:, first:first + nf]
    out, As = [], []
    for k in range(K):
        rows = o.rigid_body_state(bm, roots[k], q[k], qd[k])[0][first:first + nf]
        row, A = env_row_and_matrix(rows, None if J is None else J[k], inert, g, dtype)
        out.append(row.astype(np.float64))
        As.append(None if A is None else A.astype(np.float64))
    return np.stack(out), (np.stack(As) if with_A else None)


def generalised_velocity(model, dof, roots):
    """v [K][N]: qd for a fixed base, (root linvel, root angvel, qd) for a moving one"""
    if is_moving(model):
        return fc.generalised_velocity(dof, roots, int(model.robot_actor))
    return np.asarray(dof, np.float64)[:, 1::2]


# ---- the metrics --------------------------------------------------------------------------------------------------------------------
def split(rows, A):
    """the quantities of QUANTITIES as arrays [K][...]; the halves of A as [K][N][3] (one 3-vector per column)"""
    rows = np.asarray(rows, np.float64)
    out = {name: rows[:, cols] for name, cols in COLS.items()}
    if A is not None:
        A = np.asarray(A, np.float64)
        out["A_lin"], out["A_ang"] = np.swapaxes(A[:, 0:3, :], 1, 2), np.swapaxes(A[:, 3:6, :], 1, 2)
    return out


def scales(ref):
    """the largest norm of every quantity of split(reference) over the envs; 1 m for c"""
    out = {name: float(np.linalg.norm(a, axis=-1).max()) for name, a in ref.items()}
    out["c"] = 1.0
    return out


def errors(got, ref, D):
    """{quantity: max abs error / scale}; a quantity whose reference is zero everywhere asks for exact zeros (0.0 or inf)"""
    out = {}
    for name, r in ref.items():
        if name not in got:
            continue
        g = np.asarray(got[name], np.float64)
        if not r.any():
            out[name] = 0.0 if not g.any() else float("inf")
        else:
            out[name] = float(np.abs(g - r).max() / D[name])
    return out


# ---- references and tolerances ------------------------------------------------------------------------------------------------------
def references_at(scene, model, roots, dof, with_A=True):
    """-> namespace(rows, A, ref = split, D = scales, w32 = errors of the fp32 route, v) at the given state, fp64"""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    dof32 = np.ascontiguousarray(dof, np.float32)
    roots32 = np.ascontiguousarray(roots, np.float32)
    rows, A = route(o64, model, roots32, dof32, np.float64, with_A)
    ref = split(rows, A)
    D = scales(ref)
    rows32, A32 = route(o32, model, roots32, dof32, np.float32, with_A)
    w32 = errors(split(rows32, A32), ref, D)
    for a in (rows, A):
        if a is not None:
            a.setflags(write=False)
    return SimpleNamespace(scene=scene, model=model, rows=rows, A=A, ref=ref, D=D, w32=w32, v=generalised_velocity(model, dof32, roots32))


def fixed_scene(robot, pose="origin", gravity=True):
    return ic.scene_of(robot, pose, gravity)


@functools.lru_cache(maxsize=None)
def fixed_inputs(robot, pose="origin"):
    """-> (dof [KMAX][2n] fp32, root [A][13]) of inverse_dynamics_cases at that pose"""
    scene = fixed_scene(robot, pose)
    _, root = scene.initial_state()
    return ic.inputs(robot, pose)[0], np.asarray(root, np.float64)


@functools.lru_cache(maxsize=None)
def fixed_references(robot, pose="origin"):
    scene = fixed_scene(robot, pose)
    dof, root = fixed_inputs(robot, pose)
    return references_at(scene, scene.to_c(), root, dof)


def moving_inputs(robot):
    """-> (dof [KMAX][2n], roots [KMAX][A][13]) fp32 of floating_inverse_dynamics_cases"""
    dof, roots, _ = fi.inputs(robot)
    return dof, roots


@functools.lru_cache(maxsize=None)
def moving_references(robot):
    scene = fi.scene_of(robot)
    dof, roots = moving_inputs(robot)
    return references_at(scene, scene.to_c(), roots, dof)


def tolerances_from(*w32s):
    """{quantity: tolerance} from the fp32 route's errors (the worst of several runs); a quantity that must be exactly zero keeps 0"""
    return {name: min(round_up_125(10.0 * max(w[name] for w in w32s)), CAP) if max(w[name] for w in w32s) > 0.0 else 0.0 for name in w32s[0]}


@functools.lru_cache(maxsize=None)
def _tolerances(robot):
    if robot in MOVING_ROBOTS:
        return tolerances_from(moving_references(robot).w32)
    return tolerances_from(*(fixed_references(robot, pose).w32 for pose in FIXED_POSES))


def tolerances(robot):
    return dict(_tolerances(robot))


def report(tag, e, tol):
    return f"[{tag}] " + ", ".join(f"{name} {e[name]:.1e} ({tol[name]:.0e})" for name in e)


def within(e, tol):
    return all(e[name] <= tol[name] for name in e)


# ---- the device's own tensors (test_gpu_centroidal.py row 2) --------------------------------------------------------------------------
EPS32 = float(np.finfo(np.float32).eps)


def shifted_mass_rows(M, r):
    """rows 0:6 of M [K][N][N] moved to the centre of mass: A[0:3] = M[0:3], A[3:6] = M[3:6] - [r]x M[0:3]; r [K][3]"""
    M, r = np.asarray(M, np.float64), np.asarray(r, np.float64)
    out = np.array(M[:, 0:6, :])
    for k in range(len(M)):
        out[k, 3:6] -= fc.skew(r[k]) @ M[k, 0:3]
    return out


# ---- stepping the oracle (test_gpu_centroidal.py rows 6 and 7) ------------------------------------------------------------------------
def oracle_envs_trajectory(o, model, dof, roots, u, steps):
    """orc_envs_step from per-env dof [K][2n] and roots [K][A][13] under the constant per-env commands u [K][nu] -> (dof after every
    step [steps][K][2n], roots after every step [steps][K][A][13], contact forces [steps][K][n_rb][3]), fp64"""
    f = o.dtype
    K = len(dof)
    dof = np.ascontiguousarray(dof, f).copy()
    roots = np.ascontiguousarray(roots, f).copy()
    rb, cf = np.zeros((K, model.n_rb, 13), f), np.zeros((K, model.n_rb, 3), f)
    u = np.ascontiguousarray(u, f)
    out_dof, out_roots, out_cf = [], [], []
    for _ in range(steps):
        o.lib.orc_envs_step(C.byref(model), C.c_int(K), C.c_int(0), o.p(u), o.p(dof), o.p(roots), o.p(rb), o.p(cf))
        out_dof.append(dof.astype(np.float64))
        out_roots.append(roots.astype(np.float64))
        out_cf.append(cf.astype(np.float64))
    return np.stack(out_dof), np.stack(out_roots), np.stack(out_cf)


def _energy_tolerance(E64, E32):
    """(tolerance, scale, worst fp32 deviation): 10 x the worst deviation of the fp32 oracle's trajectory, summed in fp32, from the fp64
    one over all steps and envs, relative to the largest |value| along the fp64 trajectory, rounded up to 1-2-5, at most CAP"""
    D = float(np.abs(E64).max())
    w32 = float(np.abs(E32 - E64).max() / D)
    return min(round_up_125(10.0 * w32), CAP), D, w32


@functools.lru_cache(maxsize=None)
def energy_case():
    """An effort-driven Panda with gravity under ZERO torque (inverse_dynamics_cases.actor_file), ENERGY_K starts - the first poses of
    jacobian_cases.inputs with their +-0.1 rates -, STEPS steps of the fp64 oracle -> namespace(scene, model, root, dof0, E [STEPS][K] =
    T + V after every step, E0 [K], tol, D, w32).  The drive's damping and the joint limits take energy out: the drift is printed by
    the GPU test, not asserted against zero."""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    scene = ic.effort_scene()
    model = scene.to_c()
    _, root = scene.initial_state()
    root = np.asarray(root, np.float64)
    dof0 = np.array(ic.jc.inputs("franka_panda")[0][:ENERGY_K])
    roots = np.tile(root, (ENERGY_K, 1, 1))
    u = np.zeros((ENERGY_K, scene.nu))
    d64 = oracle_envs_trajectory(o64, model, dof0, roots, u, STEPS)[0]
    d32 = oracle_envs_trajectory(o32, model, dof0, roots, u, STEPS)[0]
    E64 = np.stack([route(o64, model, root, d, np.float64, False)[0][:, 10:12].sum(1) for d in d64])
    E32 = np.stack([route(o32, model, root, d.astype(np.float32), np.float32, False)[0][:, 10:12].sum(1) for d in d32])
    E0 = route(o64, model, root, dof0, np.float64, False)[0][:, 10:12].sum(1)
    tol, D, w32 = _energy_tolerance(E64, E32)
    return SimpleNamespace(scene=scene, model=model, root=root, dof0=dof0, E=E64, E0=E0, tol=tol, D=D, w32=w32)


@functools.lru_cache(maxsize=None)
def momentum_case():
    """A boxer with `gravity: false` BOXER_HEIGHT above the ground, upright, every env with a base twist of its own (+-0.5 m/s sideways,
    0 .. 0.2 m/s upwards, +-1 rad/s) and constant wheel commands, STEPS steps of the fp64 oracle: nothing touches it, so p and L
    change by the integrator's own error only -> namespace(scene, model, dof0, roots0, u, rows [STEPS][K][12], rows0 [K][12], cf,
    tol {p, L}, D {p, L}, w32 {p, L})"""
    from oracle.oracle import Oracle
    from scenes import build_scene
    o64, o32 = Oracle("f64"), Oracle("f32")
    scene = build_scene([boxer_actor_file()], [[0.0, 0.0, BOXER_HEIGHT]])
    model = scene.to_c()
    a = scene.robot_idx
    K = MOMENTUM_K
    dof0 = np.array(fi.inputs("boxer")[0][:K])
    roots0 = np.tile(np.asarray(scene.initial_state()[1], np.float32), (K, 1, 1))
    rng = np.random.default_rng(31)
    roots0[:, a, 7:9], roots0[:, a, 9], roots0[:, a, 10:13] = rng.uniform(-0.5, 0.5, (K, 2)), rng.uniform(0.0, 0.2, K), rng.uniform(-1.0, 1.0, (K, 3))
    u = rng.uniform(-1.0, 1.0, size=(K, scene.nu)).astype(np.float32)
    d64, r64, cf = oracle_envs_trajectory(o64, model, dof0, roots0, u, STEPS)
    d32, r32, _ = oracle_envs_trajectory(o32, model, dof0, roots0, u, STEPS)
    rows = np.stack([route(o64, model, r64[s], d64[s], np.float64, False)[0] for s in range(STEPS)])
    rows32 = np.stack([route(o32, model, r32[s].astype(np.float32), d32[s].astype(np.float32), np.float32, False)[0] for s in range(STEPS)])
    rows0 = route(o64, model, roots0, dof0, np.float64, False)[0]
    tol, D, w32 = {}, {}, {}
    for name in ("p", "L"):
        D[name] = float(np.linalg.norm(rows[:, :, COLS[name]], axis=-1).max())
        w32[name] = float(np.abs(rows32[:, :, COLS[name]] - rows[:, :, COLS[name]]).max() / D[name])
        tol[name] = min(round_up_125(10.0 * w32[name]), CAP)
    return SimpleNamespace(scene=scene, model=model, dof0=dof0, roots0=roots0, u=u, rows=rows, rows0=rows0, cf=cf, tol=tol, D=D, w32=w32)


def body_frames_from_links(model, rb):
    """the body frames' rows [K][nf][13] (the n_bodies bodies, then the base when it moves) recovered in fp64 from rigid-body rows
    rb [K][n_rb][13] of the LINKS: the first link welded to body i at (R_l, p_l) gives R_i = R_link R_l^T, p_i = p_link - R_i p_l,
    v_i = v_link - w x (R_i p_l), w_i = w_link"""
    rb = np.asarray(rb, np.float64)
    a = int(model.robot_actor)
    first, nb = int(model.actors[a].first_rb), int(model.n_bodies)
    frames = list(range(nb)) + ([-1] if is_moving(model) else [])
    out = np.zeros((len(rb), len(frames), 13))
    for j, body in enumerate(frames):
        l = next(l for l in range(int(model.n_links)) if int(model.links[l].body) == body)
        Rl, pl = np.array(list(model.links[l].R)).reshape(3, 3), np.array(list(model.links[l].p))
        for k in range(len(rb)):
            row = rb[k, first + l]
            R = fc.quat_R(row[3:7] / np.linalg.norm(row[3:7]), np.float64) @ Rl.T
            arm = R @ pl
            out[k, j, 0:3] = row[0:3] - arm
            out[k, j, 7:10] = row[7:10] - np.cross(row[10:13], arm)
            out[k, j, 10:13] = row[10:13]
            out[k, j, 3:7] = _quat_of(R)
    return out


def _quat_of(R):
    """xyzw of a rotation matrix (fp64)"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 1e-3:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(max(0.0, 1.0 + R[i, i] - R[j, j] - R[k, k])) * 2.0
    q = np.zeros(4)
    q[i], q[j], q[k], q[3] = s / 4.0, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q


def com_velocity_from_links(model, rb):
    """([K][3], [K]) in fp64: sum (m_i v_i + w_i x R_i h_i) / m over the body frames recovered from the rigid-body rows of the links, and
    the scale of what those fp32 rows carry - sum (m_i / m) (|v_i| + |w_i| (|p_i| + |h_i| / m_i)): the rows' velocities are formed about
    the WORLD origin (csrc/mppi_device.hpp, "spatial quantities in world axes about the world origin"), so a row's last bit is that of
    |w| |p| at the body's world position, and the recovery above moves it by the link's own arm"""
    frames = body_frames_from_links(model, rb)
    inert = fi.body_inertias(model, is_moving(model))
    p, scale, m = np.zeros((len(frames), 3)), np.zeros(len(frames)), 0.0
    for j, (m_j, h, _) in enumerate(inert):
        m += m_j
        for k in range(len(frames)):
            R = fc.quat_R(frames[k, j, 3:7], np.float64)
            v, w = frames[k, j, 7:10], frames[k, j, 10:13]
            p[k] += m_j * v + np.cross(w, R @ h)
            scale[k] += m_j * (np.linalg.norm(v) + np.linalg.norm(w) * np.linalg.norm(frames[k, j, 0:3])) + np.linalg.norm(w) * np.linalg.norm(h)
    return p / m, scale / m


@functools.lru_cache(maxsize=None)
def boxer_actor_file():
    """the shipped boxer with `gravity: false`, as a file of the tests' own -> its path"""
    import os
    import tempfile
    import yaml
    from mppiisaac.utils.isaacgym_utils import CONF_DIR
    with open(os.path.join(CONF_DIR, "actors", "boxer.yaml")) as fh:
        fields = yaml.safe_load(fh)
    fields["gravity"] = False
    path = os.path.join(tempfile.mkdtemp(prefix="centroidal_cases_"), "boxer_nogravity.yaml")
    with open(path, "w") as fh:
        yaml.safe_dump(fields, fh)
    return path
