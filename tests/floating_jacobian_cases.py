"""Inputs, references, metrics and tolerances of the moving-base Jacobian / mass-matrix tests (test_floating_jacobian_mass.py, no
GPU; test_gpu_floating_jacobian_mass.py): mppi_sim_floating_jacobian and mppi_sim_floating_mass_matrix (csrc/mppi_kernels.hpp
k_sim_floating_jacobian, k_sim_floating_mass_matrix; csrc/mppi_device.hpp floating_link_jacobian, floating_mass_matrix) against the
fp64 oracle, every env, every rigid body, every entry.

GENERALISED VELOCITY  v = (root linvel, root angvel, qd): columns 7:10 and 10:13 of the robot's root row, then the joints.
REFERENCES, always fp64, at the state the simulator itself holds (its tensors read back and widened):
  J_ref[:, :, c]     = columns 7:13 of Oracle("f64").rigid_body_state(model, root with root[robot, 7 + c] = 1, q, 0) for c < 6 - the
                       oracle propagates a moving base's root velocity, and the velocity columns are linear in it, so a unit base
                       twist yields a base column exactly;
  J_ref[:, :, 6 + i] = the same call with qd = e_i and zero root velocity (the joint columns of jacobian_cases.oracle_J);
  M_ref              = sum_i J_i^T [[m 1, -[h_w]x], [[h_w]x, R Io R^T]] J_i, the congruence sum over the oracle's Jacobians J_i of the
                       BODY frames: a copy of the model whose robot links are the n_bodies body frames plus the base frame, identity
                       link transforms (body_frame_model); R from the body row's quaternion, h_w = R h, (m, h, Io) the body's entry of
                       the model - the base enters with base_mass / base_h / base_Io.  On fixed-base robots the route reproduces the
                       oracle-inverse matrices of jacobian_cases.oracle_M (asserted in the no-GPU half before anything else).
METRICS  e_J, e_M of jacobian_cases (e_M scale-free by sqrt(M_ii M_jj)).
TOLERANCES, per robot, by the project's rule: 10 x the worst deviation of the fp32 oracle's route from the reference over the robot's
inputs, rounded up to 1-2-5, at most 1e-4.  The fp32 route: Oracle("f32") rows and the congruence sum wholly in np.float32.
INPUTS per robot: KMAX[robot] envs from default_rng(SEED); every env has joint positions of its own inside the joint ranges (+-2
where there is none) and a base pose of its own - position within +-2 m, roll, pitch and yaw all non-zero -, joint rates +-0.1,
base twist +-0.1 m/s and +-0.1 rad/s, all rounded to fp32 before the references are taken.  An env's inputs do not depend on how many
envs there are.  Independent draws of the base orientation make neighbouring envs differ by far more than the tolerances in J (the
lever arms turn with the base) and in M (so does the base block) - asserted in the no-GPU half: a test that cannot tell env k from
env k + 1 would pass an index mix-up."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np

import jacobian_cases as jc
from scenes import build_scene
from test_gpu_step_matrix import round_up_125

SEED = 23
QD_AMP = 0.1
TWIST_AMP = 0.1
POS_AMP = 2.0
CAP = 1e-4
# robot -> (actors of the env, name of the robot actor, envs of the largest case)
ROBOTS = {
    "boxer": (["boxer"], "boxer", 130),
    "jackal_a": (["jackal_a"], "jackal_a", 65),
    "albert": (["albert"], "albert", 65),
    "anymal": (["anymal"], "anymal", 65),
}
STORE_EDGES = [("boxer", K) for K in (1, 63, 64, 65, 130)] + [(r, 65) for r in ("jackal_a", "albert", "anymal")]
# a contact scene with a free actor and a static one: the actors of boxer_push
PUSH_SCENE = ["boxer", "block", "paper_obst1"]
# the translation the results must not notice
FAR_SHIFT = (420.0, -310.0, 0.0)


def scene_of(robot):
    return build_scene(ROBOTS[robot][0], [[0.0, 0.0, 0.3]])


def euler_quat(roll, pitch, yaw):
    """xyzw of Rz(yaw) Ry(pitch) Rx(roll)"""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], axis=-1)


def draw_inputs(scene, kmax, seed=SEED):
    """-> (dof [kmax][2n] fp32 interleaved q, qd; roots [kmax][A][13] fp32, the robot's row a base pose and twist of the env's own)"""
    rng = np.random.default_rng(seed)
    bodies = scene.robot_model["bodies"]
    n = scene.n_dof
    lo = np.array([b["lower"] if b["limited"] else -2.0 for b in bodies])
    hi = np.array([b["upper"] if b["limited"] else 2.0 for b in bodies])
    # one row of unit draws per env, filled env by env: env k's inputs do not depend on kmax
    u = rng.uniform(0.0, 1.0, size=(kmax, 2 * n + 15))
    q = lo + (hi - lo) * u[:, 0:n]
    qd = QD_AMP * (2.0 * u[:, n:2 * n] - 1.0)
    pos = POS_AMP * (2.0 * u[:, 2 * n:2 * n + 3] - 1.0)
    sign = np.where(u[:, 2 * n + 3:2 * n + 6] < 0.5, -1.0, 1.0)
    rpy = sign * (0.2 + np.array([1.0, 1.0, 2.8]) * u[:, 2 * n + 6:2 * n + 9])   # roll, pitch 0.2 .. 1.2 rad, yaw 0.2 .. 3 rad, either sign
    twist = TWIST_AMP * (2.0 * u[:, 2 * n + 9:2 * n + 15] - 1.0)
    dof = np.zeros((kmax, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = q, qd
    _, root0 = scene.initial_state()
    roots = np.tile(np.asarray(root0, np.float32), (kmax, 1, 1))
    r = scene.robot_idx
    roots[:, r, 0:3], roots[:, r, 3:7], roots[:, r, 7:13] = pos, euler_quat(rpy[:, 0], rpy[:, 1], rpy[:, 2]), twist
    return dof, roots


@functools.lru_cache(maxsize=None)
def inputs(robot):
    """-> (dof [KMAX][2n], roots [KMAX][A][13]) fp32, read-only"""
    dof, roots = draw_inputs(scene_of(robot), ROBOTS[robot][2])
    dof.setflags(write=False)
    roots.setflags(write=False)
    return dof, roots


# ---- the oracle's routes ------------------------------------------------------------------------------------------------------------
def oracle_J(o, model, roots, q):
    """[K][n_rb][6][6 + n] in fp64 from the oracle of either precision: a unit base twist / a unit joint rate per column"""
    K, n = q.shape
    r = int(model.robot_actor)
    out = np.zeros((K, model.n_rb, 6, 6 + n))
    zero, eye = np.zeros(n), np.eye(n)
    for k in range(K):
        still = np.array(roots[k], np.float64)
        still[:, 7:13] = 0.0
        for c in range(6):
            root = still.copy()
            root[r, 7 + c] = 1.0
            out[k, :, :, c] = o.rigid_body_state(model, root, q[k], zero)[0][:, 7:13]
        for i in range(n):
            out[k, :, :, 6 + i] = o.rigid_body_state(model, still, q[k], eye[i])[0][:, 7:13]
    return out


def fixed_oracle_J(o, model, root, q):
    """the same with the root of a FIXED base (its root velocity is not propagated): the six base columns are left zero"""
    K, n = q.shape
    out = np.zeros((K, model.n_rb, 6, 6 + n))
    out[:, :, :, 6:] = jc.oracle_J(o, model, root, q)
    return out


def body_frame_model(model):
    """a copy of the ctypes model whose robot links are the n_bodies body frames (body = i) plus the base frame (body = -1), identity
    link transforms; n_links, n_rb, the robot actor's n_rb and first_rb of the later actors follow -> (copy, first rigid body of the robot)"""
    m = type(model)()
    C.memmove(C.byref(m), C.byref(model), C.sizeof(model))
    nb, a = int(m.n_bodies), int(m.robot_actor)
    for l in range(nb + 1):
        L = m.links[l]
        L.body = l if l < nb else -1
        for j in range(9):
            L.R[j] = 1.0 if j % 4 == 0 else 0.0
        for j in range(3):
            L.p[j] = 0.0
    delta = nb + 1 - int(m.actors[a].n_rb)
    first = int(m.actors[a].first_rb)
    m.n_links = nb + 1
    m.actors[a].n_rb = nb + 1
    m.n_rb = int(m.n_rb) + delta
    for b in range(int(m.n_actors)):
        if b != a and int(m.actors[b].first_rb) > first:
            m.actors[b].first_rb = int(m.actors[b].first_rb) + delta
    return m, first


def quat_R(quat, dtype):
    x, y, z, w = (dtype(v) for v in quat)
    one, two = dtype(1), dtype(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], dtype)


def skew(h):
    return np.array([[0, -h[2], h[1]], [h[2], 0, -h[0]], [-h[1], h[0], 0]], h.dtype)


def congruence_M(o, model, roots, q, moving, dtype=np.float64):
    """M [K][6 + n][6 + n] (moving) or [K][n][n]: sum_i J_i^T [[m 1, -[h_w]x], [[h_w]x, R Io R^T]] J_i over the oracle's Jacobians
    of the body frames, rows of the oracle `o`, every product and sum in `dtype`.  roots: [K][A][13] (moving) or [A][13]"""
    bm, first = body_frame_model(model)
    K, n = q.shape
    nb = int(model.n_bodies)
    sym = lambda Io: np.array([[Io[0], Io[1], Io[2]], [Io[1], Io[3], Io[4]], [Io[2], Io[4], Io[5]]], dtype)
    inert = [(dtype(model.bodies[i].mass), np.array(list(model.bodies[i].h), dtype), sym(list(model.bodies[i].Io))) for i in range(nb)]
    if moving:
        inert.append((dtype(model.base_mass), np.array(list(model.base_h), dtype), sym(list(model.base_Io))))
    J = (oracle_J(o, bm, roots, q) if moving else fixed_oracle_J(o, bm, roots, q)[:, :, :, 6:]).astype(dtype)
    N = J.shape[3]
    out = np.zeros((K, N, N), dtype)
    for k in range(K):
        root = np.array(roots[k] if moving else roots, np.float64)
        root[:, 7:13] = 0.0
        rows = o.rigid_body_state(bm, root, q[k], np.zeros(n))[0]
        for i, (m_i, h, Io) in enumerate(inert):
            R = quat_R(rows[first + i, 3:7], dtype)
            hw = R @ h
            I6 = np.zeros((6, 6), dtype)
            I6[0:3, 0:3] = m_i * np.eye(3, dtype=dtype)
            I6[0:3, 3:6] = -skew(hw)
            I6[3:6, 0:3] = skew(hw)
            I6[3:6, 3:6] = R @ Io @ R.T
            Ji = J[k, first + i]
            out[k] += Ji.T @ I6 @ Ji
    return out


def base_columns(rows, base_row):
    """[n_rows][6][6] = [[1, -[r]x], [0, 1]] in fp64 with r = p_row - p_base from rigid-body rows"""
    out = np.zeros((len(rows), 6, 6))
    for b, row in enumerate(rows):
        out[b] = np.eye(6)
        out[b, 0:3, 3:6] = -skew(np.asarray(row[0:3], np.float64) - np.asarray(base_row[0:3], np.float64))
    return out


e_J, e_M = jc.e_J, jc.e_M


def references_at(scene, model, roots, q):
    """-> namespace(J [K][n_rb][6][6+n], M [K][6+n][6+n], w32 = (e_J, e_M) of the fp32 route) at the given state, fp64"""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    roots, q = np.asarray(roots, np.float64), np.asarray(q, np.float64)
    J = oracle_J(o64, model, roots, q)
    M = congruence_M(o64, model, roots, q, True)
    w32 = (e_J(oracle_J(o32, model, roots, q), J), e_M(congruence_M(o32, model, roots, q, True, np.float32), M))
    for a in (J, M):
        a.setflags(write=False)
    a = int(model.robot_actor)
    first, L = int(model.actors[a].first_rb), int(model.actors[a].n_rb)
    robot_rb = np.zeros(int(model.n_rb), bool)
    robot_rb[first:first + L] = True
    return SimpleNamespace(scene=scene, model=model, J=J, M=M, w32=w32, first=first, L=L, robot_rb=robot_rb)


@functools.lru_cache(maxsize=None)
def references(robot):
    scene = scene_of(robot)
    dof, roots = inputs(robot)
    return references_at(scene, scene.to_c(), roots, dof[:, 0::2])


def tolerances_from(w32):
    return min(round_up_125(10.0 * w32[0]), CAP), min(round_up_125(10.0 * w32[1]), CAP)


def tolerances(robot):
    """-> (tol_J, tol_M)"""
    return tolerances_from(references(robot).w32)


def generalised_velocity(dof, roots, robot_actor):
    """v [K][6 + n] = (root linvel, root angvel, qd)"""
    return np.concatenate([np.asarray(roots, np.float64)[:, robot_actor, 7:13], np.asarray(dof, np.float64)[:, 1::2]], axis=1)
