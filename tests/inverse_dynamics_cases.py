"""Inputs, references, metric and tolerances of the inverse-dynamics tests (test_inverse_dynamics.py, no GPU;
test_gpu_inverse_dynamics.py): mppi_sim_inverse_dynamics (csrc/mppi_kernels.hpp k_sim_inverse_dynamics, csrc/mppi_device.hpp
inverse_dynamics) against the fp64 oracle, every env, every joint, every combination of terms.

INPUTS per robot: the robots, envs and joint positions of jacobian_cases.inputs with gravity switched ON for the robot
(scene.robot.gravity = True: the shipped arm actors restate `gravity: false`), joint rates uniform in +-QD_AMP = 1 and joint
accelerations uniform in +-QDD_AMP = 3 from default_rng(SEED) (the +-0.1 rates of jacobian_cases make the velocity term too small
to tell apart).  An env's inputs do not depend on how many envs there are.  Base poses: the origin; TILTED - at jc.OFFSET_POS, yawed
by 0.7 rad and then rolled by 0.4 rad, so that gravity lies along no axis of the base -; and, for the mobile manipulator, FAR - its
prismatic base joints +-420 m out in every env.
REFERENCE, always fp64, from the oracle as it stands:  tau_ref = M_ref (qdd - FD(q, qd, 0))  with M_ref = jacobian_cases.oracle_M
(the fp64 inverse of the oracle's M^-1) and FD = Oracle("f64").forward_dynamics on the model with gravity on.  The parts come
from the same route with qd = 0 and / or qdd = 0:  g = -M FD(q, 0, 0),  C qd = -M FD(q, qd, 0) - g,  M qdd.
METRIC  e_tau = max over envs and joints of |tau - tau_ref|[k, j] / D_j,  D_j = max_k |tau_ref[k, j]| of the FULL-term reference over
the robot's inputs at that base pose: a per-joint torque scale (57 N m at the Panda's shoulder, 0.07 at its last wrist joint).
Calls with fewer terms are measured against the same D_j.
TOLERANCE, per robot, by the project's rule: 10 x the worst e_tau of an fp32 RESTATEMENT from tau_ref - over the robot's base poses,
the four combinations of terms and qdd given or left out -, rounded up to 1-2-5, at most CAP = 1e-4.  The restatement
(newton_euler below) is a body-frame 3-vector Newton-Euler pass over the robot's JSON model in numpy float32 on fp32-rounded
inputs - deliberately not the kernel's world-axes formulation, and never the code under test."""
import ctypes as C
import functools

import numpy as np

import jacobian_cases as jc
from scenes import build_scene
from test_gpu_step_matrix import round_up_125

SEED = 21
QD_AMP, QDD_AMP = 1.0, 3.0
CAP = 1e-4
ID_GRAVITY, ID_VELOCITY = 1, 2
# (terms, qdd given): the full call, qdd NULL with both terms, gravity only, velocity only, qdd only; then the remaining combinations
FULL = (ID_GRAVITY | ID_VELOCITY, True)
CALLS = [FULL, (ID_GRAVITY | ID_VELOCITY, False), (ID_GRAVITY, False), (ID_VELOCITY, False), (0, True)]
ALL_CALLS = CALLS + [(ID_GRAVITY, True), (ID_VELOCITY, True), (0, False)]
ROBOTS = jc.ROBOTS
STORE_EDGES = jc.STORE_EDGES
TILT_YAW, TILT_ROLL = jc.OFFSET_YAW, 0.4
_cz, _sz, _cx, _sx = np.cos(TILT_YAW / 2), np.sin(TILT_YAW / 2), np.cos(TILT_ROLL / 2), np.sin(TILT_ROLL / 2)
TILT_ORI = [float(_cz * _sx), float(_sz * _sx), float(_cx * _sz), float(_cz * _cx)]      # q_z(yaw) q_x(roll), xyzw
FAR = 420.0
POSES = {r: ("origin", "tilted") + (("far",) if r == "omnipanda" else ()) for r in ROBOTS}


def quat_to_R(q):
    """rotation of a quaternion xyzw that need not be of unit length (the root rows hold it rounded to fp32), as the oracle takes it"""
    x, y, z, w = (float(v) for v in q)
    s = 2.0 / (x * x + y * y + z * z + w * w)
    return np.array([[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                     [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                     [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]])


def scene_of(robot, pose="origin", gravity=True):
    tilted = pose == "tilted"
    scene = build_scene(ROBOTS[robot][0], [jc.OFFSET_POS if tilted else [0.0, 0.0, 0.0]], robot_overrides={"init_ori": TILT_ORI} if tilted else None)
    scene.robot.gravity = gravity
    return scene


@functools.lru_cache(maxsize=None)
def inputs(robot, pose="origin"):
    """-> (dof [KMAX][2n] fp32 interleaved q, qd; qdd [KMAX][n] fp32), read-only"""
    dof0, _ = jc.inputs(robot)
    kmax, n = dof0.shape[0], dof0.shape[1] // 2
    rng = np.random.default_rng(SEED)
    dof = np.array(dof0)
    dof[:, 1::2] = rng.uniform(-QD_AMP, QD_AMP, size=(kmax, n))
    qdd = rng.uniform(-QDD_AMP, QDD_AMP, size=(kmax, n)).astype(np.float32)
    if pose == "far":        # the two prismatic base joints of the mobile manipulator (x, y), alternating signs
        bodies = scene_of(robot).robot_model["bodies"]
        assert [b["jtype"] for b in bodies[:2]] == ["prismatic", "prismatic"]
        sign = np.where(np.arange(kmax) % 2 == 0, 1.0, -1.0)
        dof[:, 0], dof[:, 2] = FAR * sign, -FAR * sign
    dof.setflags(write=False)
    qdd.setflags(write=False)
    return dof, qdd


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def reference_parts(o64, model, root, q, qd, qdd):
    """-> dict of the three parts 'M' (M qdd), 'C' (C qd), 'g', each [K][n] in fp64, by the route of the module docstring"""
    q, qd, qdd = (np.asarray(a, np.float64) for a in (q, qd, qdd))
    K, n = q.shape
    M = jc.oracle_M(o64, model, root, q)
    zero = np.zeros(n)
    g, Cg, Mq = np.zeros((K, n)), np.zeros((K, n)), np.zeros((K, n))
    for k in range(K):
        g[k] = -M[k] @ o64.forward_dynamics(model, root, q[k], zero, zero)
        Cg[k] = -M[k] @ o64.forward_dynamics(model, root, q[k], qd[k], zero)
        Mq[k] = M[k] @ qdd[k]
    return {"M": Mq, "C": Cg - g, "g": g}


def combine(parts, terms, with_qdd):
    """tau of one call from the three parts"""
    out = np.zeros_like(parts["g"])
    if with_qdd:
        out = out + parts["M"]
    if terms & ID_VELOCITY:
        out = out + parts["C"]
    if terms & ID_GRAVITY:
        out = out + parts["g"]
    return out


def scale(parts):
    """D_j: the per-joint torque scale of the full-term reference"""
    return np.abs(combine(parts, *FULL)).max(0)


def e_tau(tau, tau_ref, D):
    return float((np.abs(np.asarray(tau, np.float64) - tau_ref) / D[None, :]).max())


# ---- the fp32 restatement -----------------------------------------------------------------------------------------------------------
def _rot_axis(a, q, f):
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f)
    return np.eye(3, dtype=f) + np.sin(q) * Kx + (f(1) - np.cos(q)) * (Kx @ Kx)


def newton_euler(model_json, q, qd, qdd, g_base, f=np.float32):
    """tau [n] = M qdd + C qd + g by the classic Newton-Euler recursion with 3-vectors in BODY frames (Luh-Walker-Paul), every
    operation in precision f on inputs rounded to f.  g_base: gravity in the axes of the (fixed) base."""
    bodies = model_json["bodies"]
    n = len(bodies)
    q, qd, qdd = (np.asarray(a, f) for a in (q, qd, qdd))
    R, p, w, wd, a, F, N = ([None] * n for _ in range(7))
    zero = np.zeros(3, f)
    for i, b in enumerate(bodies):
        ax, Rt, pt = np.asarray(b["axis"], f), np.asarray(b["R_tree"], f), np.asarray(b["p_tree"], f)
        par = b["parent"]
        rev = b["jtype"] == "revolute"
        R[i], p[i] = (Rt @ _rot_axis(ax, q[i], f), pt) if rev else (Rt, pt + (Rt @ ax) * q[i])
        wp, wdp, ap = (zero, zero, -np.asarray(g_base, f)) if par < 0 else (w[par], wd[par], a[par])
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
        m = f(I["mass"])
        h = np.asarray(I["h"], f)
        c = h / m if m > 0 else zero
        Io = np.array([[I["Io"][0], I["Io"][1], I["Io"][2]], [I["Io"][1], I["Io"][3], I["Io"][4]], [I["Io"][2], I["Io"][4], I["Io"][5]]], f)
        Ic = Io - m * ((c @ c) * np.eye(3, dtype=f) - np.outer(c, c))
        F[i] = m * (a[i] + np.cross(wd[i], c) + np.cross(w[i], np.cross(w[i], c)))
        N[i] = Ic @ wd[i] + np.cross(w[i], Ic @ w[i]) + np.cross(c, F[i])
        assert all(v.dtype == f for v in (R[i], p[i], w[i], wd[i], a[i], F[i], N[i]))
    tau = np.zeros(n, f)
    for i in reversed(range(n)):
        b = bodies[i]
        tau[i] = (N[i] if b["jtype"] == "revolute" else F[i]) @ np.asarray(b["axis"], f)
        if b["parent"] >= 0:
            fp = R[i] @ F[i]
            F[b["parent"]] = F[b["parent"]] + fp
            N[b["parent"]] = N[b["parent"]] + R[i] @ N[i] + np.cross(p[i], fp)
    return tau


def gravity_in_base(model, root):
    """the model's gravity (zero when the robot's actor has it off) in the axes of the robot's base"""
    on = bool(model.actors[model.robot_actor].gravity)
    g = np.array([model.gravity[j] for j in range(3)]) if on else np.zeros(3)
    return quat_to_R(np.asarray(root, np.float64).reshape(-1, 13)[model.robot_actor, 3:7]).T @ g


def restated(model_json, g_base, dof, qdd, terms, with_qdd, f=np.float32):
    """[K][n]: newton_euler of every env for one call (a part that is not asked for has its input zeroed)"""
    q, qd = dof[:, 0::2], dof[:, 1::2]
    zero = np.zeros(q.shape[1])
    return np.stack([newton_euler(model_json, q[k], qd[k] if terms & ID_VELOCITY else zero, qdd[k] if with_qdd else zero,
                                  g_base if terms & ID_GRAVITY else np.zeros(3), f) for k in range(len(q))])


# ---- references and tolerances ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def references(robot, pose="origin"):
    """-> (scene, model, root, parts, D, worst fp32-restatement e_tau over ALL_CALLS) at the robot's inputs and base pose"""
    from oracle.oracle import Oracle
    o64 = Oracle("f64")
    scene = scene_of(robot, pose)
    model = scene.to_c()
    _, root = scene.initial_state()
    dof, qdd = inputs(robot, pose)
    parts = reference_parts(o64, model, root, dof[:, 0::2], dof[:, 1::2], qdd)
    for a in parts.values():
        a.setflags(write=False)
    D = scale(parts)
    gb = gravity_in_base(model, root)
    w32 = max(e_tau(restated(scene.robot_model, gb, dof, qdd, t, wq), combine(parts, t, wq), D) for t, wq in ALL_CALLS)
    return scene, model, root, parts, D, w32


@functools.lru_cache(maxsize=None)
def restatement_worst(robot):
    return max(references(robot, pose)[5] for pose in POSES[robot])


def tolerance_from(worst32):
    return min(round_up_125(10.0 * worst32), CAP)


def tolerance(robot):
    return tolerance_from(restatement_worst(robot))


# ---- stepping the oracle (rows 9 and 10) --------------------------------------------------------------------------------------------
def oracle_envs_step(o, model, dof, root, u, steps=1):
    """orc_envs_step from per-env dof [K][2n] and one root [A][13] under the constant per-env commands u [K][nu] -> dof after every
    step [steps][K][2n], fp64"""
    f = o.dtype
    K = len(dof)
    dof = np.ascontiguousarray(dof, f).copy()
    roots = np.ascontiguousarray(np.tile(np.asarray(root, f).reshape(1, model.n_actors, 13), (K, 1, 1)))
    rb, cf = np.zeros((K, model.n_rb, 13), f), np.zeros((K, model.n_rb, 3), f)
    u = np.ascontiguousarray(u, f)
    out = []
    for _ in range(steps):
        o.lib.orc_envs_step(C.byref(model), C.c_int(K), C.c_int(0), o.p(u), o.p(dof), o.p(roots), o.p(rb), o.p(cf))
        out.append(dof.astype(np.float64))
    return np.stack(out)


# an effort-driven Panda under gravity: K = 65 of the Panda's poses.  HOLD: at rest, 20 steps under g(q).  TORQUE: rates +-0.3,
# accelerations +-1 (by the torque scales above |tau| stays below 0.9 of every effort limit, test_inverse_dynamics.py checks it),
# one step of a one-substep copy of the preset, the poses drawn in by 5 % towards the middle of every joint range so that no
# joint stands within a step of its limit
HOLD_K, HOLD_STEPS = 65, 20
TORQUE_QD_AMP, TORQUE_QDD_AMP, TORQUE_Q_SHRINK = 0.3, 1.0, 0.95
EFFORT_ACTOR = {"type": "robot", "name": "panda", "dof_mode": "effort", "fixed": True, "flip_visual": True, "gravity": True,
                "init_joint_pose": [0.0, 0, -0.94, 0, 0.0, 0, -2.8, 0, 0.0, 0, 1.8675, 0, 0.0, 0],
                "urdf_file": "panda_isaac/robots/franka_panda.urdf", "visualize_link": "panda_link7"}


@functools.lru_cache(maxsize=None)
def actor_file(gravity=True, dof_mode="effort", urdf="panda_isaac/robots/franka_panda.urdf", name="panda"):
    """an actor YAML of the tests' own (the shipped arm actors carry `gravity: false`) -> its path, as an entry of an actor list"""
    import os
    import tempfile
    import yaml
    d = tempfile.mkdtemp(prefix="inverse_dynamics_cases_")
    path = os.path.join(d, f"{name}_{dof_mode}_{'g' if gravity else 'nog'}.yaml")
    with open(path, "w") as fh:
        yaml.safe_dump(dict(EFFORT_ACTOR, gravity=gravity, dof_mode=dof_mode, urdf_file=urdf, name=name), fh)
    return path


@functools.lru_cache(maxsize=None)
def gravity_actor(name):
    """the shipped actor `name` with `gravity: true`, as a file of the tests' own -> its path (an entry of an actor list)"""
    import os
    import tempfile
    import yaml
    from mppiisaac.utils.isaacgym_utils import CONF_DIR
    with open(os.path.join(CONF_DIR, "actors", f"{name}.yaml")) as fh:
        fields = yaml.safe_load(fh)
    fields["gravity"] = True
    path = os.path.join(tempfile.mkdtemp(prefix="inverse_dynamics_cases_"), f"{name}_gravity.yaml")
    with open(path, "w") as fh:
        yaml.safe_dump(fields, fh)
    return path


def effort_scene(substeps=2):
    return build_scene([actor_file()], [[0.0, 0.0, 0.0]], overrides={"substeps": substeps})


@functools.lru_cache(maxsize=None)
def hold_case():
    """-> (scene, model, root, dof0 [K][2n] at rest, g_ref [K][n], bound on |q - q0| after every one of the 20 steps, sag under a zero
    command).  Bound: 10 x the drift of the fp32 oracle stepped under the fp32-rounded g_ref, rounded up to 1-2-5."""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    scene = effort_scene()
    model = scene.to_c()
    _, root = scene.initial_state()
    dof = np.array(jc.inputs("franka_panda")[0][:HOLD_K])
    dof[:, 1::2] = 0.0
    n = scene.n_dof
    parts = reference_parts(o64, model, root, dof[:, 0::2], np.zeros((HOLD_K, n)), np.zeros((HOLD_K, n)))
    g_ref = parts["g"]
    still = oracle_envs_step(o64, model, dof, root, g_ref, HOLD_STEPS)
    drift64 = np.abs(still[:, :, 0::2] - dof[None, :, 0::2].astype(np.float64)).max()
    moved32 = oracle_envs_step(o32, model, dof, root, g_ref.astype(np.float32), HOLD_STEPS)
    drift32 = np.abs(moved32[:, :, 0::2] - dof[None, :, 0::2].astype(np.float64)).max()
    sag = oracle_envs_step(o64, model, dof, root, np.zeros((HOLD_K, n)), HOLD_STEPS)
    sag = np.abs(sag[:, :, 0::2] - dof[None, :, 0::2].astype(np.float64)).max((0, 2))      # per env, within the 20 steps
    return scene, model, root, dof, g_ref, round_up_125(10.0 * drift32), sag, drift64, drift32


@functools.lru_cache(maxsize=None)
def torque_case():
    """-> (scene, model, root, dof [K][2n], qdd [K][n], tau_ref [K][n], command [K][n], dof after one step of the fp64 oracle).
    One substep: h = dt.  The effort drive is  target - kd qd'  with the rate qd' at the END of the substep (implicit), so the
    command  tau + kd (qd + h qdd)  leaves the joints exactly tau when they accelerate by qdd."""
    from oracle.oracle import Oracle
    o64 = Oracle("f64")
    scene = effort_scene(substeps=1)
    model = scene.to_c()
    _, root = scene.initial_state()
    K, n = HOLD_K, scene.n_dof
    rng = np.random.default_rng(SEED + 1)
    dof = np.array(jc.inputs("franka_panda")[0][:K])
    bodies = scene.robot_model["bodies"]
    mid = np.array([0.5 * (b["lower"] + b["upper"]) for b in bodies])
    dof[:, 0::2] = mid + TORQUE_Q_SHRINK * (dof[:, 0::2] - mid)       # (the drawn poses reach the very ends of the joint ranges)
    dof[:, 1::2] = rng.uniform(-TORQUE_QD_AMP, TORQUE_QD_AMP, size=(K, n))
    qdd = rng.uniform(-TORQUE_QDD_AMP, TORQUE_QDD_AMP, size=(K, n)).astype(np.float32)
    parts = reference_parts(o64, model, root, dof[:, 0::2], dof[:, 1::2], qdd)
    tau_ref = combine(parts, *FULL)
    kd, h = float(model.drive_kd), float(model.dt) / int(model.substeps)
    cmd = tau_ref + kd * (dof[:, 1::2].astype(np.float64) + h * qdd.astype(np.float64))
    after = oracle_envs_step(o64, model, dof, root, cmd, 1)[0]
    return scene, model, root, dof, qdd, tau_ref, cmd, after
