"""Inputs, references, metrics and tolerances of the link-Jacobian / mass-matrix tests (test_jacobian_mass.py, no GPU;
test_gpu_jacobian_mass.py): mppi_sim_jacobian and mppi_sim_mass_matrix (csrc/mppi_kernels.hpp k_sim_jacobian, k_sim_mass_matrix)
against the fp64 oracle, every env, every body, every entry.

REFERENCE, always fp64, at the joint positions the simulator itself holds (its dof tensor read back and widened):
  J_ref[:, :, i] = columns 7:13 of Oracle("f64").rigid_body_state(model, root, q, e_i) - the rigid-body velocity columns are linear
                   in qd, so a unit joint rate yields the Jacobian column exactly;
  M_ref          = for the envs that sit at a joint position of tests/golden/mass_matrices.json the matrix stored there (computed
                   from the URDF by an independent route, permuted as tests/test_mass_matrix_golden.py does); elsewhere the fp64
                   inverse of the oracle's M^-1, column by column: M^-1 e_i = qdd(tau = e_i) - qdd(tau = 0) at qd = 0.
METRICS  e_J = max |J - J_ref| (lever arms in metres, unit axes);  e_M = max_ij |M - M_ref|_ij / sqrt(M_ref,ii M_ref,jj).
TOLERANCES, per robot, from the oracle alone (the rule of test_gpu_step_matrix.py): 10 x the worst deviation of the fp32 oracle's
route (J from Oracle("f32").rigid_body_state, M the fp64 inverse of the fp32 oracle's M^-1) from the reference over the robot's
inputs below, rounded up to 1-2-5, at most 1e-4.

INPUTS per robot: KMAX[robot] envs; envs 0-2 sit at the three joint positions of the fixture (rounded to fp32: what the simulator
holds - the fixture's matrix is then off by that rounding, and so is the fp32 route the tolerance comes from), every other env at a
draw of default_rng(SEED) inside the joint ranges (joints without a range: +-2), ordered as inputs() says.  An env's inputs do not
depend on how many envs there are.  The Panda is also placed away from the origin (OFFSET_POS, OFFSET_YAW).
Joint rates +-QD_AMP, for J qd against the rb rows of mppi_sim_materialise: those rows are velocity sums about the WORLD origin
in fp32, each term rounded at 2^-24 |p| |qd| - 2.5e-6 at the 420 m of the mobile manipulator's fixture positions and 0.1 rad/s, a
dozen terms per row -, which has to stay inside the step matrix's velocity tolerance (5e-5) that the comparison grants them."""
import functools
import json
import os
import tempfile

import numpy as np

from scenes import build_scene
from test_gpu_step_matrix import round_up_125

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = {os.path.basename(r["urdf_file"]): r for r in json.load(open(os.path.join(HERE, "golden", "mass_matrices.json")))["robots"]}
SEED = 20
QD_AMP = 0.1
CAP = 1e-4
# robot -> (actors of the env, name of the robot actor, fixture entry, envs of the largest case)
ROBOTS = {
    "franka_panda": (["panda"], "panda", "franka_panda.urdf", 130),
    "panda_gripper": (["panda_gripper"], "panda", "franka_panda_gripper.urdf", 65),
    "point_robot": (["point_robot"], "point_robot", "point_robot.urdf", 65),
    "heijn": (["heijn"], "heijn", "heijn.urdf", 65),
    "omnipanda": (["omnipanda"], "omnipanda", "omniPandaWithGripper.urdf", 65),
}
STORE_EDGES = [("franka_panda", K) for K in (1, 63, 64, 65, 130)] + [(r, 65) for r in ("panda_gripper", "point_robot", "heijn", "omnipanda")]
# the gripper scene (a contact-scene context with a fixed-base robot): the robot's inputs are those of panda_gripper
GRIPPER_SCENE = ["panda_gripper", "panda_pick_block", "table"]
# the Panda's base 2 m and -2 m off in x and y, yawed by 0.7 rad
OFFSET_POS, OFFSET_YAW = [2.0, -2.0, 0.0], 0.7
OFFSET_ORI = [0.0, 0.0, float(np.sin(OFFSET_YAW / 2)), float(np.cos(OFFSET_YAW / 2))]


def scene_of(robot, offset=False):
    actors = ROBOTS[robot][0]
    return build_scene(actors, [OFFSET_POS if offset else [0.0, 0.0, 0.0]], robot_overrides={"init_ori": OFFSET_ORI} if offset else None)


@functools.lru_cache(maxsize=None)
def two_point_robot_actors():
    """actor list of an env of TWO fixed-base point robots (one forest, n_dof = 6), the second one described by a file of its own"""
    import yaml
    d = tempfile.mkdtemp(prefix="jacobian_cases_")
    second = os.path.join(d, "point_robot2.yaml")
    with open(second, "w") as f:
        yaml.safe_dump({"type": "robot", "name": "point_robot2", "fixed": True, "urdf_file": "point_robot.urdf"}, f)
    return ("point_robot", second), [[0.0, 0.0, 0.05], [1.0, -0.5, 0.05]]


@functools.lru_cache(maxsize=None)
def inputs(robot):
    """-> (dof [KMAX][2n] fp32 interleaved q, qd; number of leading envs that sit at the fixture's joint positions), read-only"""
    scene = scene_of(robot)
    _, _, urdf, kmax = ROBOTS[robot]
    gold = GOLD[urdf]
    perm = [gold["joints"].index(n) for n in scene.dof_names]
    rng = np.random.default_rng(SEED)
    bodies = scene.robot_model["bodies"]
    lo = np.array([b["lower"] if b["limited"] else -2.0 for b in bodies])
    hi = np.array([b["upper"] if b["limited"] else 2.0 for b in bodies])
    q = rng.uniform(lo, hi, size=(kmax, scene.n_dof))
    # the ORDER of the drawn envs: sorted by the angle of the robot's first revolute joint, then the two halves interleaved, so
    # that neighbours stand about half a turn apart there.  The mass matrix of the planar bases (heijn: x, y, yaw) depends on
    # the yaw alone, and by 1e-3 (scale-free) at most: among 64 independent draws some neighbours always fall within 100
    # tolerances of each other (none of 300 seeds tried avoids it) - and a test that cannot tell env k from env k + 1 would
    # pass an index mix-up
    first_rev = next(i for i, b in enumerate(bodies) if b["jtype"] != "prismatic")
    order = np.argsort(np.mod(q[:, first_rev], 2 * np.pi), kind="stable")
    half = (kmax + 1) // 2
    q = q[np.ravel(np.column_stack([order[:half], np.resize(order[half:], half)]))[:kmax]] if kmax > 1 else q
    qd = rng.uniform(-QD_AMP, QD_AMP, size=(kmax, scene.n_dof))
    for k, case in enumerate(gold["cases"]):
        q[k] = np.asarray(case["q"])[perm]
    dof = np.zeros((kmax, 2 * scene.n_dof), np.float32)
    dof[:, 0::2], dof[:, 1::2] = q, qd
    dof.setflags(write=False)
    return dof, len(gold["cases"])


def golden_M(robot, scene):
    gold = GOLD[ROBOTS[robot][2]]
    perm = [gold["joints"].index(n) for n in scene.dof_names]
    return [np.asarray(case["M"])[np.ix_(perm, perm)] for case in gold["cases"]]


# ---- the oracle's routes ------------------------------------------------------------------------------------------------------------
def oracle_J(o, model, root, q):
    """[K][n_rb][6][n] in fp64 from the oracle of either precision: column i = the rb velocity columns under the unit rate e_i"""
    K, n = q.shape
    out = np.zeros((K, model.n_rb, 6, n))
    eye = np.eye(n)
    for k in range(K):
        for i in range(n):
            out[k, :, :, i] = o.rigid_body_state(model, root, q[k], eye[i])[0][:, 7:13]
    return out


def oracle_M(o, model, root, q):
    """[K][n][n]: the fp64 inverse of the oracle's M^-1 (either precision), column by column"""
    K, n = q.shape
    out = np.zeros((K, n, n))
    zero, eye = np.zeros(n), np.eye(n)
    for k in range(K):
        g = o.forward_dynamics(model, root, q[k], zero, zero).astype(np.float64)
        Minv = np.stack([o.forward_dynamics(model, root, q[k], zero, eye[i]).astype(np.float64) - g for i in range(n)], axis=1)
        out[k] = np.linalg.inv(Minv)
    return out


def reference_M(o64, model, root, q, golden=()):
    """M_ref [K][n][n]: the URDF-route matrices for the leading envs that sit at the fixture's joint positions, the oracle's elsewhere"""
    M = oracle_M(o64, model, root, q)
    for k, G in enumerate(golden):
        if k < len(M):
            M[k] = G
    return M


def e_J(J, J_ref):
    return float(np.abs(np.asarray(J, np.float64) - J_ref).max())


def e_M(M, M_ref):
    d = np.sqrt(np.einsum("kii->ki", M_ref))
    return float((np.abs(np.asarray(M, np.float64) - M_ref) / (d[:, :, None] * d[:, None, :])).max())


@functools.lru_cache(maxsize=None)
def references(robot, offset=False):
    """-> (scene, model, root, J_ref, M_ref, fp32-route e_J, fp32-route e_M) at the robot's inputs, base at the origin or at OFFSET"""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    scene = scene_of(robot, offset)
    model = scene.to_c()
    _, root = scene.initial_state()
    dof, n_gold = inputs(robot)
    q = dof[:, 0::2].astype(np.float64)
    J_ref = oracle_J(o64, model, root, q)
    M_ref = reference_M(o64, model, root, q, golden_M(robot, scene)[:n_gold])
    for a in (J_ref, M_ref):
        a.setflags(write=False)
    return scene, model, root, J_ref, M_ref, e_J(oracle_J(o32, model, root, q), J_ref), e_M(oracle_M(o32, model, root, q), M_ref)


@functools.lru_cache(maxsize=None)
def oracle32_worst(robot):
    """worst fp32-route deviation (e_J, e_M) over the robot's inputs - for the Panda at both base poses"""
    runs = [references(robot)] + ([references(robot, True)] if robot == "franka_panda" else [])
    return max(r[5] for r in runs), max(r[6] for r in runs)


def tolerances(robot):
    """-> (tol_J, tol_M)"""
    wJ, wM = oracle32_worst(robot)
    return min(round_up_125(10.0 * wJ), CAP), min(round_up_125(10.0 * wM), CAP)


# the step matrix's tolerances of the rb velocity columns of a contact-free / a contact scene (for J qd against the rb tensor)
def velocity_tolerances(contact=False):
    from test_gpu_step_matrix import TOL
    t = TOL["contact" if contact else "free"]
    return t["lin"], t["ang"]
