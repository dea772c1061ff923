"""Inputs, references, metrics and tolerances of the moving-base forward-dynamics tests (test_floating_forward_dynamics.py, no GPU;
test_gpu_floating_forward_dynamics.py): mppi_sim_floating_forward_dynamics (csrc/mppi_kernels.hpp k_sim_floating_forward_dynamics,
csrc/mppi_device.hpp floating_forward_dynamics) against an fp64 reference built from what the oracle exports, every env, every row,
every combination of terms.

GENERALISED VELOCITY  v = (root linvel, root angvel, qd) of floating_jacobian_cases; tau the force dual to v (rows 0:3 the force on
the base, rows 3:6 the moment about the base origin, world axes, then the joints), vd the time derivative of v.
INPUTS per robot: the robots, env counts, poses, rates and vd* (+-3) of floating_inverse_dynamics_cases.inputs; tau is the fp64 full
reference tau of that module at vd*, rounded to fp32 - so vd_ref is O(1) in every row (D_j >= 1, asserted by the no-GPU half).
REFERENCE, always fp64, at the state the simulator holds, per call:
    vd_ref = solve(M_ref, tau (zero when left out) - C (with ID_VELOCITY) - g (with ID_GRAVITY))
  M_ref    floating_jacobian_cases.congruence_M;
  C, g     floating_inverse_dynamics_cases.reference_parts (its 'M' part is not used).
  It is believed only after the no-GPU half has shown that the same route on the fixed-base mobile manipulator and heijn
  (fixed_parts, jacobian_cases.oracle_M) reproduces Oracle("f64").forward_dynamics within FIXED_ROUTE_AGREE, and that
  M_ref vd_ref + bias returns the fp32 tau within SOLVE_RESIDUAL.
METRICS, as in forward_dynamics_cases:
  (a) e_vd  = max |vd - ref|[k, j] / D_j,  D_j = max_k |ref_full[k, j]|;
  (b) e_res = max |M_ref (vd - ref)|[k, j] / Dtau_j,  Dtau the floored per-unit scale of floating_inverse_dynamics_cases.scale on the
      full tau.
  Calls with fewer terms are measured on the same scales.
TOLERANCES, per robot and metric, by the project's rule: 10 x the worst deviation of an fp32 RESTATEMENT over the eight calls, rounded
up to 1-2-5; at most forward_dynamics_cases.CAP_QDD = 1e-3 for (a) and floating_inverse_dynamics_cases.CAP = 1e-4 for (b).  The
restatement is deliberately not the routine under test: congruence_M in np.float32, the bias from
floating_inverse_dynamics_cases.restated in fp32, np.linalg.solve in float32.
COLUMNS of M^-1 (terms = 0, tau = e_c): |col - ref|[j, c] / sqrt(Minv_ref[j, j] Minv_ref[c, c]); tolerance from the fp32 dense inverse
of the fp32 congruence_M by the same rule, at most CAP_QDD."""
import functools
from types import SimpleNamespace

import numpy as np

import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
import forward_dynamics_cases as fd
from test_gpu_step_matrix import round_up_125

CAP_QDD = fd.CAP_QDD
CAP_RES = fi.CAP
# measured on the CPU (test_floating_forward_dynamics.py prints them): the fixed-base route against Oracle("f64").forward_dynamics in
# e_qdd 1.6e-11 at worst (the mobile manipulator's calls with the velocity part: the Richardson difference behind C agrees to 3e-12
# in torque and the solve amplifies it by the conditioning of the arm; 6e-13 without it, 2.6e-14 on heijn);
# |M_ref vd_ref + bias - tau| / Dtau 3.8e-16 at worst (anymal).  The next 1-2-5 step above each:
FIXED_ROUTE_AGREE = 2e-11
SOLVE_RESIDUAL = 5e-16
ID_GRAVITY, ID_VELOCITY = fi.ID_GRAVITY, fi.ID_VELOCITY
FULL, CALLS, ALL_CALLS = fi.FULL, fi.CALLS, fi.ALL_CALLS
ROBOTS = fi.ROBOTS
STORE_EDGES = fi.STORE_EDGES
PUSH_SCENE = fi.PUSH_SCENE
FAR_SHIFT = fi.FAR_SHIFT
SEED = fi.SEED
scene_of = fi.scene_of


@functools.lru_cache(maxsize=None)
def inputs(robot):
    """-> (dof [KMAX][2n], roots [KMAX][A][13], tau [KMAX][6 + n]) fp32, read-only: tau the full reference tau of
    floating_inverse_dynamics_cases at its vd*"""
    dof, roots, _ = fi.inputs(robot)
    tau = fi.combine(fi.references(robot).parts, *fi.FULL).astype(np.float32)
    tau.setflags(write=False)
    return dof, roots, tau


def tau_for(scene, model, roots, dof, vd):
    """the fp32 tau that asks for vd at a state of its own (a scene, a live state): the full fp64 reference tau there, rounded"""
    r = fi.references_at(scene, model, roots, dof, vd)
    return fi.combine(r.parts, *fi.FULL).astype(np.float32)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def solve_calls(M, C, g, tau, calls=ALL_CALLS):
    """{call: [K][N]} = solve(M, tau (given) - C (velocity) - g (gravity)) in the precision of the arguments"""
    out = {}
    for terms, with_tau in calls:
        rhs = np.zeros_like(C)
        if with_tau:
            rhs = rhs + tau
        if terms & ID_VELOCITY:
            rhs = rhs - C
        if terms & ID_GRAVITY:
            rhs = rhs - g
        out[terms, with_tau] = np.linalg.solve(M, rhs[:, :, None])[:, :, 0]
        assert out[terms, with_tau].dtype == C.dtype
    return out


def e_vd(vd, ref, D):
    return float((np.abs(np.asarray(vd, np.float64) - ref) / D[None, :]).max())


def e_res(vd, ref, M_ref, Dtau):
    r = np.einsum("kij,kj->ki", M_ref, np.asarray(vd, np.float64) - ref)
    return float((np.abs(r) / Dtau[None, :]).max())


def measure(got, r):
    """{call: (e_vd, e_res)} of the results `got` {call: [K][N]} against the references r"""
    return {c: (e_vd(got[c], r.ref[c], r.D), e_res(got[c], r.ref[c], r.M, r.Dtau)) for c in got}


def restated_calls(scene, model, roots32, dof32, tau32, calls=ALL_CALLS):
    """the fp32 restatement: congruence_M in np.float32, the bias of floating_inverse_dynamics_cases.restated in fp32, a dense fp32 solve"""
    from oracle.oracle import Oracle
    K, n = dof32.shape[0], dof32.shape[1] // 2
    M32 = fc.congruence_M(Oracle("f32"), model, np.asarray(roots32, np.float64), dof32[:, 0::2].astype(np.float64), True, np.float32)
    zero = np.zeros((K, 6 + n), np.float32)
    C32 = fi.restated(scene.robot_model, model, roots32, dof32, zero, ID_VELOCITY, False)
    g32 = fi.restated(scene.robot_model, model, roots32, dof32, zero, ID_GRAVITY, False)
    assert M32.dtype == C32.dtype == g32.dtype == np.float32
    return solve_calls(M32, C32, g32, np.asarray(tau32, np.float32), calls), M32


def references_at(scene, model, roots, dof, tau):
    """-> namespace(ref {call: vd [K][6 + n]}, M, C, g, D, Dtau, gap, residual = worst |M vd_ref + bias - tau| / Dtau of the full call,
    w32 = (worst e_vd, worst e_res) of the fp32 restatement over ALL_CALLS, cond = (cond M, cond of M scaled to a unit diagonal) of env 0,
    M32) at the given state, fp64"""
    from oracle.oracle import Oracle
    o64 = Oracle("f64")
    roots32, dof32, tau32 = (np.ascontiguousarray(a, np.float32) for a in (roots, dof, tau))
    v = fc.generalised_velocity(dof32, roots32, int(model.robot_actor))
    q = dof32[:, 0::2].astype(np.float64)
    parts, gap = fi.reference_parts(o64, model, roots32, q, v, np.zeros_like(v))
    M = fc.congruence_M(o64, model, roots32.astype(np.float64), q, True)
    tau64 = tau32.astype(np.float64)
    ref = solve_calls(M, parts["C"], parts["g"], tau64)
    force_rows = fi.row_units(scene.robot_model)
    D = np.abs(ref[FULL]).max(0)
    Dtau = fi.scale(tau64, force_rows)
    residual = float((np.abs(np.einsum("kij,kj->ki", M, ref[FULL]) + parts["C"] + parts["g"] - tau64) / Dtau[None, :]).max())
    for a in list(ref.values()) + [M]:
        a.setflags(write=False)
    s = 1.0 / np.sqrt(np.diag(M[0]))
    cond = (float(np.linalg.cond(M[0])), float(np.linalg.cond(M[0] * s[:, None] * s[None, :])))
    r = SimpleNamespace(scene=scene, model=model, ref=ref, M=M, C=parts["C"], g=parts["g"], D=D, Dtau=Dtau, gap=gap, residual=residual,
                        force_rows=force_rows, cond=cond, v=v)
    r32, r.M32 = restated_calls(scene, model, roots32, dof32, tau32)
    w = measure(r32, r)
    r.w32 = (max(e[0] for e in w.values()), max(e[1] for e in w.values()))
    return r


@functools.lru_cache(maxsize=None)
def references(robot):
    scene = scene_of(robot)
    dof, roots, tau = inputs(robot)
    return references_at(scene, scene.to_c(), roots, dof, tau)


def tolerances_from(w32):
    return min(round_up_125(10.0 * w32[0]), CAP_QDD), min(round_up_125(10.0 * w32[1]), CAP_RES)


def tolerances(robot):
    """-> (tol_vd, tol_res)"""
    return tolerances_from(references(robot).w32)


# ---- M^-1 ---------------------------------------------------------------------------------------------------------------------------
def e_X(X, X_ref):
    """max |X - X_ref|_jc / sqrt(X_ref,jj X_ref,cc)"""
    s = np.sqrt(np.einsum("kii->ki", X_ref))
    return float((np.abs(np.asarray(X, np.float64) - X_ref) / (s[:, :, None] * s[:, None, :])).max())


def Minv_reference_at(r):
    """-> (X_ref [K][N][N], tolerance: 10 x the e_X of the fp32 dense inverse of the fp32 congruence_M, rounded up to 1-2-5, at most
    CAP_QDD, that e_X)"""
    X_ref = np.linalg.inv(r.M)
    X32 = np.linalg.inv(r.M32)
    assert X32.dtype == np.float32
    w32 = e_X(X32, X_ref)
    return X_ref, min(round_up_125(10.0 * w32), CAP_QDD), w32


@functools.lru_cache(maxsize=None)
def Minv_reference(robot):
    out = Minv_reference_at(references(robot))
    out[0].setflags(write=False)
    return out
