"""Inputs of the lane-scalar fixtures (tests/golden/lane_scalars, tools/make_lane_scalar_golden.py, tests/test_gpu_lane_scalars.py):
the smallest contact-free rollouts in which the per-joint scalars of the octet kernels take every path - a joint held at a stop, a
velocity clamped at vmax and a wavefront that takes the saturated second solve, all within ONE rollout of each case.

How the states get there: the controls reach 3 rad/s (m/s) with a noise of the same size, beyond every vmax of the three robots,
so the velocity drive (kd h = 15 against joint inertias of 1e-3 .. 1 kg m^2) asks for more than the effort limits in the first
substep (the second solve) and carries the light joints to vmax within it (the clamp); one joint starts a millimetre (a
milliradian) short of its upper stop and moving towards it (the stop, and the zero velocity behind it)."""
import ctypes as C

import numpy as np

from mppiisaac.backend import capi
from mppiisaac.planner.mppi import MPPIConfig, make_config
from scenes import build_scene, panda_reach, point_reach

KERNELS = ("oct-pair", "oct")
UMAX, SIGMA = 3.0, 3.0


def _wide(nu):
    return dict(u_min=[-UMAX], u_max=[UMAX], noise_sigma=(SIGMA * np.eye(nu)).tolist(), lambda_=0.5)


def panda_stick(K, H):
    scene, m, cfg, cost, dof, root = panda_reach(K=K, H=H, **_wide(7))
    dof = np.array(dof, np.float64)
    dof[2 * 3], dof[2 * 3 + 1] = m.bodies[3].upper - 1e-3, 0.5           # joint 4: a milliradian short of its upper stop
    return scene, m, cfg, cost, dof, root


def panda_stick_cmd_map(K, H):
    """five commands drive the seven joints through a mixed two-term map: the all-revolute instantiation WITHOUT the identity
    map (targets formed per lane from the lane's own row of the map)"""
    scene, m, cfg, cost, dof, root = panda_reach(K=K, H=H, **_wide(5))
    m.nu = 5
    for i in range(m.n_bodies):
        m.cmd_col[i][0], m.cmd_col[i][1] = i % 5, (i + 2) % 5
        m.cmd_coef[i][0], m.cmd_coef[i][1] = 1.0, 0.5
    assert cfg.nu == 5
    dof = np.array(dof, np.float64)
    dof[2 * 3], dof[2 * 3 + 1] = m.bodies[3].upper - 1e-3, 0.5
    return scene, m, cfg, cost, dof, root


def panda_stick_point_cost(K, H):
    """the point cost (q0, q1 against a target) on the all-revolute arm: the hand-over / stage cost that reads two positions
    replicated out of a joint vector"""
    scene, m, cfg, cost, dof, root = panda_stick(K, H)
    cost = capi.Cost()
    cost.kind = capi.COST_POINT_REACH
    cost.actor[0] = scene.actor_index("goal")
    cost.w[0] = 2.0
    return scene, m, cfg, cost, dof, root


def panda_gripper(K, H):
    """nine bodies, two prismatic fingers on one hand (a branch): the generic instantiation"""
    scene = build_scene(["panda_gripper", "goal"], [[0.0, 0.0, 0.0]])
    assert scene.nu == 9
    m = scene.to_c()
    cfg = make_config(MPPIConfig(num_samples=K, horizon=H, sample_null_action=True, **_wide(9)), viz_link=scene.viz_link_index())
    cost = capi.Cost()
    cost.kind = capi.COST_PANDA_REACH
    cost.link[0] = scene.rigid_body_index(scene.robot.name, "panda_hand")
    cost.actor[0] = scene.actor_index("goal")
    cost.w[0], cost.w[1] = 1.0, 0.1
    dof, root = scene.initial_state()
    dof = np.array(dof, np.float64)
    root[scene.actor_index("goal"), 0:3] = [0.6, 0.3, 0.5]
    dof[2 * 7], dof[2 * 7 + 1] = m.bodies[7].upper - 1e-3, 0.1           # left finger: a millimetre short of fully open
    dof[2 * 3], dof[2 * 3 + 1] = m.bodies[3].upper - 1e-3, 0.5
    return scene, m, cfg, cost, dof, root


def point_robot(K, H):
    scene, m, cfg, cost, dof, root = point_reach(K=K, H=H, goal=(48.0, 0.2), **_wide(3))
    dof = np.array(dof, np.float64)
    dof[0], dof[1] = m.bodies[0].upper - 1e-3, 1.0                       # x: a millimetre short of the end of its rail
    return scene, m, cfg, cost, dof, root


CASES = {"panda_stick-K24-H3": (panda_stick, 24, 3), "panda_stick-K16-H1": (panda_stick, 16, 1),
         "panda_gripper-K24-H3": (panda_gripper, 24, 3), "point_robot-K24-H3": (point_robot, 24, 3),
         "panda_stick_cmd_map-K24-H3": (panda_stick_cmd_map, 24, 3), "panda_stick_point_cost-K24-H3": (panda_stick_point_cost, 24, 3)}


def nominal(cfg):
    return (0.25 * UMAX * np.random.default_rng(0).normal(size=(cfg.horizon, cfg.nu))).astype(np.float32)


def limits(m):
    """lower, upper, vmax per body as the float32 values the kernels hold"""
    b = [m.bodies[i] for i in range(m.n_bodies)]
    return tuple(np.array([getattr(x, f) for x in b], np.float32) for f in ("lower", "upper", "velocity"))


def path_counts(m, q, qd):
    """q, qd [H][n][K] after every step -> (entries of q equal to a stop, entries of |qd| equal to vmax), bit for bit"""
    lo, hi, vmax = limits(m)
    q, qd = np.asarray(q, np.float32), np.asarray(qd, np.float32)
    at_stop = (q == lo[None, :, None]) | (q == hi[None, :, None])
    at_vmax = np.abs(qd) == vmax[None, :, None]
    return int(at_stop.sum()), int(at_vmax.sum())


def oracle_paths(o, m, cfg, cost, dof, root, U, eps, prior=None):
    """the same rollout on the CPU oracle `o`: (q, qd) [H][n][K] after every step and the saturation sets [K][H * substeps]
    (`prior`: the sequence the sample before the last takes under use_priors; its saturation set is the noise sample's)"""
    K, H, nu, n = cfg.num_samples, cfg.horizon, cfg.nu, m.n_bodies
    lo, hi = np.array([cfg.u_min[c] for c in range(nu)]), np.array([cfg.u_max[c] for c in range(nu)])
    q, qd = np.zeros((H, n, K)), np.zeros((H, n, K))
    logs = np.zeros((K, H * m.substeps), np.uint32)
    o.lib.orc_rollout_satlog.restype = o.ctype
    for k in range(K):
        x, v = np.array(dof[0::2], np.float64), np.array(dof[1::2], np.float64)
        for t in range(H):
            u = np.asarray(U[t], np.float64) + eps[t, :, k]
            if cfg.sample_null_action and cfg.k_offset + k == cfg.k_total - 1:
                u = np.zeros(nu)
            if prior is not None and cfg.use_priors and cfg.k_offset + k == cfg.k_total - 2:
                u = np.asarray(prior[t], np.float64)
            x, v = o.step(m, root, x, v, o.cmd_map(m, np.clip(u, lo, hi)))
            q[t, :, k], qd[t, :, k] = x, v
        o.lib.orc_rollout_satlog(C.byref(m), C.byref(cfg), C.byref(cost), o.p(o.arr(dof)), o.p(o.arr(root)), o.p(o.arr(U)), o.p(o.arr(eps)),
                                 C.c_int(k), logs[k].ctypes.data_as(C.POINTER(C.c_uint32)))
    return q, qd, logs


def run_gpu(lib, make, K, H, kernel):
    """One rollout + update and one trajectory dump of a fresh context under MPPI_ROLLOUT=`kernel`, at the case's state and nominal
    and the configuration's own noise (seed 0) -> (kernel info, {name: float32 array})"""
    import os

    import torch
    scene, m, cfg, cost, dof, root = make(K, H)
    old = os.environ.get("MPPI_ROLLOUT")
    os.environ["MPPI_ROLLOUT"] = kernel
    try:
        ctx = C.c_void_p()
        capi.check(lib, lib.mppi_create(C.byref(m), C.byref(cfg), 0, C.byref(ctx)))
    finally:
        os.environ.pop("MPPI_ROLLOUT") if old is None else os.environ.__setitem__("MPPI_ROLLOUT", old)

    def call(name, *args):
        capi.check(lib, getattr(lib, name)(ctx, *args))

    def get(name, shape):
        out = np.zeros(shape, np.float32)
        call(name, capi.fptr(out))
        return out

    call("mppi_set_cost", C.byref(cost))
    buf = C.create_string_buffer(512)
    call("mppi_kernel_info", buf, 512)
    info = dict(kv.split("=", 1) for kv in buf.value.decode().split())
    call("mppi_sample", C.c_uint32(0))
    d, r, U0 = np.ascontiguousarray(dof, np.float32), np.ascontiguousarray(root, np.float32), nominal(cfg)
    call("mppi_set_state", capi.fptr(d), capi.fptr(r))
    call("mppi_set_nominal", capi.fptr(U0))
    out = {"eps": get("mppi_get_noise", (H, cfg.nu, K))}
    # the DUMP instantiation first: it leaves the nominal alone
    n = m.n_bodies
    traj = torch.zeros((H * K, 2 * n), dtype=torch.float32, device="cuda")
    call("mppi_rollout_trajectory")
    call("mppi_materialise_trajectory", C.c_void_p(traj.data_ptr()), None, None, None)
    call("mppi_synchronize")
    out["dump_dof"] = traj.cpu().numpy().reshape(H, K, 2 * n)
    out["dump_S"] = get("mppi_get_costs", (K,))
    out["dump_du"] = get("mppi_get_perturbations", (H, cfg.nu, K))
    call("mppi_rollout")
    out["S"] = get("mppi_get_costs", (K,))
    out["du"] = get("mppi_get_perturbations", (H, cfg.nu, K))
    if cfg.want_rollouts:
        out["viz"] = get("mppi_get_rollouts", (H, K, 3))
    call("mppi_reduce", None)
    call("mppi_update", None, 1)
    out["beta_eta"] = get("mppi_get_weights_stats", (2,))
    out["U"] = get("mppi_get_nominal", (H, cfg.nu))
    out["action"] = get("mppi_get_action", (cfg.nu,))
    lib.mppi_destroy(ctx)
    return info, out


def dump_q_qd(dump_dof):
    """[H][K][2n] rows of the trajectory dump -> q, qd [H][n][K]"""
    return dump_dof[:, :, 0::2].transpose(0, 2, 1), dump_dof[:, :, 1::2].transpose(0, 2, 1)
