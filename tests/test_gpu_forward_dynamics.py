"""mppi_sim_forward_dynamics (csrc/mppi_kernels.hpp k_sim_forward_dynamics) and the wrapper's forward_dynamics /
acquire_free_acceleration_tensor / refresh_free_acceleration_tensors / inverse_mass_matrix on the GPU, against the fp64 oracle at the
joint positions and rates the simulator itself holds: EVERY env, EVERY joint, both metrics.  Inputs, references, metrics and
tolerances: forward_dynamics_cases.py (its conditions are checked on the oracle alone by test_forward_dynamics.py); outputs are
NaN-filled before every launch and every entry must come back finite; the measured maxima are printed next to the tolerances before
anything is asserted.

 1 edges of the staged load and store: Panda (rows of 7 floats) at K = 1, 63, 64, 65, 130; gripper Panda (9, branched, prismatic
   fingers), point robot and heijn (3), the mobile manipulator (12) at K = 65.  Per row the full call, tau NULL with both terms,
   gravity only, velocity only, tau only with terms = 0; a guard band of one row behind row K - 1 stays NaN; the wrapper's free
   acceleration tensor is zero until refreshed, then the raw call
 2 the Panda's base away from the origin, yawed AND rolled; the mobile manipulator with its prismatic base joints 420 m out - at the
   tolerance of its origin row; the gripper scene (a contact-scene context with a fixed-base robot): the inputs of panda_gripper
 3 after two steps with per-env commands, at the stepped q and qd: K = 17 (`lane` step) and K = 65 (`quad` step)
 4 round trip on the device: mppi_sim_inverse_dynamics(mppi_sim_forward_dynamics(tau)) gives tau back within tol_res + tol_tau
 5 inverse_mass_matrix() against the fp64 M^-1 of the oracle, symmetric bit for bit, and X @ M from mppi_sim_mass_matrix
 6 one step of the effort-driven Panda under gravity: (qd1 - qd0) / dt against forward_dynamics(tau) at the start state
 7 through the planner: an Objective that reads forward_dynamics() runs per step, with the logged reason; PerStepOnly on a horizon view
 8 refusals before any launch: a moving base (MPPI_EUNSUPPORTED, NotImplementedError), a null qdd_dev, unknown bits (MPPI_EINVAL)
 9 a tree built on demand ([-1,0,1,1,3]) carries the kernel - in a process of its own: a plugin stays loaded for the rest of a process,
   and test_gpu_jacobian_mass.py asserts that this very tree is BUILT when it asks for it"""
import ctypes as C
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import forward_dynamics_cases as fc
import inverse_dynamics_cases as ic
import jacobian_cases as jc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
G, V = fc.ID_GRAVITY, fc.ID_VELOCITY


def make_sim(actors, K, init_positions=None, substeps=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    if substeps is not None:
        icfg.substeps = substeps
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def kernel_info(sim):
    buf = C.create_string_buffer(512)
    capi.check(sim._lib, sim._lib.mppi_kernel_info(sim._ctx, buf, 512))
    return buf.value.decode()


def launch(sim, tau, terms):
    """one raw call into a NaN-filled output with a guard band of one row behind row K - 1 -> qdd [K][n] (numpy); tau: a device
    tensor or None"""
    K, n = sim.num_envs, sim.scene.n_dof
    out = torch.full(((K + 1) * n,), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_forward_dynamics(sim._ctx, ptr(tau), terms, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * n:]).all(), "the guard row behind qdd was written"
    assert np.isfinite(got[:K * n]).all(), "entries that were never written (or not finite)"
    return got[:K * n].reshape(K, n)


def all_calls(sim, tau):
    tau_dev = torch.from_numpy(np.array(tau, np.float32)).to(sim.device)
    return {call: launch(sim, tau_dev if call[1] else None, call[0]) for call in fc.CALLS}


def check(tag, sim, got, ref, D, M_ref, Dtau, tols):
    """prints the measured maxima of both metrics next to the tolerances, then asserts them and that the partial calls sum to the full one"""
    tq, tr = tols
    e = fc.measure(got, ref, D, M_ref, Dtau)
    parts_sum = got[(G, False)].astype(np.float64) + got[(V, False)] + got[(0, True)]
    full = got[fc.FULL].astype(np.float64)
    sq, sr = fc.e_qdd(parts_sum, full, D), fc.e_res(parts_sum, full, M_ref, Dtau)
    names = {fc.FULL: "full", (3, False): "tau NULL", (1, False): "gravity", (2, False): "velocity", (0, True): "tau only"}
    print(f"\n[{tag}] K {sim.num_envs}: e_qdd / e_res " + " | ".join(f"{names[c]} {a:.2e} / {b:.2e}" for c, (a, b) in e.items())
          + f" (tol {tq:.0e} / {tr:.0e}) | parts - full {sq:.2e} / {sr:.2e} (tol {2 * tq:.0e} / {2 * tr:.0e})")
    wq, wr = max(a for a, _ in e.values()), max(b for _, b in e.values())
    assert wq <= tq, f"{tag}: e_qdd {wq:.3e} > {tq:.0e}"
    assert wr <= tr, f"{tag}: e_res {wr:.3e} > {tr:.0e}"
    assert sq <= 2.0 * tq and sr <= 2.0 * tr
    return wq, wr


def cut(refs, K):
    """(ref, D, M_ref, Dtau) of fc.references for the first K envs (the scales stay those of the robot's whole input set)"""
    return {c: v[:K] for c, v in refs[4].items()}, refs[5], refs[6][:K], refs[7]


def set_inputs(sim, dof):
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    got = sim._dof_state.cpu().numpy()
    assert np.array_equal(got, dof), "the simulator holds other joint states than the inputs"     # (the references were taken at these)
    return got


def place_base(sim, actor_name, pos, ori):
    row = np.zeros(13, np.float32)
    row[0:3], row[3:7] = pos, ori
    sim.set_root_state_tensor_by_actor_idx(torch.from_numpy(row), sim.scene.actor_index(actor_name))


# ---- 1. edges of the staged load and store ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", fc.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in fc.STORE_EDGES])
def test_load_and_store_edges(robot, K):
    actors, actor_name, _, _ = fc.ROBOTS[robot]
    refs = fc.references(robot)
    scene, root = refs[0], refs[3]
    sim = make_sim([ic.gravity_actor(a) for a in actors], K, [[0.0, 0.0, 0.0]])
    assert sim._c_model.actors[sim._c_model.robot_actor].gravity == 1
    assert np.array_equal(sim._root_state[0].cpu().numpy(), root.astype(np.float32))
    dof, tau = fc.inputs(robot)
    set_inputs(sim, dof[:K])
    got = all_calls(sim, tau[:K])
    check(f"edges {robot}", sim, got, *cut(refs, K), fc.tolerances(robot))
    assert not launch(sim, None, 0).any()                        # nothing asked for, no tau: exact zeros
    # the wrapper: the free acceleration tensor is zero until refreshed, then what the raw call gave; forward_dynamics() is the raw call
    free = sim.acquire_free_acceleration_tensor(actor_name)
    assert tuple(free.shape) == (K, scene.n_dof) and not free.any()
    assert sim.acquire_free_acceleration_tensor(actor_name) is free
    sim.refresh_free_acceleration_tensors()
    assert np.array_equal(free.cpu().numpy(), got[(3, False)])
    tau_dev = torch.from_numpy(np.array(tau[:K])).to(sim.device)
    assert np.array_equal(sim.forward_dynamics(tau_dev).cpu().numpy(), got[fc.FULL])
    assert np.array_equal(sim.forward_dynamics(velocity=False).cpu().numpy(), got[(G, False)])
    assert np.array_equal(sim.forward_dynamics(gravity=False).cpu().numpy(), got[(V, False)])
    assert np.array_equal(sim.forward_dynamics(tau_dev, gravity=False, velocity=False).cpu().numpy(), got[(0, True)])
    sim.stop_sim()


# ---- 2. tilted, far, the gripper scene ----------------------------------------------------------------------------------------------
def test_base_yawed_and_rolled():
    K = 65
    refs = fc.references("franka_panda", "tilted")
    root = refs[3]
    sim = make_sim([ic.gravity_actor("panda")], K, [jc.OFFSET_POS])
    place_base(sim, "panda", jc.OFFSET_POS, ic.TILT_ORI)
    assert np.array_equal(sim._root_state[0].cpu().numpy(), root.astype(np.float32))
    dof, tau = fc.inputs("franka_panda", "tilted")
    set_inputs(sim, dof[:K])
    got = all_calls(sim, tau[:K])
    tq, tr = fc.tolerances("franka_panda")
    check("tilted franka_panda", sim, got, *cut(refs, K), (tq, tr))
    # the row cannot pass by ignoring the base pose: gravity's part differs from the upright base's by hundreds of tolerances
    upright = fc.references("franka_panda")
    assert fc.e_qdd(got[(G, False)], upright[4][(G, False)][:K], refs[5]) > 100.0 * tq
    sim.stop_sim()


def test_mobile_manipulator_far_from_the_origin():
    K = 65
    refs, origin = fc.references("omnipanda", "far"), fc.references("omnipanda", "origin")
    sim = make_sim([ic.gravity_actor("omnipanda")], K, [[0.0, 0.0, 0.0]])
    dof, tau = fc.inputs("omnipanda", "far")
    set_inputs(sim, dof[:K])
    pos = sim._rigid_body_state.cpu().numpy()[:, -1, 0:2]
    assert np.abs(pos).min() > ic.FAR - 5.0                       # the arm does stand 420 m out, in x and in y
    tols = fc.tolerances_from(origin[8], origin[9])               # the tolerance of the origin row alone
    assert tols[0] <= fc.tolerances("omnipanda")[0] and tols[1] <= fc.tolerances("omnipanda")[1]
    check("far omnipanda, at the tolerance of origin", sim, all_calls(sim, tau[:K]), *cut(refs, K), tols)
    sim.stop_sim()


def test_contact_scene_context():
    K = 65
    refs = fc.references("panda_gripper")
    root = refs[3]
    sim = make_sim([ic.gravity_actor("panda_gripper")] + jc.GRIPPER_SCENE[1:], K, [[0.0, 0.0, 0.0]])
    assert " step=scene" in kernel_info(sim), kernel_info(sim)
    assert np.array_equal(sim._root_state[0, sim.scene.robot_idx].cpu().numpy(), root[0].astype(np.float32))
    dof, tau = fc.inputs("panda_gripper")
    set_inputs(sim, dof[:K])
    check("contact scene panda_gripper", sim, all_calls(sim, tau[:K]), *cut(refs, K), fc.tolerances("panda_gripper"))
    sim.stop_sim()


# ---- 3. after stepping --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", [(17, "lane"), (65, "quad")])
def test_after_stepping(K, step, oracle64):
    sim = make_sim([ic.gravity_actor("panda")], K, [[0.0, 0.0, 0.0]])
    assert f" step={step} " in kernel_info(sim) + " ", kernel_info(sim)
    dof0, tau = fc.inputs("franka_panda")
    start = set_inputs(sim, dof0[:K])
    rng = np.random.default_rng(7)
    for _ in range(2):
        sim.apply_robot_cmd(torch.from_numpy(rng.uniform(-1.0, 1.0, size=(K, sim.scene.nu)).astype(np.float32)).to(sim.device))
        sim.step()
    dof = sim._dof_state.cpu().numpy()                            # the materialised dof tensor: the reference is taken from it
    assert np.abs(dof[:, 0::2] - start[:, 0::2]).max(1).min() > 1e-3 and np.abs(dof[:, 1::2] - start[:, 1::2]).max(1).min() > 1e-3     # every env has moved
    root = sim._root_state[0].cpu().numpy().astype(np.float64)
    _, model, model_off, _ = fc.models_of("franka_panda")
    q, qd = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64)
    ref = fc.reference_calls(oracle64, model, model_off, root, q, qd, tau[:K], fc.CALLS)
    M_ref = jc.oracle_M(oracle64, model, root, q)
    Dtau = fc.references("franka_panda")[7]
    got = all_calls(sim, tau[:K])
    check(f"stepped ({step})", sim, got, ref, fc.scale(ref), M_ref, Dtau, fc.tolerances("franka_panda"))
    # the result follows the envs' current state: against the references of the start state it is off by hundreds of tolerances
    assert fc.e_qdd(got[fc.FULL], fc.references("franka_panda")[4][fc.FULL][:K], fc.scale(ref)) > 100.0 * fc.tolerances("franka_panda")[0]
    sim.stop_sim()


# ---- 4. round trip on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["franka_panda", "panda_gripper", "omnipanda"])
def test_round_trip_on_the_device(robot):
    K = 65
    actors = fc.ROBOTS[robot][0]
    sim = make_sim([ic.gravity_actor(a) for a in actors], K, [[0.0, 0.0, 0.0]])
    dof, tau = fc.inputs(robot)
    set_inputs(sim, dof[:K])
    n = sim.scene.n_dof
    tau_dev = torch.from_numpy(np.array(tau[:K])).to(sim.device)
    qdd = torch.full((K, n), float("nan"), dtype=torch.float32, device=sim.device)
    back = torch.full((K, n), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_forward_dynamics(sim._ctx, ptr(tau_dev), G | V, ptr(qdd)))
    capi.check(sim._lib, sim._lib.mppi_sim_inverse_dynamics(sim._ctx, ptr(qdd), G | V, ptr(back)))
    Dtau = fc.references(robot)[7]
    e = ic.e_tau(back.cpu().numpy(), tau[:K].astype(np.float64), Dtau)
    tol = fc.tolerances(robot)[1] + ic.tolerance(robot)      # (the inverse dynamics is linear in qdd: the two errors add)
    print(f"\n[round trip {robot}] K {K}: e_tau of ID(FD(tau)) against tau {e:.2e} (tol_res {fc.tolerances(robot)[1]:.0e} + tol_tau {ic.tolerance(robot):.0e})")
    assert e <= tol
    sim.stop_sim()


# ---- 5. inverse_mass_matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["franka_panda", "omnipanda"])
def test_inverse_mass_matrix(robot):
    K = 65
    actors, actor_name, _, _ = fc.ROBOTS[robot]
    sim = make_sim([ic.gravity_actor(a) for a in actors], K, [[0.0, 0.0, 0.0]])
    dof, _ = fc.inputs(robot)
    set_inputs(sim, dof[:K])
    n = sim.scene.n_dof
    X_ref, tol_X, w32 = fc.Minv_reference(robot, K)
    X = sim.inverse_mass_matrix()
    assert tuple(X.shape) == (K, n, n) and bool(torch.isfinite(X).all())
    assert torch.equal(X, X.transpose(1, 2))                      # symmetric bit for bit
    e = fc.e_X(X.cpu().numpy(), X_ref)
    M = sim.acquire_mass_matrix_tensor(actor_name)
    sim.refresh_mass_matrix_tensors()
    # X @ M against the identity, entry (i, j) on the scale sqrt(X_ref,ii M_ref,jj) of a row of X times a column of M
    M_ref = fc.references(robot)[6][:K]
    tol_M = jc.tolerances(robot)[1]
    R = X.cpu().numpy().astype(np.float64) @ M.cpu().numpy().astype(np.float64) - np.eye(n)
    sx, sm = np.sqrt(np.einsum("kii->ki", X_ref)), np.sqrt(np.einsum("kii->ki", M_ref))
    e_id = float((np.abs(R) / (sx[:, :, None] * sm[:, None, :])).max())
    print(f"\n[M^-1 {robot}] K {K}: e_X {e:.2e} (tol {tol_X:.0e}; the fp32 oracle {w32:.1e}); X @ M - 1 scaled {e_id:.2e} (tol {tol_X:.0e} + {tol_M:.0e})")
    assert w32 <= 0.1 * tol_X
    assert e <= tol_X
    assert e_id <= tol_X + tol_M
    sim.stop_sim()


# ---- 6. one step of the effort-driven Panda -----------------------------------------------------------------------------------------
def test_one_step_is_the_forward_dynamics(oracle64):
    scene, model, root, dof, qdd_star, tau_ref, cmd_ref, after = ic.torque_case()
    K = len(dof)
    sim = make_sim([ic.actor_file()], K, [[0.0, 0.0, 0.0]], substeps=1)
    m = sim._c_model
    assert m.substeps == 1 and m.drive_mode == capi.DRIVE_EFFORT and m.actors[m.robot_actor].gravity == 1
    h = float(m.dt) / int(m.substeps)
    set_inputs(sim, dof)
    tau32 = tau_ref.astype(np.float32)
    q, qd0 = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64)
    # the oracle's own gap: its step under the reference command against its forward dynamics under the joint force that command leaves
    fd64 = np.stack([oracle64.forward_dynamics(model, root, q[k], qd0[k], tau32[k].astype(np.float64)) for k in range(K)])
    D = np.abs(fd64).max(0)
    gap64 = float((np.abs((after[:, 1::2] - qd0) / h - fd64) / D[None, :]).max())
    fd = sim.forward_dynamics(torch.from_numpy(tau32).to(sim.device)).cpu().numpy().astype(np.float64)
    sim.apply_robot_cmd(torch.from_numpy(cmd_ref.astype(np.float32)).to(sim.device))
    sim.step()
    qd1 = sim._dof_state.cpu().numpy()[:, 1::2].astype(np.float64)
    gap = float((np.abs((qd1 - qd0) / h - fd) / D[None, :]).max())
    tq = fc.tolerances("franka_panda")[0]
    print(f"\n[one step] K {K}, h {h}: (qd1 - qd0) / h against forward_dynamics(tau): the fp64 oracle's own gap {gap64:.2e}, the device's {gap:.2e} "
          f"(bound: the oracle's + {tq:.0e}); forward_dynamics(tau) against the oracle's {fc.e_qdd(fd, fd64, D):.2e}")
    assert gap <= gap64 + tq
    sim.stop_sim()


# ---- 7. the wrapper, and through the planner ----------------------------------------------------------------------------------------
class FreeFall(object):
    """|qdd| of the envs left to themselves: the norm of forward_dynamics() over the joints; keeps what it saw and what it charged"""
    weights = {}

    def __init__(self, scale=1.0):
        self.weights = {}
        self.scale = scale
        self.seen = []

    def reset(self):
        pass

    def compute_cost(self, sim):
        c = torch.linalg.norm(sim.forward_dynamics(), dim=1)
        self.seen.append((sim.get_dof_state().clone(), c.clone()))
        return self.scale * c


def test_wrapper_and_planner(caplog):
    from mppiisaac.planner.mppi_isaac import MPPIisaacPlanner
    K, H = 64, 3
    q0 = [0.0, -0.94, 0.0, -2.8, 0.0, 1.8675, 0.0]
    qd0 = [0.3, -0.2, 0.1, 0.25, -0.3, 0.2, -0.1]
    cfg = load_config({"defaults": [{"mppi": "panda"}, {"isaacgym": "normal"}], "actors": [ic.gravity_actor("panda"), "goal"],
                       "initial_actor_positions": [[0.0, 0.0, 0.0]], "nx": 14},
                      overrides={"mppi.num_samples": K, "mppi.horizon": H, "mppi.filter_u": False})
    objective = FreeFall()
    with caplog.at_level(logging.WARNING, logger="mppiisaac"):
        planner = MPPIisaacPlanner(cfg, objective)
        planner.compute_action(q0, qd0)
    S = planner.mppi.get_costs().cpu().numpy().astype(np.float64)
    said = " | ".join(r.getMessage() for r in caplog.records)
    assert planner.mppi._fused_cost is None and "not traceable" in said and "forward_dynamics" in said        # not traced, and why
    assert planner.mppi._batch_sig[0] == "per-step" and "runs per step" in said and "per-step only" in said and "forward dynamics" in said
    # the per-step calls of that command: the last H of them, on the live envs, each stepped on from the one before
    steps = objective.seen[-H:]
    assert len(steps) == H
    assert all(tuple(d.shape) == (K, 14) for d, _ in steps) and not torch.equal(steps[0][0], steps[1][0]) and not torch.equal(steps[1][0], steps[2][0])
    gamma = float(cfg.mppi.rollout_var_discount)
    wrapper_checks(planner.sim, K)
    planner.sim.stop_sim()
    # the same command with the Objective's costs switched off: what is left is the control cost, by the same per-step route
    idle = FreeFall(scale=0.0)
    base = MPPIisaacPlanner(cfg, idle)
    base.compute_action(q0, qd0)
    S0 = base.mppi.get_costs().cpu().numpy().astype(np.float64)
    assert base.mppi._batch_sig[0] == "per-step" and len(idle.seen) == len(objective.seen)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(idle.seen[-H:], steps))      # the same noise, the same states
    base.sim.stop_sim()
    # ... and the same quantity computed eagerly, step by step, on a simulator of its own at the states the Objective saw
    eager = make_sim([ic.gravity_actor("panda"), "goal"], K, [[0.0, 0.0, 0.0]])
    want = np.zeros(K)
    for t, (dof, c) in enumerate(steps):
        eager.set_dof_state_tensor(dof)
        c_eager = torch.linalg.norm(eager.forward_dynamics(), dim=1)
        assert torch.equal(c_eager, c)                              # the same kernel on the same state: bit for bit
        want += gamma ** t * c_eager.cpu().numpy().astype(np.float64)
    eager.stop_sim()
    err = np.abs((S - S0) - want).max()
    # S and S0 are fp32 sums of H + 1 terms each (H discounted costs and the control cost): every addition rounds by at most half an
    # ulp of the sum so far, 2^-24 |S|; the discount factors are fp32 powers (a few 1e-7 of the term)
    bound = 2.0 * (H + 2) * 2.0 ** -24 * max(np.abs(S).max(), np.abs(S0).max()) + 1e-6 * np.abs(want).max()
    print(f"\n[planner] K {K}, H {H}: costs {S.min():.3f} .. {S.max():.3f}, without the Objective {S0.min():.3f} .. {S0.max():.3f}; "
          f"(S - S0) against the discounted sum of the eager per-step values ({want.min():.3f} .. {want.max():.3f}): {err:.1e} (bound {bound:.1e})")
    assert np.isfinite(S).all() and want.min() > 0.0 and want.max() - want.min() > 1e-3 * want.max()          # the samples differ
    assert err <= bound


def wrapper_checks(sim, K):
    n = sim.scene.n_dof
    # inside a horizon view all of them refuse
    free = sim.acquire_free_acceleration_tensor("panda")
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (sim.forward_dynamics, sim.refresh_free_acceleration_tensors, lambda: sim.acquire_free_acceleration_tensor("panda"), sim.inverse_mass_matrix):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "forward dynamics" in str(e.value)
    # the free acceleration tensor is written by refresh only
    sim.refresh_free_acceleration_tensors()
    f0 = free.clone()
    assert torch.equal(f0, sim.forward_dynamics())
    sim.apply_robot_cmd(torch.linspace(-1.0, 1.0, K * sim.scene.nu, device=sim.device).reshape(K, sim.scene.nu))
    sim.step()
    fresh = sim.forward_dynamics()
    assert torch.equal(free, f0) and not torch.equal(free, fresh)          # stale before a refresh
    sim.refresh_free_acceleration_tensors()
    assert torch.equal(free, fresh)                                        # fresh after
    # tau as [n_dof] (the same for every env) and as [K, n_dof]; anything else raises
    a = torch.linspace(-3.0, 3.0, n, device=sim.device)
    one = sim.forward_dynamics(a)
    assert tuple(one.shape) == (K, n)
    assert torch.equal(one, sim.forward_dynamics(a.repeat(K, 1))) and torch.equal(one, sim.forward_dynamics(a.cpu().numpy()))
    assert not torch.equal(one, fresh)
    for wrong in (torch.zeros(n + 1), torch.zeros(K, n + 1), torch.zeros(K + 1, n), torch.zeros(1, n), torch.zeros(K, n, 1), torch.zeros(())):
        with pytest.raises(ValueError, match="tau has shape"):
            sim.forward_dynamics(wrong)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    lib = boxer._lib
    n = boxer.scene.n_dof
    out = torch.full((K, n), float("nan"), dtype=torch.float32, device=boxer.device)
    tau = torch.zeros((K, n), dtype=torch.float32, device=boxer.device)
    for t in (tau, None):
        assert lib.mppi_sim_forward_dynamics(boxer._ctx, ptr(t), 3, ptr(out)) == capi.MPPI_EUNSUPPORTED
        said = lib.mppi_last_error().decode()
        assert "mppi_sim_forward_dynamics" in said and "moving base" in said and "unsupported" in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                            # nothing was launched
    boxer.acquire_free_acceleration_tensor("boxer")
    for call in (boxer.forward_dynamics, lambda: boxer.forward_dynamics(tau), lambda: boxer.forward_dynamics(tau[0]),
                 boxer.refresh_free_acceleration_tensors, boxer.inverse_mass_matrix):
        with pytest.raises(NotImplementedError, match="moving base"):
            call()
    boxer.stop_sim()
    panda = make_sim([ic.gravity_actor("panda")], K, [[0.0, 0.0, 0.0]])
    n = panda.scene.n_dof
    out = torch.full((K, n), float("nan"), dtype=torch.float32, device=panda.device)
    tau = torch.zeros((K, n), dtype=torch.float32, device=panda.device)
    assert lib.mppi_sim_forward_dynamics(panda._ctx, ptr(tau), 3, None) == capi.MPPI_EINVAL
    assert "null" in lib.mppi_last_error().decode()
    for terms in (4, 7, 8, -1, 1 << 30):
        assert lib.mppi_sim_forward_dynamics(panda._ctx, ptr(tau), terms, ptr(out)) == capi.MPPI_EINVAL, terms
        assert "unknown bits" in lib.mppi_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    capi.check(lib, lib.mppi_sim_forward_dynamics(panda._ctx, ptr(tau), 3, ptr(out)))      # the context is as healthy as before
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        panda.acquire_free_acceleration_tensor("no_such_actor")
    panda.stop_sim()


# ---- 9. a tree built on demand ------------------------------------------------------------------------------------------------------
def on_demand_tree(tmp):
    """runs in a process of its own (see the module docstring): builds the tree [-1,0,1,1,3] into an empty cache under tmp and checks
    the plugin's kernel against the oracle"""
    from oracle.oracle import Oracle
    from test_gpu_runtime_tree import actor_yaml, write_branched_urdf
    urdf, actor = os.path.join(tmp, "branched5.urdf"), os.path.join(tmp, "arm5.yaml")
    write_branched_urdf(urdf)
    text = open(urdf).read()       # (its second branch hangs off l2 instead of l1: the tree of test_gpu_jacobian_mass.py)
    assert text.count('<parent link="l1"/><child link="l3"/>') == 1
    with open(urdf, "w") as f:
        f.write(text.replace('<parent link="l1"/><child link="l3"/>', '<parent link="l2"/><child link="l3"/>'))
    actor_yaml(actor, urdf)
    os.environ["MPPI_JIT_CACHE"] = os.path.join(tmp, "jit")
    K = 65
    sim = make_sim([actor], K, [[0.1, -0.2, 0.0]])
    assert "topology=[-1,0,1,1,3]" in kernel_info(sim), kernel_info(sim)
    info = C.create_string_buffer(512)
    capi.check(sim._lib, sim._lib.mppi_jit_info(info, 512))
    assert info.value.decode().startswith("built ") and "topo_m1_0_1_1_3_free" in info.value.decode(), info.value
    n = sim.scene.n_dof
    bodies = sim.scene.robot_model["bodies"]
    lo = np.array([b["lower"] if b["limited"] else -2.0 for b in bodies])
    hi = np.array([b["upper"] if b["limited"] else 2.0 for b in bodies])
    rng = np.random.default_rng(ic.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(lo, hi, size=(K, n)), rng.uniform(-ic.QD_AMP, ic.QD_AMP, size=(K, n))
    qdd_star = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, n)).astype(np.float32)
    set_inputs(sim, dof)
    root = sim._root_state[0].cpu().numpy().astype(np.float64)
    o64, o32 = Oracle("f64"), Oracle("f32")
    model = sim._c_model
    assert model.actors[model.robot_actor].gravity == 1
    model_off = sim.scene.to_c()
    model_off.actors[model_off.robot_actor].gravity = 0
    q, qd = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64)
    parts = ic.reference_parts(o64, model, root, q, qd, qdd_star)
    tau = ic.combine(parts, *ic.FULL).astype(np.float32)
    ref = fc.reference_calls(o64, model, model_off, root, q, qd, tau)
    r32 = fc.reference_calls(o32, model, model_off, root, q, qd, tau)
    D, Dtau, M_ref = fc.scale(ref), ic.scale(parts), jc.oracle_M(o64, model, root, q)
    tols = fc.tolerances_from(max(fc.e_qdd(r32[c], ref[c], D) for c in fc.ALL_CALLS), max(fc.e_res(r32[c], ref[c], M_ref, Dtau) for c in fc.ALL_CALLS))
    check("on-demand tree [-1,0,1,1,3]", sim, all_calls(sim, tau), {c: ref[c] for c in fc.CALLS}, D, M_ref, Dtau, tols)     # the rule of the cases file on these inputs
    sim.stop_sim()


def test_tree_built_on_demand(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env, capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "[on-demand tree [-1,0,1,1,3]]" in run.stdout


if __name__ == "__main__":
    on_demand_tree(sys.argv[1])
