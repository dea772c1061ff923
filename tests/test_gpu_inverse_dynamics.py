"""mppi_sim_inverse_dynamics (csrc/mppi_kernels.hpp k_sim_inverse_dynamics) and the wrapper's acquire_bias_force_tensor /
refresh_bias_force_tensors / inverse_dynamics on the GPU, against the fp64 oracle at the joint positions and rates the simulator
itself holds: EVERY env, EVERY joint.  Inputs, references, metric and tolerances: inverse_dynamics_cases.py (its conditions are
checked on the oracle alone by test_inverse_dynamics.py); outputs are NaN-filled before every launch and every entry must come back
finite; the measured maxima are printed next to the tolerances before anything is asserted.

 1 edges of the staged load and store: Panda (rows of 7 floats) at K = 1, 63, 64, 65, 130; gripper Panda (9, branched, prismatic
   fingers), point robot and heijn (3), the mobile manipulator (12) at K = 65.  Per row the full call, qdd NULL with both terms,
   gravity only, velocity only, qdd only with terms = 0; the partial calls sum to the full one within two tolerances; a guard band
   of 64 floats behind tau stays NaN; the wrapper's bias tensor is zero until refreshed, then the raw call
 2 base pose: the Panda's base away from the origin, yawed AND rolled (gravity along no base axis); the mobile manipulator with
   its prismatic base joints 420 m out - the same tolerances
 3 after two steps with per-env commands, at the stepped q and qd: K = 17 (`lane` step) and K = 65 (`quad` step)
 4 a contact-scene context with a fixed-base robot (gripper Panda, block, table): the values of the contact-free gripper Panda
 5 two fixed-base point robots as one forest: another qdd for the second robot leaves the first robot's tau bit for bit
 6 a tree built on demand (the branched arm of test_gpu_runtime_tree.py, one branch moved): the plugin's table carries the launcher
 7 refusals before any launch: a moving base (MPPI_EUNSUPPORTED, NotImplementedError), a null tau_dev, unknown bits (MPPI_EINVAL)
 8 wrapper: [n_dof] and [K, n_dof] qdd, a wrong shape raises, PerStepOnly on a horizon view, an Objective that costs
   |inverse_dynamics()| runs per step - neither traced nor on the horizon view -, with the logged reason
 9 it holds the arm up: an effort-driven Panda under gravity, 65 poses at rest, commanded inverse_dynamics(gravity only) for 20 steps
10 computed torque: one step under tau + kd (qd + h qdd) changes the rates by h qdd"""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

import inverse_dynamics_cases as ic
import jacobian_cases as jc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config
from test_gpu_step_matrix import TOL

pytestmark = pytest.mark.gpu
GUARD = 64


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


def launch(sim, qdd, terms):
    """one raw call into a NaN-filled output with a guard band behind it -> tau [K][n] (numpy); qdd: a device tensor or None"""
    K, n = sim.num_envs, sim.scene.n_dof
    out = torch.full((K * n + GUARD,), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_inverse_dynamics(sim._ctx, ptr(qdd), terms, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * n:]).all(), "the guard band behind tau was written"
    assert np.isfinite(got[:K * n]).all(), "entries that were never written (or not finite)"
    return got[:K * n].reshape(K, n)


def all_calls(sim, qdd):
    qdd_dev = torch.from_numpy(np.array(qdd, np.float32)).to(sim.device)
    return {call: launch(sim, qdd_dev if call[1] else None, call[0]) for call in ic.CALLS}


def check(tag, sim, got, parts, D, tol):
    """prints the measured maxima next to the tolerance, then asserts them and that the partial calls sum to the full one"""
    e = {call: ic.e_tau(got[call], ic.combine(parts, *call), D) for call in got}
    parts_sum = got[(ic.ID_GRAVITY, False)].astype(np.float64) + got[(ic.ID_VELOCITY, False)] + got[(0, True)]
    e_sum = ic.e_tau(parts_sum, got[ic.FULL].astype(np.float64), D)
    print(f"\n[{tag}] K {sim.num_envs}: e_tau full {e[ic.FULL]:.2e} | qdd NULL {e[(3, False)]:.2e} | gravity {e[(1, False)]:.2e} | velocity {e[(2, False)]:.2e} | "
          f"qdd only {e[(0, True)]:.2e} (tol {tol:.0e}) | parts - full {e_sum:.2e} (tol {2 * tol:.0e})")
    assert max(e.values()) <= tol, f"{tag}: e_tau {max(e.values()):.3e} > {tol:.0e}"
    assert e_sum <= 2.0 * tol
    return max(e.values())


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
@pytest.mark.parametrize("robot,K", ic.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in ic.STORE_EDGES])
def test_load_and_store_edges(robot, K):
    actors, actor_name, _, _ = ic.ROBOTS[robot]
    scene, model, root, parts, D, _ = ic.references(robot)
    sim = make_sim([ic.gravity_actor(a) for a in actors], K, [[0.0, 0.0, 0.0]])
    assert sim._c_model.actors[sim._c_model.robot_actor].gravity == 1
    assert np.array_equal(sim._root_state[0].cpu().numpy(), root.astype(np.float32))
    dof, qdd = ic.inputs(robot)
    set_inputs(sim, dof[:K])
    got = all_calls(sim, qdd[:K])
    check(f"edges {robot}", sim, got, {p: v[:K] for p, v in parts.items()}, D, ic.tolerance(robot))
    assert not launch(sim, None, 0).any()                        # nothing asked for: exact zeros
    # the wrapper: the bias tensor is zero until refreshed, then what the raw call gave; inverse_dynamics() is the raw call
    bias = sim.acquire_bias_force_tensor(actor_name)
    assert tuple(bias.shape) == (K, scene.n_dof) and not bias.any()
    assert sim.acquire_bias_force_tensor(actor_name) is bias
    sim.refresh_bias_force_tensors()
    assert np.array_equal(bias.cpu().numpy(), got[(3, False)])
    qdd_dev = torch.from_numpy(np.array(qdd[:K])).to(sim.device)
    assert np.array_equal(sim.inverse_dynamics(qdd_dev).cpu().numpy(), got[ic.FULL])
    assert np.array_equal(sim.inverse_dynamics(velocity=False).cpu().numpy(), got[(ic.ID_GRAVITY, False)])
    assert np.array_equal(sim.inverse_dynamics(gravity=False).cpu().numpy(), got[(ic.ID_VELOCITY, False)])
    assert np.array_equal(sim.inverse_dynamics(qdd_dev, gravity=False, velocity=False).cpu().numpy(), got[(0, True)])
    sim.stop_sim()


# ---- 2. base pose -------------------------------------------------------------------------------------------------------------------
def test_base_yawed_and_rolled():
    K = 65
    scene, model, root, parts, D, _ = ic.references("franka_panda", "tilted")
    _, _, _, parts0, _, _ = ic.references("franka_panda")
    sim = make_sim([ic.gravity_actor("panda")], K, [jc.OFFSET_POS])
    place_base(sim, "panda", jc.OFFSET_POS, ic.TILT_ORI)
    assert np.array_equal(sim._root_state[0].cpu().numpy(), root.astype(np.float32))
    dof, qdd = ic.inputs("franka_panda", "tilted")
    set_inputs(sim, dof[:K])
    got = all_calls(sim, qdd[:K])
    tol = ic.tolerance("franka_panda")
    check("tilted franka_panda", sim, got, {p: v[:K] for p, v in parts.items()}, D, tol)
    # the row cannot pass by ignoring the base pose: gravity's part differs from the upright base's by thousands of tolerances
    assert ic.e_tau(got[(ic.ID_GRAVITY, False)], parts0["g"][:K], D) > 1000.0 * tol
    sim.stop_sim()


def test_mobile_manipulator_far_from_the_origin():
    K = 65
    scene, model, root, parts, D, _ = ic.references("omnipanda", "far")
    sim = make_sim([ic.gravity_actor("omnipanda")], K, [[0.0, 0.0, 0.0]])
    dof, qdd = ic.inputs("omnipanda", "far")
    set_inputs(sim, dof[:K])
    pos = sim._rigid_body_state.cpu().numpy()[:, -1, 0:2]
    assert np.abs(pos).min() > ic.FAR - 5.0                       # the arm does stand 420 m out, in x and in y
    check("far omnipanda", sim, all_calls(sim, qdd[:K]), {p: v[:K] for p, v in parts.items()}, D, ic.tolerance("omnipanda"))
    sim.stop_sim()


# ---- 3. after stepping --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", [(17, "lane"), (65, "quad")])
def test_after_stepping(K, step, oracle64):
    sim = make_sim([ic.gravity_actor("panda")], K, [[0.0, 0.0, 0.0]])
    assert f" step={step} " in kernel_info(sim) + " ", kernel_info(sim)
    dof0, qdd = ic.inputs("franka_panda")
    start = set_inputs(sim, dof0[:K])
    rng = np.random.default_rng(7)
    for _ in range(2):
        sim.apply_robot_cmd(torch.from_numpy(rng.uniform(-1.0, 1.0, size=(K, sim.scene.nu)).astype(np.float32)).to(sim.device))
        sim.step()
    dof = sim._dof_state.cpu().numpy()
    assert np.abs(dof[:, 0::2] - start[:, 0::2]).max(1).min() > 1e-3 and np.abs(dof[:, 1::2] - start[:, 1::2]).max(1).min() > 1e-3     # every env has moved
    root = sim._root_state[0].cpu().numpy().astype(np.float64)
    parts = ic.reference_parts(oracle64, sim._c_model, root, dof[:, 0::2], dof[:, 1::2], qdd[:K])
    check(f"stepped ({step})", sim, all_calls(sim, qdd[:K]), parts, ic.scale(parts), ic.tolerance("franka_panda"))
    sim.stop_sim()


# ---- 4. a contact-scene context with a fixed-base robot ----------------------------------------------------------------------------
def test_contact_scene_context():
    K = 65
    scene, model, root, parts, D, _ = ic.references("panda_gripper")
    sim = make_sim([ic.gravity_actor("panda_gripper")] + jc.GRIPPER_SCENE[1:], K, [[0.0, 0.0, 0.0]])
    assert " step=scene" in kernel_info(sim), kernel_info(sim)
    assert np.array_equal(sim._root_state[0, sim.scene.robot_idx].cpu().numpy(), root[0].astype(np.float32))
    dof, qdd = ic.inputs("panda_gripper")
    set_inputs(sim, dof[:K])
    got = all_calls(sim, qdd[:K])
    check("contact scene panda_gripper", sim, got, {p: v[:K] for p, v in parts.items()}, D, ic.tolerance("panda_gripper"))
    sim.stop_sim()


# ---- 5. two fixed-base robots as one forest -----------------------------------------------------------------------------------------
def test_two_point_robots_are_one_forest(oracle64):
    K = 65
    actors, init = jc.two_point_robot_actors()
    sim = make_sim(actors, K, init)
    n = sim.scene.n_dof
    assert n == 6 and sim._c_model.actors[sim._c_model.robot_actor].gravity == 1
    rng = np.random.default_rng(ic.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(-2.0, 2.0, size=(K, n)), rng.uniform(-ic.QD_AMP, ic.QD_AMP, size=(K, n))
    qdd = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, n)).astype(np.float32)
    set_inputs(sim, dof)
    root = sim._root_state[0].cpu().numpy().astype(np.float64)
    parts = ic.reference_parts(oracle64, sim._c_model, root, dof[:, 0::2], dof[:, 1::2], qdd)
    D, tol = ic.scale(parts), ic.tolerance("point_robot")
    w32 = max(ic.e_tau(ic.restated(sim.scene.robot_model, ic.gravity_in_base(sim._c_model, root), dof, qdd, *call), ic.combine(parts, *call), D)
              for call in ic.ALL_CALLS)
    assert w32 <= 0.1 * tol                                       # the point robot's tolerance fits the forest's inputs
    got = all_calls(sim, qdd)
    check("two point robots", sim, got, parts, D, tol)
    other = np.array(qdd)
    other[:, 3:] = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, 3)).astype(np.float32)
    again = launch(sim, torch.from_numpy(other).to(sim.device), ic.ID_GRAVITY | ic.ID_VELOCITY)
    assert np.array_equal(again[:, :3], got[ic.FULL][:, :3])     # the first robot: bit for bit
    assert np.abs(again[:, 3:] - got[ic.FULL][:, 3:]).max(1).min() > 100.0 * tol * D[3:].min()     # the second robot: every env moved
    sim.stop_sim()


# ---- 6. a tree built on demand ------------------------------------------------------------------------------------------------------
def test_tree_built_on_demand(tmp_path, monkeypatch, oracle64):
    from test_gpu_runtime_tree import actor_yaml, write_branched_urdf
    urdf, actor = str(tmp_path / "branched5.urdf"), str(tmp_path / "arm5.yaml")
    write_branched_urdf(urdf)
    # (its prismatic branch hangs off l1 instead of l2 here: tree [-1,0,0,0,3].  A plugin stays loaded for the rest of the process;
    # test_gpu_runtime_tree.py and test_gpu_jacobian_mass.py assert that THEIR trees - [-1,0,1,0,3], [-1,0,1,0] and [-1,0,1,1,3] - are
    # built when they ask for them)
    text = open(urdf).read()
    assert text.count('<parent link="l2"/><child link="l4"/>') == 1
    with open(urdf, "w") as f:
        f.write(text.replace('<parent link="l2"/><child link="l4"/>', '<parent link="l1"/><child link="l4"/>'))
    actor_yaml(actor, urdf)
    monkeypatch.setenv("MPPI_JIT_CACHE", str(tmp_path / "jit"))
    K = 65
    sim = make_sim([actor], K, [[0.1, -0.2, 0.0]])
    assert "topology=[-1,0,0,0,3]" in kernel_info(sim), kernel_info(sim)
    info = C.create_string_buffer(512)
    capi.check(sim._lib, sim._lib.mppi_jit_info(info, 512))
    assert info.value.decode().startswith("built ") and "topo_m1_0_0_0_3_free" in info.value.decode(), info.value
    n = sim.scene.n_dof
    bodies = sim.scene.robot_model["bodies"]
    lo = np.array([b["lower"] if b["limited"] else -2.0 for b in bodies])
    hi = np.array([b["upper"] if b["limited"] else 2.0 for b in bodies])
    rng = np.random.default_rng(ic.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(lo, hi, size=(K, n)), rng.uniform(-ic.QD_AMP, ic.QD_AMP, size=(K, n))
    qdd = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, n)).astype(np.float32)
    set_inputs(sim, dof)
    root = sim._root_state[0].cpu().numpy().astype(np.float64)
    parts = ic.reference_parts(oracle64, sim._c_model, root, dof[:, 0::2], dof[:, 1::2], qdd)
    D = ic.scale(parts)
    w32 = max(ic.e_tau(ic.restated(sim.scene.robot_model, ic.gravity_in_base(sim._c_model, root), dof, qdd, *call), ic.combine(parts, *call), D)
              for call in ic.ALL_CALLS)
    check("on-demand tree [-1,0,0,0,3]", sim, all_calls(sim, qdd), parts, D, ic.tolerance_from(w32))     # the rule of the cases file on these inputs
    sim.stop_sim()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    lib = boxer._lib
    n = boxer.scene.n_dof
    out = torch.full((K, n), float("nan"), dtype=torch.float32, device=boxer.device)
    qdd = torch.zeros((K, n), dtype=torch.float32, device=boxer.device)
    for q in (qdd, None):
        assert lib.mppi_sim_inverse_dynamics(boxer._ctx, ptr(q), 3, ptr(out)) == capi.MPPI_EUNSUPPORTED
        said = lib.mppi_last_error().decode()
        assert "mppi_sim_inverse_dynamics" in said and "moving base" in said and "unsupported" in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                            # nothing was launched
    boxer.acquire_bias_force_tensor("boxer")
    for call in (boxer.refresh_bias_force_tensors, boxer.inverse_dynamics, lambda: boxer.inverse_dynamics(qdd)):
        with pytest.raises(NotImplementedError, match="moving base"):
            call()
    boxer.stop_sim()
    panda = make_sim([ic.gravity_actor("panda")], K, [[0.0, 0.0, 0.0]])
    n = panda.scene.n_dof
    out = torch.full((K, n), float("nan"), dtype=torch.float32, device=panda.device)
    qdd = torch.zeros((K, n), dtype=torch.float32, device=panda.device)
    assert lib.mppi_sim_inverse_dynamics(panda._ctx, ptr(qdd), 3, None) == capi.MPPI_EINVAL
    assert "null" in lib.mppi_last_error().decode()
    for terms in (4, 7, 8, -1, 1 << 30):
        assert lib.mppi_sim_inverse_dynamics(panda._ctx, ptr(qdd), terms, ptr(out)) == capi.MPPI_EINVAL, terms
        assert "unknown bits" in lib.mppi_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    capi.check(lib, lib.mppi_sim_inverse_dynamics(panda._ctx, ptr(qdd), 3, ptr(out)))      # the context is as healthy as before
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    with pytest.raises(ValueError):
        panda.acquire_bias_force_tensor("no_such_actor")
    panda.stop_sim()


# ---- 8. the wrapper, and through the planner ----------------------------------------------------------------------------------------
class JointForce(object):
    """|tau| of the motion the envs are in: the norm of inverse_dynamics() over the joints"""
    weights = {}

    def __init__(self):
        self.weights = {}

    def reset(self):
        pass

    def compute_cost(self, sim):
        return torch.linalg.norm(sim.inverse_dynamics(), dim=1)


def test_wrapper_and_planner(caplog):
    from mppiisaac.planner.mppi_isaac import MPPIisaacPlanner
    K, H = 16, 3
    q0 = [0.0, -0.94, 0.0, -2.8, 0.0, 1.8675, 0.0]
    qd0 = [0.3, -0.2, 0.1, 0.25, -0.3, 0.2, -0.1]
    cfg = load_config({"defaults": [{"mppi": "panda"}, {"isaacgym": "normal"}], "actors": [ic.gravity_actor("panda"), "goal"],
                       "initial_actor_positions": [[0.0, 0.0, 0.0]], "nx": 14},
                      overrides={"mppi.num_samples": K, "mppi.horizon": H, "mppi.filter_u": False})
    with caplog.at_level(logging.WARNING, logger="mppiisaac"):
        planner = MPPIisaacPlanner(cfg, JointForce())
        planner.compute_action(q0, qd0)
    S = planner.mppi.get_costs().numpy().astype(np.float64)
    said = " | ".join(r.getMessage() for r in caplog.records)
    assert planner.mppi._fused_cost is None and "not traceable" in said and "inverse_dynamics" in said        # not traced, and why
    assert planner.mppi._batch_sig[0] == "per-step" and "runs per step" in said and "per-step only" in said and "inverse dynamics" in said
    assert np.isfinite(S).all() and S.min() > 0.0 and S.max() - S.min() > 1e-3 * S.max()                      # the samples differ
    planner.compute_action(q0, qd0)                          # the second command goes straight to the per-step loop
    assert planner.mppi._batch_sig[0] == "per-step" and np.isfinite(planner.mppi.get_costs().numpy()).all()
    sim = planner.sim
    n = sim.scene.n_dof
    # inside a horizon view all three refuse
    bias = sim.acquire_bias_force_tensor("panda")
    sim.acquire_mass_matrix_tensor("panda")
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (sim.inverse_dynamics, sim.refresh_bias_force_tensors, lambda: sim.acquire_bias_force_tensor("panda")):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "inverse dynamics" in str(e.value)
        with pytest.raises(PerStepOnly, match="link Jacobians and the mass matrix are per-step only"):     # the two earlier callers keep their wording
            sim.refresh_mass_matrix_tensors()
    # the bias tensor is written by refresh only
    sim.refresh_bias_force_tensors()
    b0 = bias.clone()
    assert torch.equal(b0, sim.inverse_dynamics())
    sim.apply_robot_cmd(torch.linspace(-1.0, 1.0, K * sim.scene.nu, device=sim.device).reshape(K, sim.scene.nu))
    sim.step()
    sim.step()
    fresh = sim.inverse_dynamics()
    assert torch.equal(bias, b0) and not torch.equal(bias, fresh)          # stale before a refresh
    sim.refresh_bias_force_tensors()
    assert torch.equal(bias, fresh)                                        # fresh after
    # qdd as [n_dof] (the same for every env) and as [K, n_dof]; anything else raises
    a = torch.linspace(-3.0, 3.0, n, device=sim.device)
    one = sim.inverse_dynamics(a)
    assert tuple(one.shape) == (K, n)
    assert torch.equal(one, sim.inverse_dynamics(a.repeat(K, 1))) and torch.equal(one, sim.inverse_dynamics(a.cpu().numpy()))
    assert not torch.equal(one, fresh)
    for wrong in (torch.zeros(n + 1), torch.zeros(K, n + 1), torch.zeros(K + 1, n), torch.zeros(1, n), torch.zeros(K, n, 1), torch.zeros(())):
        with pytest.raises(ValueError, match="qdd has shape"):
            sim.inverse_dynamics(wrong)
    sim.stop_sim()


# ---- 9. it holds the arm up ---------------------------------------------------------------------------------------------------------
def test_it_holds_the_arm_up():
    scene, model, root, dof0, g_ref, bound, sag, _, _ = ic.hold_case()
    K = ic.HOLD_K
    sim = make_sim([ic.actor_file()], K, [[0.0, 0.0, 0.0]])
    assert sim._c_model.drive_mode == capi.DRIVE_EFFORT and sim._c_model.actors[sim._c_model.robot_actor].gravity == 1
    set_inputs(sim, dof0)
    q0 = dof0[:, 0::2].astype(np.float64)
    D = ic.references("franka_panda")[4]      # (the Panda's torque scales: gravity alone leaves the vertical first joint's at 0)
    worst, e_g = 0.0, 0.0
    for t in range(ic.HOLD_STEPS):
        tau = sim.inverse_dynamics(gravity=True, velocity=False)
        if t == 0:
            e_g = ic.e_tau(tau.cpu().numpy(), g_ref, D)
        sim.apply_robot_cmd(tau)
        sim.step()
        worst = max(worst, np.abs(sim._dof_state.cpu().numpy()[:, 0::2].astype(np.float64) - q0).max())
    print(f"\n[hold] K {K}, {ic.HOLD_STEPS} steps under inverse_dynamics(gravity only): |q - q0| <= {worst:.2e} (bound {bound:.0e}); e_tau of g against g_ref "
          f"{e_g:.1e}; under a zero command the oracle's envs sag by >= {sag.min():.1e}")
    assert worst <= bound
    sim.stop_sim()


# ---- 10. computed torque ------------------------------------------------------------------------------------------------------------
def test_computed_torque_one_step():
    scene, model, root, dof, qdd, tau_ref, cmd_ref, after = ic.torque_case()
    K = len(dof)
    sim = make_sim([ic.actor_file()], K, [[0.0, 0.0, 0.0]], substeps=1)
    m = sim._c_model
    assert m.substeps == 1 and m.drive_mode == capi.DRIVE_EFFORT
    kd, h = float(m.drive_kd), float(m.dt) / int(m.substeps)
    set_inputs(sim, dof)
    qdd_dev = torch.from_numpy(np.array(qdd)).to(sim.device)
    qd_dev = sim.get_dof_state()[:, 1::2]
    tau = sim.inverse_dynamics(qdd_dev)
    cmd = tau + kd * (qd_dev + h * qdd_dev)
    sim.apply_robot_cmd(cmd)
    sim.step()
    got = sim._dof_state.cpu().numpy().astype(np.float64)
    tol_qd = TOL["free"]["qd"]                                # the step matrix's contact-free qd tolerance
    e_ref = np.abs(got[:, 1::2] - after[:, 1::2]).max()
    e_id = np.abs(got[:, 1::2] - dof[:, 1::2].astype(np.float64) - h * qdd.astype(np.float64)).max()
    e_cmd = np.abs(cmd.cpu().numpy().astype(np.float64) - cmd_ref).max()
    print(f"\n[computed torque] K {K}: qd' against the oracle's step under the reference command {e_ref:.2e}, qd' - qd - h qdd {e_id:.2e} (tol {tol_qd:.0e}); "
          f"command against the reference command {e_cmd:.1e} N m")
    assert e_ref <= tol_qd and e_id <= tol_qd
    sim.stop_sim()
