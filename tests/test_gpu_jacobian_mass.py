"""mppi_sim_jacobian / mppi_sim_mass_matrix (csrc/mppi_kernels.hpp k_sim_jacobian, k_sim_mass_matrix) and the wrapper's
acquire_* / refresh_* / get_actor_link_jacobian_by_name on the GPU, against the fp64 oracle at the joint positions the simulator
itself holds: EVERY env, EVERY body, EVERY entry.  Inputs, references, metrics and tolerances: jacobian_cases.py (its conditions
are checked on the oracle alone by test_jacobian_mass.py); the measured maxima are printed next to the tolerances before anything
is asserted.

 1 edges of the staged store: Panda (rows of 42 / 49 floats) at K = 1, 63, 64, 65, 130, gripper Panda (branched, prismatic fingers),
   point robot, heijn and the 12-joint mobile manipulator (even rows of 72 / 144 floats) at K = 65; envs 0-2 at the fixture's joint
   positions, where M meets the URDF route; all bodies in one call, then every body alone - bit for bit the slice
 2 the Panda's base away from the origin and yawed: the same tolerances, the rigid-body positions did move
 3 after two steps with per-env commands, at the stepped joint positions: K = 17 (`lane` step) and K = 65 (`quad` step)
 4 a contact-scene context with a fixed-base robot (gripper Panda, block, table): zero blocks for the table's and the block's bodies
 5 two fixed-base point robots as one forest: exact zeros off the diagonal blocks of M and in the other robot's Jacobian columns
 6 a tree built on demand (the branched arm of test_gpu_runtime_tree.py, one branch moved: a tree of its own): the plugin's launch
   table carries both launchers
 7 in every row: M == M^T bit for bit, Cholesky of every M succeeds, J qd against the rb tensor of mppi_sim_materialise within
   tol(J) sum |qd| + the step matrix's linear / angular velocity tolerance
 8 refusals before any launch: a moving base (MPPI_EUNSUPPORTED, NotImplementedError), a null pointer, a range past n_rb (MPPI_EINVAL)
 9 through the planner: an Objective that costs |J qd| runs per step - neither traced nor on the horizon view - and yields the
   trajectory costs of the Objective that reads the same velocity from the rigid-body row; acquire_* tensors change on refresh only"""
import ctypes as C
import logging

import numpy as np
import pytest
import torch

import jacobian_cases as jc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def kernel_info(sim):
    buf = C.create_string_buffer(512)
    capi.check(sim._lib, sim._lib.mppi_kernel_info(sim._ctx, buf, 512))
    return buf.value.decode()


def launch_all(sim):
    """both tensors of all envs and all rigid bodies through the raw entries, into NaN-filled outputs (every entry must be written)"""
    K, B, n = sim.num_envs, sim.scene.n_rb, sim.scene.n_dof
    J = torch.full((K, B, 6, n), float("nan"), dtype=torch.float32, device=sim.device)
    M = torch.full((K, n, n), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_jacobian(sim._ctx, 0, B, ptr(J)))
    capi.check(sim._lib, sim._lib.mppi_sim_mass_matrix(sim._ctx, ptr(M)))
    return J.cpu().numpy(), M.cpu().numpy()


def each_body_alone_equals_the_slice(sim, J):
    K, B, n = sim.num_envs, sim.scene.n_rb, sim.scene.n_dof
    for b in range(B):
        one = torch.full((K, 6, n), float("nan"), dtype=torch.float32, device=sim.device)
        capi.check(sim._lib, sim._lib.mppi_sim_jacobian(sim._ctx, b, 1, ptr(one)))
        assert np.array_equal(one.cpu().numpy(), J[:, b]), f"body {b} alone differs from its slice"


def check(tag, sim, J, M, J_ref, M_ref, tols, contact=False):
    """prints the measured maxima next to the tolerances, then asserts them and the properties of row 7"""
    tol_J, tol_M = tols
    assert np.isfinite(J).all() and np.isfinite(M).all(), f"{tag}: entries that were never written (or not finite)"
    eJ, eM = jc.e_J(J, J_ref), jc.e_M(M, M_ref)
    dof = sim._dof_state.cpu().numpy().astype(np.float64)
    qd = dof[:, 1::2]
    rb = sim._rigid_body_state.cpu().numpy().astype(np.float64)
    v = np.einsum("kbri,ki->kbr", J.astype(np.float64), qd)
    lin, ang = jc.velocity_tolerances(contact)
    slack = tol_J * np.abs(qd).sum(1)[:, None, None]
    d_lin = np.abs(v[:, :, 0:3] - rb[:, :, 7:10]) - slack
    d_ang = np.abs(v[:, :, 3:6] - rb[:, :, 10:13]) - slack
    print(f"\n[{tag}] K {sim.num_envs}: e_J {eJ:.2e} (tol {tol_J:.0e}) | e_M {eM:.2e} (tol {tol_M:.0e}) | J qd - rb beyond tol(J) sum|qd|: "
          f"lin {max(d_lin.max(), 0.0):.1e} ({lin:.0e}) ang {max(d_ang.max(), 0.0):.1e} ({ang:.0e})")
    assert eJ <= tol_J, f"{tag}: e_J {eJ:.3e} > {tol_J:.0e}"
    assert eM <= tol_M, f"{tag}: e_M {eM:.3e} > {tol_M:.0e}"
    assert np.array_equal(M, M.transpose(0, 2, 1)), f"{tag}: M is not symmetric bit for bit"
    for k in range(len(M)):
        np.linalg.cholesky(M[k].astype(np.float64))
    assert d_lin.max() <= lin and d_ang.max() <= ang, f"{tag}: J qd differs from the rb velocity columns"


def set_inputs(sim, dof):
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    got = sim._dof_state.cpu().numpy()
    assert np.array_equal(got, dof), "the simulator holds other joint states than the inputs"     # (the references were taken at these)
    return got


# ---- 1. edges of the staged store ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", jc.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in jc.STORE_EDGES])
def test_store_edges(robot, K):
    actors, actor_name, _, _ = jc.ROBOTS[robot]
    scene, model, root, J_ref, M_ref, _, _ = jc.references(robot)
    sim = make_sim(actors, K, [[0.0, 0.0, 0.0]])
    assert np.array_equal(sim._root_state[0].cpu().numpy(), root.astype(np.float32))
    set_inputs(sim, jc.inputs(robot)[0][:K])
    J, M = launch_all(sim)
    check(f"edges {robot}", sim, J, M, J_ref[:K], M_ref[:K], jc.tolerances(robot))
    each_body_alone_equals_the_slice(sim, J)
    # the wrapper's tensors: zero until refreshed, then what the raw entries gave
    Jt, Mt = sim.acquire_jacobian_tensor(actor_name), sim.acquire_mass_matrix_tensor(actor_name)
    assert tuple(Jt.shape) == (K, model.n_rb, 6, scene.n_dof) and tuple(Mt.shape) == (K, scene.n_dof, scene.n_dof)
    assert not Jt.any() and not Mt.any()
    sim.refresh_jacobian_tensors()
    sim.refresh_mass_matrix_tensors()
    assert np.array_equal(Jt.cpu().numpy(), J) and np.array_equal(Mt.cpu().numpy(), M)
    last = scene.link_names[-1]
    assert np.array_equal(sim.get_actor_link_jacobian_by_name(actor_name, last).cpu().numpy(), J[:, scene.rigid_body_index(actor_name, last)])
    sim.stop_sim()


# ---- 2. away from the origin --------------------------------------------------------------------------------------------------------
def test_base_away_from_the_origin(oracle64):
    K = 65
    scene, model, root, J_ref, M_ref, _, _ = jc.references("franka_panda", True)
    _, _, root0, _, _, _, _ = jc.references("franka_panda")
    sim = make_sim(["panda"], K, [jc.OFFSET_POS])
    row = np.zeros(13, np.float32)
    row[0:3], row[3:7] = jc.OFFSET_POS, jc.OFFSET_ORI
    sim.set_root_state_tensor_by_actor_idx(torch.from_numpy(row), sim.scene.actor_index("panda"))
    assert np.array_equal(sim._root_state[0].cpu().numpy(), root.astype(np.float32))
    dof = set_inputs(sim, jc.inputs("franka_panda")[0][:K])
    J, M = launch_all(sim)
    check("offset franka_panda", sim, J, M, J_ref[:K], M_ref[:K], jc.tolerances("franka_panda"))
    # the row cannot pass by ignoring the base pose: every link stands where the yawed, shifted base puts it
    pos = sim._rigid_body_state.cpu().numpy()[:, :, 0:3].astype(np.float64)
    c, s = np.cos(jc.OFFSET_YAW), np.sin(jc.OFFSET_YAW)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    worst = 0.0
    for k in range(K):
        p0 = oracle64.rigid_body_state(model, root0, dof[k, 0::2].astype(np.float64), np.zeros(scene.n_dof))[0][:, 0:3]
        worst = max(worst, np.abs(pos[k] - (p0 @ Rz.T + np.asarray(jc.OFFSET_POS))).max())
        assert np.abs(pos[k] - p0).max() > 1.9
    print(f"[offset franka_panda] rigid-body positions against the moved origin ones: {worst:.1e} (1e-5)")
    assert worst < 1e-5      # (fp32 positions 3 m from the origin: 2^-24 x 3 m per term)
    sim.stop_sim()


# ---- 3. after stepping --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,step", [(17, "lane"), (65, "quad")])
def test_after_stepping(K, step, oracle64):
    sim = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    assert f" step={step} " in kernel_info(sim) + " ", kernel_info(sim)
    start = set_inputs(sim, jc.inputs("franka_panda")[0][:K])
    rng = np.random.default_rng(7)
    for _ in range(2):
        sim.apply_robot_cmd(torch.from_numpy(rng.uniform(-1.0, 1.0, size=(K, sim.scene.nu)).astype(np.float32)).to(sim.device))
        sim.step()
    dof = sim._dof_state.cpu().numpy()
    q = dof[:, 0::2].astype(np.float64)
    assert np.abs(dof[:, 0::2] - start[:, 0::2]).max(1).min() > 1e-3       # every env has moved
    root = sim._root_state[0].cpu().numpy().astype(np.float64)
    J_ref, M_ref = jc.oracle_J(oracle64, sim._c_model, root, q), jc.oracle_M(oracle64, sim._c_model, root, q)
    J, M = launch_all(sim)
    check(f"stepped ({step})", sim, J, M, J_ref, M_ref, jc.tolerances("franka_panda"))
    sim.stop_sim()


# ---- 4. a contact-scene context with a fixed-base robot ----------------------------------------------------------------------------
def test_contact_scene_context():
    K = 65
    scene, model, root, J_ref, M_ref, _, _ = jc.references("panda_gripper")
    sim = make_sim(jc.GRIPPER_SCENE, K, [[0.0, 0.0, 0.0]])
    assert " step=scene" in kernel_info(sim), kernel_info(sim)
    first, nl = sim.scene.first_rb[sim.scene.robot_idx], len(sim.scene.link_names)
    assert sim.scene.n_rb == nl + 2 and nl == model.n_rb
    assert np.array_equal(sim._root_state[0, sim.scene.robot_idx].cpu().numpy(), root[0].astype(np.float32))
    set_inputs(sim, jc.inputs("panda_gripper")[0][:K])
    J, M = launch_all(sim)
    full_ref = np.zeros((K, sim.scene.n_rb, 6, scene.n_dof))
    full_ref[:, first:first + nl] = J_ref[:K]
    check("contact scene panda_gripper", sim, J, M, full_ref, M_ref[:K], jc.tolerances("panda_gripper"), contact=True)
    others = [b for b in range(sim.scene.n_rb) if not first <= b < first + nl]
    assert len(others) == 2 and not J[:, others].any()          # the table's and the block's bodies: zero blocks
    each_body_alone_equals_the_slice(sim, J)
    assert tuple(sim.acquire_jacobian_tensor("table").shape) == (K, 1, 6, scene.n_dof)
    sim.refresh_jacobian_tensors()
    assert not sim.acquire_jacobian_tensor("table").any()
    sim.stop_sim()


# ---- 5. two fixed-base robots as one forest -----------------------------------------------------------------------------------------
def test_two_point_robots_are_one_forest(oracle64, oracle32):
    K = 65
    actors, init = jc.two_point_robot_actors()
    sim = make_sim(actors, K, init)
    n = sim.scene.n_dof
    assert n == 6 and sim.scene.nu == 6
    rng = np.random.default_rng(jc.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(-2.0, 2.0, size=(K, n)), rng.uniform(-jc.QD_AMP, jc.QD_AMP, size=(K, n))
    set_inputs(sim, dof)
    q, root = dof[:, 0::2].astype(np.float64), sim._root_state[0].cpu().numpy().astype(np.float64)
    J_ref, M_ref = jc.oracle_J(oracle64, sim._c_model, root, q), jc.oracle_M(oracle64, sim._c_model, root, q)
    w32 = jc.e_J(jc.oracle_J(oracle32, sim._c_model, root, q), J_ref), jc.e_M(jc.oracle_M(oracle32, sim._c_model, root, q), M_ref)
    tols = jc.tolerances("point_robot")
    assert w32[0] <= 0.1 * tols[0] and w32[1] <= 0.1 * tols[1]      # the point robot's tolerances fit the forest's inputs
    J, M = launch_all(sim)
    check("two point robots", sim, J, M, J_ref, M_ref, tols)
    assert not M[:, :3, 3:].any() and not M[:, 3:, :3].any()       # block diagonal, exact zeros
    sim.refresh_jacobian_tensors()      # (nothing acquired yet: a no-op)
    J1, J2 = sim.acquire_jacobian_tensor("point_robot"), sim.acquire_jacobian_tensor("point_robot2")
    sim.refresh_jacobian_tensors()
    J1, J2 = J1.cpu().numpy(), J2.cpu().numpy()
    assert J1.shape[1] + J2.shape[1] == sim.scene.n_rb
    assert np.array_equal(np.concatenate([J1, J2], axis=1), J)
    assert J1[..., :3].any() and not J1[..., 3:].any()             # each robot's links move with its own joints only
    assert J2[..., 3:].any() and not J2[..., :3].any()
    sim.stop_sim()


# ---- 6. a tree built on demand ------------------------------------------------------------------------------------------------------
def test_tree_built_on_demand(tmp_path, monkeypatch, oracle64, oracle32):
    from test_gpu_runtime_tree import actor_yaml, write_branched_urdf
    urdf, actor = str(tmp_path / "branched5.urdf"), str(tmp_path / "arm5.yaml")
    write_branched_urdf(urdf)
    # (its second branch hangs off l2 instead of l1 here: tree [-1,0,1,1,3].  A plugin stays loaded for the rest of the process, and
    # test_gpu_runtime_tree.py asserts that ITS trees - [-1,0,1,0,3] and [-1,0,1,0] - are built, or refused, when it asks for them)
    text = open(urdf).read()
    assert text.count('<parent link="l1"/><child link="l3"/>') == 1
    with open(urdf, "w") as f:
        f.write(text.replace('<parent link="l1"/><child link="l3"/>', '<parent link="l2"/><child link="l3"/>'))
    actor_yaml(actor, urdf)
    monkeypatch.setenv("MPPI_JIT_CACHE", str(tmp_path / "jit"))
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
    rng = np.random.default_rng(jc.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(lo, hi, size=(K, n)), rng.uniform(-jc.QD_AMP, jc.QD_AMP, size=(K, n))
    set_inputs(sim, dof)
    q, root = dof[:, 0::2].astype(np.float64), sim._root_state[0].cpu().numpy().astype(np.float64)
    J_ref, M_ref = jc.oracle_J(oracle64, sim._c_model, root, q), jc.oracle_M(oracle64, sim._c_model, root, q)
    w32 = jc.e_J(jc.oracle_J(oracle32, sim._c_model, root, q), J_ref), jc.e_M(jc.oracle_M(oracle32, sim._c_model, root, q), M_ref)
    tols = tuple(min(jc.round_up_125(10.0 * w), jc.CAP) for w in w32)     # the rule of jacobian_cases.tolerances on these inputs
    J, M = launch_all(sim)
    check("on-demand tree [-1,0,1,1,3]", sim, J, M, J_ref, M_ref, tols)
    each_body_alone_equals_the_slice(sim, J)
    sim.stop_sim()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    lib = boxer._lib
    B, n = boxer.scene.n_rb, boxer.scene.n_dof
    out = torch.full((K, B, 6, n), float("nan"), dtype=torch.float32, device=boxer.device)
    for rc in (lib.mppi_sim_jacobian(boxer._ctx, 0, B, ptr(out)), lib.mppi_sim_mass_matrix(boxer._ctx, ptr(out))):
        assert rc == capi.MPPI_EUNSUPPORTED
        assert "moving base" in lib.mppi_last_error().decode() and "unsupported" in lib.mppi_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                            # nothing was launched
    boxer.acquire_jacobian_tensor("boxer")
    boxer.acquire_mass_matrix_tensor("boxer")
    for call in (boxer.refresh_jacobian_tensors, boxer.refresh_mass_matrix_tensors, lambda: boxer.get_actor_link_jacobian_by_name("boxer", boxer.scene.link_names[0])):
        with pytest.raises(NotImplementedError, match="moving base"):
            call()
    boxer.stop_sim()
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    B, n = panda.scene.n_rb, panda.scene.n_dof
    out = torch.full((K, B + 1, 6, n), float("nan"), dtype=torch.float32, device=panda.device)
    assert lib.mppi_sim_jacobian(panda._ctx, 0, B, None) == capi.MPPI_EINVAL
    assert lib.mppi_sim_mass_matrix(panda._ctx, None) == capi.MPPI_EINVAL
    for first, count in ((B, 1), (0, B + 1), (B - 1, 2), (-1, 1), (0, 0), (0, -1), (1, 2 ** 31 - 1)):
        assert lib.mppi_sim_jacobian(panda._ctx, first, count, ptr(out)) == capi.MPPI_EINVAL, (first, count)
        assert "outside [0, " in lib.mppi_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    capi.check(lib, lib.mppi_sim_jacobian(panda._ctx, B - 1, 1, ptr(out)))      # the context is as healthy as before
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.view(-1)[: K * 6 * n]).all())
    with pytest.raises(ValueError):
        panda.acquire_jacobian_tensor("no_such_actor")
    panda.stop_sim()


# ---- 9. through the planner ---------------------------------------------------------------------------------------------------------
class _Objective(object):
    weights = {}

    def __init__(self):
        self.weights = {}

    def reset(self):
        pass


class JacobianSpeed(_Objective):
    """|J qd| of the Panda's last link, from the link Jacobian"""

    def compute_cost(self, sim):
        J = sim.get_actor_link_jacobian_by_name("panda", "panda_link7")
        qd = sim.get_dof_state()[:, 1::2]
        return torch.linalg.norm(torch.einsum("kri,ki->kr", J, qd), dim=1)


class RowSpeed(_Objective):
    """the same six velocity columns, read from the link's rigid-body row"""

    def compute_cost(self, sim):
        return torch.linalg.norm(sim.get_actor_link_by_name("panda", "panda_link7")[:, 7:13], dim=1)


def test_through_the_planner(monkeypatch, caplog):
    from mppiisaac.planner.mppi_isaac import MPPIisaacPlanner
    K, H = 16, 3
    q0 = [0.0, -0.94, 0.0, -2.8, 0.0, 1.8675, 0.0]
    qd0 = [0.3, -0.2, 0.1, 0.25, -0.3, 0.2, -0.1]

    def plan(objective):
        cfg = load_config({"defaults": [{"mppi": "panda"}, {"isaacgym": "normal"}], "actors": ["panda", "goal"],
                           "initial_actor_positions": [[0.0, 0.0, 0.0]], "nx": 14},
                          overrides={"mppi.num_samples": K, "mppi.horizon": H, "mppi.filter_u": False})
        planner = MPPIisaacPlanner(cfg, objective)
        planner.compute_action(q0, qd0)
        return planner, planner.mppi.get_costs().numpy().astype(np.float64)

    with caplog.at_level(logging.WARNING, logger="mppiisaac"):
        pa, S_a = plan(JacobianSpeed())
    said = " | ".join(r.getMessage() for r in caplog.records)
    assert pa.mppi._fused_cost is None and "not traceable" in said and "get_actor_link_jacobian_by_name" in said     # not traced, and why
    assert pa.mppi._batch_sig[0] == "per-step" and "runs per step" in said and "per-step only" in said              # not batched, and why
    monkeypatch.setenv("MPPI_TRACE_OBJECTIVE", "0")     # the partner stays in generic mode too (on the horizon view)
    pb, S_b = plan(RowSpeed())
    assert pb.mppi._fused_cost is None and pb.mppi._batch_sig[0] in ("ok", "no")
    rel = np.abs(S_a - S_b).max() / np.abs(S_b).max()
    print(f"\n[planner] trajectory costs of |J qd| against |rb row 7:13|: {rel:.1e} relative (1e-4); S in [{S_b.min():.3f}, {S_b.max():.3f}]")
    assert S_b.min() > 0.0 and S_b.max() - S_b.min() > 1e-2 * S_b.max()        # the samples differ: the comparison says something
    assert rel <= 1e-4
    pa.compute_action(q0, qd0)                          # the second command goes straight to the per-step loop
    assert pa.mppi._batch_sig[0] == "per-step" and np.isfinite(pa.mppi.get_costs().numpy()).all()
    # inside a horizon view the accessors refuse
    sim = pa.sim
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (lambda: sim.get_actor_link_jacobian_by_name("panda", "panda_link7"), sim.refresh_jacobian_tensors, sim.refresh_mass_matrix_tensors):
            sim.acquire_jacobian_tensor("panda"), sim.acquire_mass_matrix_tensor("panda")
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly)
    # acquire_* tensors are written by refresh_* only
    Jt, Mt = sim.acquire_jacobian_tensor("panda"), sim.acquire_mass_matrix_tensor("panda")
    sim.refresh_jacobian_tensors()
    sim.refresh_mass_matrix_tensors()
    J0, M0 = Jt.clone(), Mt.clone()
    sim.apply_robot_cmd(torch.linspace(-1.0, 1.0, K * sim.scene.nu, device=sim.device).reshape(K, sim.scene.nu))
    sim.step()
    sim.step()
    fresh = sim.get_actor_link_jacobian_by_name("panda", "panda_link7")
    b = sim.scene.rigid_body_index("panda", "panda_link7") - sim.scene.first_rb[sim.scene.actor_index("panda")]
    assert torch.equal(Jt, J0) and torch.equal(Mt, M0) and not torch.equal(Jt[:, b], fresh)      # stale before a refresh
    sim.refresh_jacobian_tensors()
    sim.refresh_mass_matrix_tensors()
    assert torch.equal(Jt[:, b], fresh) and not torch.equal(Mt, M0)                              # fresh after
    pa.sim.stop_sim()
    pb.sim.stop_sim()
