"""mppi_sim_momentum, mppi_sim_centroidal_matrix and mppi_sim_floating_centroidal_matrix (csrc/mppi_kernels.hpp k_sim_momentum,
k_sim_centroidal_matrix, k_sim_floating_centroidal_matrix) and the wrapper's accessors on the GPU, against the fp64 reference at the
state the simulator itself holds: EVERY env, EVERY entry.  Inputs, reference, metrics and tolerances: centroidal_cases.py (its conditions
are checked on the oracle alone by test_centroidal.py); outputs are NaN-filled before every launch with a guard band behind them that
must stay NaN, and every entry must come back finite; the measured maxima are printed next to the tolerances before anything is asserted.

 1 reference parity at the edges of the staged store: franka_panda and boxer at K = 1, 63, 64, 65, 130, the other robots at K = 65, the
   fixed-base robots also yawed and rolled (K = 65); states in by mppi_sim_set_states
 2 against the device's own tensors, at 10 fp32 epsilons of the scale of each sum: A v against the momentum row, T against v^T M v / 2,
   for a moving base A against the shifted rows 0:6 of the device's M, (A[0:3] / m) v against a centre-of-mass velocity summed in fp64
   from the device's rigid-body rows
 3 inside contact scenes the free actors contribute nothing: the gripper scene (a fixed base), the push scene (a moving base); NaN in
   the block's root velocity reaches no output
 4 inside a captured torch.cuda.graph (a side stream, the default queue count), replayed twice after the states changed: bit-equal to
   eager runs
 5 refusals before any launch, the outputs still all NaN
 6 through the steps, energy: an effort-driven Panda under gravity and zero torque - T + V after every step within the energy tolerance
   of the fp64 oracle's trajectory; the oracle's own drift is printed
 7 through the steps, momentum: a boxer without gravity 1 m above the ground, wheels commanded - no contact force anywhere, p and L
   within tolerance of the oracle's; the oracle's drift is printed

MEASURED on an MI355X (profiles/r22a_gpu_centroidal.txt): see DESIGN.md 5.5i."""
import ctypes as C

import numpy as np
import pytest
import torch

import centroidal_cases as cc
import floating_jacobian_cases as fc
import inverse_dynamics_cases as ic
import jacobian_cases as jc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
BASE_INIT = [[0.0, 0.0, 0.3]]
EPS = cc.EPS32


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _launch(sim, entry, row_len):
    """one raw call into a NaN-filled output with a guard band of one env behind it -> [K][row_len] (numpy)"""
    K = sim.num_envs
    out = torch.full(((K + 1) * row_len,), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, entry(sim._ctx, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * row_len:]).all(), "the guard band behind the output was written"
    assert np.isfinite(got[:K * row_len]).all(), "entries that were never written (or not finite)"
    return got[:K * row_len].reshape(K, row_len)


def momentum(sim):
    return _launch(sim, sim._lib.mppi_sim_momentum, 12)


def matrix(sim):
    moving = cc.is_moving(sim._c_model)
    N = sim.scene.n_dof + (6 if moving else 0)
    entry = sim._lib.mppi_sim_floating_centroidal_matrix if moving else sim._lib.mppi_sim_centroidal_matrix
    return _launch(sim, entry, 6 * N).reshape(sim.num_envs, 6, N)


def push_fixed(sim, dof):
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    got = sim._dof_state.cpu().numpy()
    assert np.array_equal(got, dof), "the simulator holds other joint states than the inputs"
    return got


def push_moving(sim, dof, roots):
    """the per-env states in through mppi_sim_set_states -> (dof, roots) as the simulator holds them"""
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    sim.set_actor_root_state_tensor(torch.from_numpy(np.array(roots, np.float32)))
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.array_equal(held_dof, dof) and np.array_equal(held_roots[:, a, 3:13], roots[:, a, 3:13])
    assert np.abs(held_roots[:, a, 0:3] - roots[:, a, 0:3]).max() <= 1e-6       # (x, y pass through the scene's relative coordinates)
    return held_dof, held_roots


def place_base(sim, actor_name, pos, ori):
    row = np.zeros(13, np.float32)
    row[0:3], row[3:7] = pos, ori
    sim.set_root_state_tensor_by_actor_idx(torch.from_numpy(row), sim.scene.actor_index(actor_name))


def check(tag, sim, ref, D, tol):
    rows, A = momentum(sim), matrix(sim)
    e = cc.errors(cc.split(rows, A), ref, D)
    print("\n" + cc.report(f"{tag}, K {sim.num_envs}: error (tolerance)", e, tol))
    assert cc.within(e, tol), {k: (v, tol[k]) for k, v in e.items() if v > tol[k]}
    return rows, A


def fixed_sim(robot, pose, K, extra=()):
    actors, name, _, _ = ic.ROBOTS[robot]
    tilted = pose == "tilted"
    sim = make_sim([ic.gravity_actor(a) for a in actors] + list(extra), K, [jc.OFFSET_POS if tilted else [0.0, 0.0, 0.0]])
    if tilted:
        place_base(sim, name, jc.OFFSET_POS, ic.TILT_ORI)
    root = cc.fixed_inputs(robot, pose)[1]
    assert np.array_equal(sim._root_state[0, sim.scene.robot_idx].cpu().numpy(), root[sim.scene.robot_idx].astype(np.float32))
    assert sim._c_model.actors[sim._c_model.robot_actor].gravity == 1
    return sim


def slice_ref(r, K):
    return {name: a[:K] for name, a in r.ref.items()}


# ---- 1. reference parity at the edges of the staged store ---------------------------------------------------------------------------
FIXED_PARITY = [(r, "origin", K) for r, K in cc.FIXED_STORE_EDGES] + [(r, "tilted", 65) for r in cc.FIXED_ROBOTS]


@pytest.mark.parametrize("robot,pose,K", FIXED_PARITY, ids=[f"{r}-{p}-K{K}" for r, p, K in FIXED_PARITY])
def test_fixed_base_parity(robot, pose, K):
    sim = fixed_sim(robot, pose, K)
    r = cc.fixed_references(robot, pose)
    push_fixed(sim, cc.fixed_inputs(robot, pose)[0][:K])
    rows, A = check(f"{robot} {pose}", sim, slice_ref(r, K), r.D, cc.tolerances(robot))
    # the wrapper: zero until refreshed, then what the raw calls gave
    name = ic.ROBOTS[robot][1]
    t, At = sim.acquire_momentum_tensor(name), sim.acquire_centroidal_matrix_tensor(name)
    assert tuple(t.shape) == (K, 12) and not t.any() and not At.any() and sim.acquire_momentum_tensor(name) is t
    sim.refresh_momentum_tensors()
    sim.refresh_centroidal_matrix_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(rows)) and np.array_equal(bits(At.cpu().numpy()), bits(A))
    assert np.array_equal(bits(sim.centre_of_mass().cpu().numpy()), bits(rows[:, 1:4])) and np.array_equal(bits(sim.robot_momentum().cpu().numpy()), bits(rows[:, 4:10]))
    assert np.array_equal(bits(sim.kinetic_energy().cpu().numpy()), bits(rows[:, 10])) and np.array_equal(bits(sim.potential_energy().cpu().numpy()), bits(rows[:, 11]))
    assert np.allclose(sim.com_jacobian(name).cpu().numpy(), A[:, 0:3] / rows[:, 0, None, None], rtol=4 * EPS, atol=0.0)        # (one division per entry)
    sim.stop_sim()


@pytest.mark.parametrize("robot,K", cc.MOVING_STORE_EDGES, ids=[f"{r}-K{K}" for r, K in cc.MOVING_STORE_EDGES])
def test_moving_base_parity(robot, K):
    actors, name, _ = fc.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    assert sim._c_model.actors[sim._c_model.robot_actor].gravity == 1
    dof, roots = cc.moving_inputs(robot)
    held_dof, held_roots = push_moving(sim, dof[:K], roots[:K])
    r = cc.references_at(sim.scene, sim._c_model, held_roots, held_dof)               # at what the simulator holds
    tol = cc.tolerances(robot)
    rows, A = check(robot, sim, r.ref, cc.moving_references(robot).D, tol)
    assert np.abs(rows[:, 11]).min() > 0.0 and not A[:, 3:6, 0:3].any()
    At = sim.acquire_floating_centroidal_matrix_tensor(name)
    sim.refresh_floating_centroidal_matrix_tensors()
    assert np.array_equal(bits(At.cpu().numpy()), bits(A))
    assert np.allclose(sim.com_jacobian(name).cpu().numpy(), A[:, 0:3] / rows[:, 0, None, None], rtol=4 * EPS, atol=0.0)        # (one division per entry)
    sim.stop_sim()


# ---- 2. against the device's own tensors --------------------------------------------------------------------------------------------
def device_consistency(tag, sim, v, p_base):
    """the four comparisons of row 2; v [K][N] fp64, p_base [K][3] fp64.  Every bound is 10 eps x the sum of the magnitudes that enter."""
    K, moving = sim.num_envs, cc.is_moving(sim._c_model)
    rows, A = momentum(sim).astype(np.float64), matrix(sim).astype(np.float64)
    N = A.shape[2]
    M = torch.full((K, N, N), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, (sim._lib.mppi_sim_floating_mass_matrix if moving else sim._lib.mppi_sim_mass_matrix)(sim._ctx, ptr(M)))
    M = M.cpu().numpy().astype(np.float64)
    rb = sim._rigid_body_state.cpu().numpy().astype(np.float64)
    a = int(sim._c_model.robot_actor)
    first, L = int(sim._c_model.actors[a].first_rb), int(sim._c_model.actors[a].n_rb)
    r = rows[:, 1:4] - p_base
    reach = np.linalg.norm(rb[:, first:first + L, 0:3] - p_base[:, None, :], axis=2).max(1)       # the longest lever arm of the env
    # A v against (p, L): the angular sums are taken about the base origin and moved by r
    Av = np.einsum("kri,ki->kr", A, v)
    terms = np.einsum("kri,ki->kr", np.abs(A), np.abs(v))
    lever = (np.linalg.norm(r, axis=1) + reach)[:, None] * np.linalg.norm(terms[:, 0:3], axis=1)[:, None]
    bound = 10 * EPS * np.concatenate([terms[:, 0:3], terms[:, 3:6] + lever], axis=1)
    e_Av = float((np.abs(Av - rows[:, 4:10]) / bound).max())
    # T against v^T M v / 2
    T = 0.5 * np.einsum("ki,kij,kj->k", v, M, v)
    bound_T = 10 * EPS * 0.5 * np.einsum("ki,kij,kj->k", np.abs(v), np.abs(M), np.abs(v))
    e_T = float((np.abs(T - rows[:, 10]) / bound_T).max())
    # (A[0:3] / m) v against the centre-of-mass velocity of the device's own rigid-body rows
    # (both sides are fp32 results: the bound is the scale of A v / m plus the scale of what the rigid-body rows themselves carry)
    vc, rb_scale = cc.com_velocity_from_links(sim._c_model, rb)
    e_vc = float((np.abs(Av[:, 0:3] / rows[:, 0:1] - vc) / (10 * EPS * (terms[:, 0:3] / rows[:, 0:1] + rb_scale[:, None]))).max())
    out = {"A v": e_Av, "T": e_T, "com velocity": e_vc}
    if moving:  # A against the shifted rows 0:6 of the device's M
        shifted = cc.shifted_mass_rows(M, r)
        col = np.linalg.norm(M[:, 0:3, :], axis=1)                                                  # |f_j| of every column
        bound_A = 10 * EPS * np.concatenate([np.abs(M[:, 0:3, :]) + 1e-30, np.abs(M[:, 3:6, :]) + ((np.linalg.norm(r, axis=1) + reach)[:, None] * col)[:, None, :]], axis=1)
        out["A against M"] = float((np.abs(A - shifted) / bound_A).max())
    print(f"\n[{tag}] K {K}, in units of the bound (10 eps x the scale of the sum): " + ", ".join(f"{k} {x:.2f}" for k, x in out.items()))
    assert max(out.values()) <= 1.0, out


# (not the mobile manipulator: its inputs stand up to 500 m out and turn by hundreds of radians, where the rigid-body rows' own velocity
# columns - formed about the world origin - carry 1e-4 m/s of rounding through a chain of twelve bodies; its parity is row 1's)
@pytest.mark.parametrize("robot", ["franka_panda", "panda_gripper"])
def test_fixed_base_against_the_devices_own_tensors(robot):
    K = 65
    sim = fixed_sim(robot, "tilted", K)
    dof = push_fixed(sim, cc.fixed_inputs(robot, "tilted")[0][:K])
    p_base = np.tile(cc.fixed_inputs(robot, "tilted")[1][sim.scene.robot_idx, 0:3], (K, 1))
    device_consistency(f"{robot} tilted", sim, dof[:, 1::2].astype(np.float64), p_base)
    sim.stop_sim()


@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_moving_base_against_the_devices_own_tensors(robot):
    K = 65
    sim = make_sim(fc.ROBOTS[robot][0], K, BASE_INIT)
    dof, roots = cc.moving_inputs(robot)
    held_dof, held_roots = push_moving(sim, dof[:K], roots[:K])
    a = sim.scene.robot_idx
    device_consistency(robot, sim, fc.generalised_velocity(held_dof, held_roots, a), held_roots[:, a, 0:3].astype(np.float64))
    sim.stop_sim()


# ---- 3. inside contact scenes -------------------------------------------------------------------------------------------------------
def poison_block_velocity(sim, block):
    roots = sim._root_state.cpu().numpy().copy()
    roots[:, sim.scene.actor_index(block), 7:13] = np.nan
    sim.set_actor_root_state_tensor(torch.from_numpy(roots))
    assert np.isnan(sim._root_state.cpu().numpy()[:, sim.scene.actor_index(block), 7:13]).all()


def test_gripper_scene_a_fixed_base_inside_a_contact_scene():
    K = 65
    sim = fixed_sim("panda_gripper", "origin", K, extra=cc.GRIPPER_SCENE[1:])
    assert int(sim._c_model.n_actors) == 3
    r = cc.fixed_references("panda_gripper")
    push_fixed(sim, cc.fixed_inputs("panda_gripper")[0][:K])
    rows, A = check("gripper scene", sim, slice_ref(r, K), r.D, cc.tolerances("panda_gripper"))
    poison_block_velocity(sim, cc.GRIPPER_SCENE[1])
    assert np.array_equal(bits(momentum(sim)), bits(rows)) and np.array_equal(bits(matrix(sim)), bits(A))
    sim.stop_sim()


def test_push_scene_a_moving_base_with_a_free_and_a_static_actor():
    K = 65
    sim = make_sim(cc.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    dof0, roots0 = fc.draw_inputs(sim.scene, K)
    dof, roots, _ = cc.fi.draw_rates(dof0, roots0, sim.scene.robot_idx)
    held_dof, held_roots = push_moving(sim, dof, roots)
    r = cc.references_at(sim.scene, sim._c_model, held_roots, held_dof)
    tol = cc.tolerances("boxer")
    assert all(r.w32[k] <= 0.5 * tol[k] for k in tol if tol[k] > 0.0)                  # boxer's tolerances fit the scene's inputs
    assert int(sim._c_model.n_actors) == 3
    rows, A = check("push scene", sim, r.ref, r.D, tol)
    poison_block_velocity(sim, cc.PUSH_SCENE[1])
    assert np.array_equal(bits(momentum(sim)), bits(rows)) and np.array_equal(bits(matrix(sim)), bits(A))
    sim.stop_sim()


# ---- 4. inside a captured graph -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["albert", "franka_panda"])
def test_the_entries_replay_from_a_captured_graph(robot):
    K = 32
    moving = robot in cc.MOVING_ROBOTS
    if moving:
        sim = make_sim(fc.ROBOTS[robot][0], K, BASE_INIT)
        dof, roots = cc.moving_inputs(robot)
        states = [(np.ascontiguousarray(dof[i * K:(i + 1) * K]), np.ascontiguousarray(roots[i * K:(i + 1) * K])) for i in range(2)]
        put = lambda s: push_moving(sim, *s)
    else:
        sim = fixed_sim(robot, "origin", K)
        dof = cc.fixed_inputs(robot)[0]
        states = [np.ascontiguousarray(dof[i * K:(i + 1) * K]) for i in range(2)]
        put = lambda s: push_fixed(sim, s)
    put(states[0])
    eager = (momentum(sim), matrix(sim))                            # (also the warm-up outside the capture)
    N = eager[1].shape[2]
    rows = torch.full((K, 12), float("nan"), dtype=torch.float32, device=sim.device)
    A = torch.full((K, 6, N), float("nan"), dtype=torch.float32, device=sim.device)
    lib, ctx = sim._lib, sim._ctx
    entry = lib.mppi_sim_floating_centroidal_matrix if moving else lib.mppi_sim_centroidal_matrix
    torch.cuda.synchronize()
    g, main = torch.cuda.CUDAGraph(), torch.cuda.current_stream()
    try:
        with torch.cuda.graph(g):      # torch's side stream; two launches one after the other: no parallel branches
            capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            capi.check(lib, lib.mppi_sim_momentum(ctx, ptr(rows)))
            capi.check(lib, entry(ctx, ptr(A)))
    finally:
        capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(main.cuda_stream)))
    for s, want in ((states[1], None), (states[0], eager)):        # two replays, each after the states changed
        put(s)
        rows.fill_(float("nan"))
        A.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        got = (rows.cpu().numpy(), A.cpu().numpy())
        want = want or (momentum(sim), matrix(sim))
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        if s is states[1]:
            assert not np.array_equal(bits(got[0]), bits(eager[0]))
    sim.stop_sim()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    K = 8
    out = None

    def refused(sim, entry, code, *words):
        assert entry(sim._ctx, ptr(out)) == code
        said = sim._lib.mppi_last_error().decode()
        assert all(w in said for w in words), said
        return said
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    lib = panda._lib
    out = torch.full((K * 6 * 32,), float("nan"), dtype=torch.float32, device=panda.device)
    refused(panda, lib.mppi_sim_floating_centroidal_matrix, capi.MPPI_EUNSUPPORTED, "mppi_sim_floating_centroidal_matrix", "fixed base", "use mppi_sim_centroidal_matrix")
    panda.acquire_floating_centroidal_matrix_tensor("panda")
    with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_centroidal_matrix"):
        panda.refresh_floating_centroidal_matrix_tensors()
    with panda._horizon_view(dict(panda._state_t_own), K):
        for call in (lambda: panda.acquire_momentum_tensor("panda"), panda.refresh_momentum_tensors, panda.centre_of_mass, lambda: panda.com_jacobian("panda")):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly)
    for entry in (lib.mppi_sim_momentum, lib.mppi_sim_centroidal_matrix, lib.mppi_sim_floating_centroidal_matrix):
        assert entry(panda._ctx, None) == capi.MPPI_EINVAL and "null output" in lib.mppi_last_error().decode()
    panda.stop_sim()
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    refused(boxer, lib.mppi_sim_centroidal_matrix, capi.MPPI_EUNSUPPORTED, "mppi_sim_centroidal_matrix", "moving base", "use mppi_sim_floating_centroidal_matrix")
    boxer.acquire_centroidal_matrix_tensor("boxer")
    with pytest.raises(NotImplementedError, match="moving base .* use mppi_sim_floating_centroidal_matrix"):
        boxer.refresh_centroidal_matrix_tensors()
    for entry in (lib.mppi_sim_momentum, lib.mppi_sim_centroidal_matrix, lib.mppi_sim_floating_centroidal_matrix):
        assert entry(boxer._ctx, None) == capi.MPPI_EINVAL and "null output" in lib.mppi_last_error().decode()
    boxer.stop_sim()
    # the forest of two jackals (conf/mppi/multi-jackal.yaml)
    two = make_sim(["jackal_a", "jackal_b"], K, [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    assert int(two._c_model.n_extra_bases) == 1
    for entry in (lib.mppi_sim_momentum, lib.mppi_sim_centroidal_matrix, lib.mppi_sim_floating_centroidal_matrix):
        said = refused(two, entry, capi.MPPI_EUNSUPPORTED, "several moving bases")
        assert "fixed base" not in said
    two.acquire_momentum_tensor("jackal_a")
    with pytest.raises(NotImplementedError, match="several moving bases"):
        two.refresh_momentum_tensors()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                             # none of these launched anything
    two.stop_sim()


# ---- 6. through the steps: energy ---------------------------------------------------------------------------------------------------
def test_energy_through_the_steps_follows_the_oracle():
    case = cc.energy_case()
    K = cc.ENERGY_K
    sim = make_sim([ic.actor_file()], K, [[0.0, 0.0, 0.0]])
    assert np.array_equal(sim._root_state[0].cpu().numpy(), case.root.astype(np.float32))
    push_fixed(sim, case.dof0)
    zero = torch.zeros((K, sim.scene.nu), dtype=torch.float32, device=sim.device)
    E0 = (sim.kinetic_energy() + sim.potential_energy()).cpu().numpy().astype(np.float64)
    E = []
    for _ in range(cc.STEPS):
        sim.apply_robot_cmd(zero)
        sim.step()
        E.append((sim.kinetic_energy() + sim.potential_energy()).cpu().numpy().astype(np.float64))
    E = np.stack(E)
    e = np.abs(E - case.E).max(1) / case.D
    drift = case.E[-1] - case.E0
    print(f"\n[energy] T + V of the device against the fp64 oracle's trajectory, of the scale {case.D:.1f} J: after step 1 {e[0]:.1e}, 10 {e[9]:.1e}, 25 {e[24]:.1e}, "
          f"50 {e[49]:.1e}, worst {e.max():.1e} (tol {case.tol:.0e}, fp32 oracle {case.w32:.1e}); at the start {np.abs(E0 - case.E0).max() / case.D:.1e}")
    print(f"[energy] the ORACLE's own drift of T + V over {cc.STEPS} steps (zero torque; the drive's damping kd = {float(case.model.drive_kd):g} and the joint limits "
          f"take energy out, the integrator is semi-implicit): from {drift.min():.2f} to {drift.max():.2f} J of {case.E0.min():.1f} .. {case.E0.max():.1f} J")
    assert np.abs(E0 - case.E0).max() / case.D <= case.tol and e.max() <= case.tol
    sim.stop_sim()


# ---- 7. through the steps: momentum -------------------------------------------------------------------------------------------------
def test_momentum_through_the_steps_follows_the_oracle():
    case = cc.momentum_case()
    K = cc.MOMENTUM_K
    sim = make_sim([cc.boxer_actor_file()], K, [[0.0, 0.0, cc.BOXER_HEIGHT]])
    assert sim._c_model.actors[sim._c_model.robot_actor].gravity == 0 and not np.abs(case.cf).max()
    push_moving(sim, case.dof0, case.roots0)
    u = torch.from_numpy(case.u).to(sim.device)
    rows, touched = [], 0.0
    t = sim.acquire_momentum_tensor("boxer")
    for _ in range(cc.STEPS):
        sim.apply_robot_cmd(u)
        sim.step()
        touched = max(touched, float(sim._net_contact_force.abs().max()))
        sim.refresh_momentum_tensors()
        rows.append(t.cpu().numpy().astype(np.float64))
    rows = np.stack(rows)
    assert touched == 0.0                                           # the contact-force tensor is all zeros: nothing touched the robot
    assert not rows[:, :, 11].any()                                 # no gravity: V is exact zeros
    e = {name: np.abs(rows[:, :, cc.COLS[name]] - case.rows[:, :, cc.COLS[name]]).max((1, 2)) / case.D[name] for name in ("p", "L")}
    drift = {name: np.abs(case.rows[:, :, cc.COLS[name]] - case.rows0[None, :, cc.COLS[name]]).max() for name in ("p", "L")}
    for name in ("p", "L"):
        print(f"\n[momentum] {name} of the device against the fp64 oracle's trajectory, of the scale {case.D[name]:.3g}: after step 1 {e[name][0]:.1e}, 25 {e[name][24]:.1e}, "
              f"50 {e[name][49]:.1e}, worst {e[name].max():.1e} (tol {case.tol[name]:.0e}, fp32 oracle {case.w32[name]:.1e})")
    print(f"[momentum] the ORACLE's own drift over {cc.STEPS} steps without any external force: p {drift['p']:.2e} of {case.D['p']:.3g} kg m/s, "
          f"L {drift['L']:.2e} of {case.D['L']:.3g} kg m^2/s (the semi-implicit step)")
    assert e["p"].max() <= case.tol["p"] and e["L"].max() <= case.tol["L"]
    sim.stop_sim()
