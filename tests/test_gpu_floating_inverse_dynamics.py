"""mppi_sim_floating_inverse_dynamics (csrc/mppi_kernels.hpp k_sim_floating_inverse_dynamics) and the wrapper's
floating_inverse_dynamics / acquire_floating_bias_force_tensor / refresh_floating_bias_force_tensors on the GPU, against the fp64
reference at the state the simulator itself holds (its dof and root tensors read back through mppi_sim_materialise and widened):
EVERY env, EVERY row, EVERY part.  Inputs, reference, metric and tolerances: floating_inverse_dynamics_cases.py (its conditions are
checked on the oracle alone by test_floating_inverse_dynamics.py); outputs are NaN-filled before every launch with a guard band behind
them that must stay NaN, and every entry must come back finite; the measured maxima are printed next to the tolerances before
anything is asserted.

 1 edges of the staged load and store: boxer (rows of 8 floats) at K = 1, 63, 64, 65, 130; jackal_a (10), albert (15), anymal (18) at
   K = 65 - every env with joint positions, rates, a base pose and a base twist of its own, pushed with mppi_sim_set_states; the eight
   combinations of terms and vd; terms = 0 without vd gives exact zeros; equality with the host build's figures to the tolerance
 2 a contact scene with a free and a static actor (boxer + block + obstacle)
 3 live state: after two steps of boxer on the ground the references are taken at the materialised state; the start state's
   references are far off
 4 device against device: terms = 0 on vd = e_c reproduces column c of mppi_sim_floating_mass_matrix; tau^T v of the velocity part is
   the finite-difference power v^T Mdot v / 2 of the reference
 5 with every base translated by (420, -310, 0) tau comes out bit for bit the same
 6 the launch inside a captured torch.cuda.graph (one stream), replayed after the states were changed by mppi_sim_set_states:
   bit-equal to a direct call at the new states
 7 the wrapper: the acquired tensor changes on refresh only; PerStepOnly on a horizon view; NotImplementedError with the library's
   text for the Panda
 8 refusals before any launch, the output still all NaN: a fixed-base Panda, the forest of two jackals, a null output, unknown bits;
   the six fixed-base entries keep refusing boxer with their text
(No on-demand moving-base tree is built here - its scene unit takes tens of seconds; test_floating_inverse_dynamics.py shows that the
plugin units fill the pointer through the same function.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BASE_INIT = [[0.0, 0.0, 0.3]]
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(sim, vd, terms):
    """one raw call into a NaN-filled output with a guard band of one env behind it -> tau [K][6 + n] (numpy).  vd: numpy [K][6 + n] or None"""
    K, N = sim.num_envs, 6 + sim.scene.n_dof
    out = torch.full(((K + 1) * N,), float("nan"), dtype=torch.float32, device=sim.device)
    vd_t = torch.from_numpy(np.array(vd, np.float32)).to(sim.device) if vd is not None else None
    capi.check(sim._lib, sim._lib.mppi_sim_floating_inverse_dynamics(sim._ctx, ptr(vd_t), terms, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * N:]).all(), "the guard band behind tau was written"
    assert np.isfinite(got[:K * N]).all(), "entries that were never written (or not finite)"
    return got[:K * N].reshape(K, N)


def push(sim, dof, roots):
    """the per-env states in through mppi_sim_set_states -> (dof, roots) as the simulator holds them, read back through
    mppi_sim_materialise (the joints, the base orientations and the twists exactly the inputs)"""
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    sim.set_actor_root_state_tensor(torch.from_numpy(np.array(roots, np.float32)))
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.array_equal(held_dof, dof) and np.array_equal(held_roots[:, a, 3:13], roots[:, a, 3:13])
    assert np.abs(held_roots[:, a, 0:3] - roots[:, a, 0:3]).max() <= 1e-6       # (x, y pass through the scene's relative coordinates)
    return held_dof, held_roots


def check_calls(tag, sim, r, vd, tol, calls=fi.ALL_CALLS):
    """every call shape against the reference's combination -> {call: tau}"""
    got, worst = {}, {}
    for terms, with_vd in calls:
        got[terms, with_vd] = launch(sim, vd if with_vd else None, terms)
        worst[terms, with_vd] = fi.e_tau(got[terms, with_vd], fi.combine(r.parts, terms, with_vd), r.force_rows)
    print(f"\n[{tag}] K {sim.num_envs}: e per call (terms, vd given): " + ", ".join(f"{t}{'+vd' if w else ''} {e:.1e}" for (t, w), e in worst.items())
          + f"; tol {tol:.0e}, fp32 restatement {r.w32:.1e}, Richardson gap {r.gap:.1e}")
    assert r.gap <= fi.RICHARDSON_AGREE
    for call, e in worst.items():
        assert e <= tol, f"{tag} {call}: e {e:.3e} > {tol:.0e}"
    return got


@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_inverse_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_inverse_dynamics_hostemu.so"))


# ---- 1. edges of the staged load and store ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", fi.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in fi.STORE_EDGES])
def test_store_edges(robot, K, hostemu):
    actors, _, _ = fi.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, vd = fi.inputs(robot)
    held_dof, held_roots = push(sim, dof[:K], roots[:K])
    r = fi.references_at(sim.scene, sim._c_model, held_roots, held_dof, vd[:K])       # at what the simulator holds
    tol = fi.tolerance(robot)
    assert fi.tolerance_from(r.w32) == tol
    got = check_calls(f"edges {robot}", sim, r, vd[:K], tol)
    assert not got[0, False].any()                                  # nothing asked for: exact zeros
    assert not got[fi.ID_GRAVITY, False][:, 0:2].any()              # the weight has no x / y force
    # the host build's figures, to the tolerance
    n = sim.scene.n_dof
    host = np.full((K, 6 + n), np.nan, np.float32)
    q, qd = np.ascontiguousarray(held_dof[:, 0::2]), np.ascontiguousarray(held_dof[:, 1::2])
    assert hostemu.emu_floating_inverse_dynamics(C.byref(sim._c_model), K, fp(np.ascontiguousarray(held_roots)), fp(q), fp(qd),
                                                 fp(np.ascontiguousarray(vd[:K])), 3, fp(host)) == 0
    e = fi.e_tau(got[fi.FULL], host.astype(np.float64), r.force_rows)
    print(f"[edges {robot}] against the host build: e {e:.2e}")
    assert e <= tol
    sim.stop_sim()


# ---- 2. a contact scene with a free and a static actor ------------------------------------------------------------------------------
def test_contact_scene_with_a_free_and_a_static_actor():
    K = 65
    sim = make_sim(fi.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    dof0, roots0 = fc.draw_inputs(sim.scene, K)
    dof, roots, vd = fi.draw_rates(dof0, roots0, sim.scene.robot_idx)
    held_dof, held_roots = push(sim, dof, roots)
    r = fi.references_at(sim.scene, sim._c_model, held_roots, held_dof, vd)
    tol = fi.tolerance("boxer")
    assert fi.tolerance_from(r.w32) == tol                          # boxer's tolerance fits the scene's inputs
    assert int(sim._c_model.n_actors) == 3 and int(sim._c_model.n_rb) == int(sim._c_model.actors[sim.scene.robot_idx].n_rb) + 2
    check_calls("boxer + block + obstacle", sim, r, vd, tol, fi.CALLS)
    sim.stop_sim()


# ---- 3. live state ------------------------------------------------------------------------------------------------------------------
def test_live_state_after_two_steps():
    K = 65
    sim = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    u = torch.from_numpy(np.random.default_rng(fi.SEED).uniform(-1.0, 1.0, size=(K, sim.scene.nu)).astype(np.float32)).to(sim.device)
    start_dof, start = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    for _ in range(2):
        sim.apply_robot_cmd(u)
        sim.step()
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.abs(held_roots[:, a, 3:7] - start[:, a, 3:7]).max() > 1e-3 and np.abs(held_roots[:, a, 7:13]).max() > 1e-2     # turned and moving
    vd = fi.inputs("boxer")[2][:K]
    r = fi.references_at(sim.scene, sim._c_model, held_roots, held_dof, vd)
    tol = fi.tolerance("boxer")
    got = check_calls("boxer after two steps", sim, r, vd, tol, fi.CALLS)
    # the kernel reads the live per-env base and rates, not x0: the references at the start state are off by hundreds of tolerances
    x0 = fi.references_at(sim.scene, sim._c_model, start, start_dof, vd)
    off = fi.e_tau(got[fi.FULL], fi.combine(x0.parts, *fi.FULL), r.force_rows)
    print(f"[boxer after two steps] the start state's references are off by {off:.1e}")
    assert off > 100.0 * tol
    sim.stop_sim()


# ---- 4. device against device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_unit_accelerations_give_the_mass_matrix_and_the_velocity_part_its_power(robot, oracle64):
    K = 65
    actors, _, _ = fi.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, vd = fi.inputs(robot)
    held_dof, held_roots = push(sim, dof[:K], roots[:K])
    N = 6 + sim.scene.n_dof
    M = torch.full((K, N, N), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_floating_mass_matrix(sim._ctx, ptr(M)))
    M = M.cpu().numpy()
    # column c of M: the same sums by another routine (composite inertias there, a Newton-Euler pass here) - to the mass-matrix
    # tests' own tolerance and metric
    cols = np.stack([launch(sim, np.tile(np.eye(N, dtype=np.float32)[c], (K, 1)), 0) for c in range(N)], axis=2)
    tol_M = fc.tolerances(robot)[1]
    eM = fc.e_M(cols, M.astype(np.float64))
    print(f"\n[{robot}] terms = 0 on vd = e_c against mppi_sim_floating_mass_matrix: e_M {eM:.2e} (tol {tol_M:.0e})")
    assert eM <= tol_M
    # the power of the velocity part against the finite-difference power of the reference
    tol = fi.tolerance(robot)
    Cv = launch(sim, None, fi.ID_VELOCITY).astype(np.float64)
    v = fc.generalised_velocity(held_dof, held_roots, sim.scene.robot_idx)
    ref = fi.references(robot)
    scale_C = np.abs(ref.parts["C"]).max(0)
    worst = 0.0
    for k in range(0, K, 8):
        gap, power = fi.power_gap(oracle64, sim._c_model, held_roots[k], held_dof[k, 0::2].astype(np.float64), v[k], ref.parts["C"][k])
        assert abs(gap) <= 1e-8 * scale_C.max()
        # |v^T (C v - ref)| <= sum_j |v_j| tol D_j
        bound = tol * float(np.abs(v[k]) @ fi.scale(ref.parts["C"], ref.force_rows))
        worst = max(worst, abs(float(v[k] @ Cv[k]) - (power - gap)) / bound)
    print(f"[{robot}] tau^T v of the velocity part against v^T Mdot v / 2: {worst:.2e} of the bound")
    assert worst <= 1.0
    sim.stop_sim()


# ---- 5. translation independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_result_does_not_depend_on_where_the_base_stands(robot):
    K = 65
    actors, _, _ = fi.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, vd = fi.inputs(robot)
    push(sim, dof[:K], roots[:K])
    tau = launch(sim, vd[:K], 3)
    far = np.array(roots[:K])
    a = sim.scene.robot_idx
    far[:, a, 0:3] += np.asarray(fi.FAR_SHIFT, np.float32)
    sim.set_actor_root_state_tensor(torch.from_numpy(far))
    held = sim._root_state.cpu().numpy()[:, a]
    assert np.abs(held[:, 0] - far[:, a, 0]).max() <= 1e-4 and held[:, 0].min() > 400.0 and np.array_equal(held[:, 3:13], far[:, a, 3:13])
    assert np.array_equal(bits(launch(sim, vd[:K], 3)), bits(tau))
    sim.stop_sim()


# ---- 6. inside a captured graph -----------------------------------------------------------------------------------------------------
def test_the_entry_replays_from_a_captured_graph():
    K = 32
    sim = make_sim(["albert"], K, BASE_INIT)
    dof, roots, vd = fi.inputs("albert")
    push(sim, dof[:K], roots[:K])
    N = 6 + sim.scene.n_dof
    eager = launch(sim, vd[:K], 3)                                  # (also the warm-up outside the capture)
    vd_t = torch.from_numpy(np.array(vd[:K])).to(sim.device)
    tau = torch.full((K, N), float("nan"), dtype=torch.float32, device=sim.device)
    lib, ctx = sim._lib, sim._ctx
    torch.cuda.synchronize()
    g, main = torch.cuda.CUDAGraph(), torch.cuda.current_stream()
    try:
        with torch.cuda.graph(g):      # one stream, one launch: no parallel branches
            capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            capi.check(lib, lib.mppi_sim_floating_inverse_dynamics(ctx, ptr(vd_t), 3, ptr(tau)))
    finally:
        capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(main.cuda_stream)))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(tau.cpu().numpy()), bits(eager))
    # the states changed by mppi_sim_set_states: the replay gives what a direct call gives there
    push(sim, np.ascontiguousarray(dof[K:2 * K]), np.ascontiguousarray(roots[K:2 * K]))
    tau.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(bits(tau.cpu().numpy()), bits(eager))
    assert np.array_equal(bits(tau.cpu().numpy()), bits(launch(sim, vd[:K], 3)))
    sim.stop_sim()


# ---- 7. the wrapper -----------------------------------------------------------------------------------------------------------------
def test_wrapper_tensors():
    K = 16
    sim = make_sim(fi.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    N = 6 + sim.scene.n_dof
    dof0, roots0 = fc.draw_inputs(sim.scene, 2 * K)
    dof, roots, vd = fi.draw_rates(dof0, roots0, sim.scene.robot_idx)
    push(sim, dof[:K], roots[:K])
    t = sim.acquire_floating_bias_force_tensor("boxer")
    assert tuple(t.shape) == (K, N) and not t.any() and sim.acquire_floating_bias_force_tensor("boxer") is t
    bias = launch(sim, None, 3)
    assert not t.any()                                              # zero until refreshed
    sim.refresh_floating_bias_force_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(bias))
    # it changes on refresh only
    push(sim, np.ascontiguousarray(dof[K:]), np.ascontiguousarray(roots[K:]))
    assert np.array_equal(bits(t.cpu().numpy()), bits(bias))
    bias2 = launch(sim, None, 3)
    assert not np.array_equal(bias2, bias)
    sim.refresh_floating_bias_force_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(bias2))
    # fresh tensors: every combination, one acceleration for all envs or one per env
    assert np.array_equal(bits(sim.floating_inverse_dynamics().cpu().numpy()), bits(bias2))
    assert np.array_equal(bits(sim.floating_inverse_dynamics(vd=torch.from_numpy(np.array(vd[K:]))).cpu().numpy()), bits(launch(sim, vd[K:], 3)))
    assert np.array_equal(bits(sim.floating_inverse_dynamics(vd=vd[K], gravity=False).cpu().numpy()), bits(launch(sim, np.tile(vd[K], (K, 1)), fi.ID_VELOCITY)))
    assert np.array_equal(bits(sim.floating_inverse_dynamics(velocity=False).cpu().numpy()), bits(launch(sim, None, fi.ID_GRAVITY)))
    assert not sim.floating_inverse_dynamics(gravity=False, velocity=False).any()
    with pytest.raises(ValueError, match="expected"):
        sim.floating_inverse_dynamics(vd=np.zeros(N - 1, np.float32))
    # a horizon view refuses all of them, with wording of their own
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (lambda: sim.acquire_floating_bias_force_tensor("boxer"), sim.refresh_floating_bias_force_tensors, sim.floating_inverse_dynamics):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "moving-base inverse dynamics" in str(e.value)
    with pytest.raises(ValueError):
        sim.acquire_floating_bias_force_tensor("no_such_actor")
    sim.stop_sim()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    lib = panda._lib
    entry = lib.mppi_sim_floating_inverse_dynamics
    out = torch.full((K * 32,), float("nan"), dtype=torch.float32, device=panda.device)
    assert entry(panda._ctx, None, 3, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_floating_inverse_dynamics" in said and "fixed base" in said and "use mppi_sim_inverse_dynamics" in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                             # nothing was launched
    panda.acquire_floating_bias_force_tensor("panda")
    for call in (panda.refresh_floating_bias_force_tensors, panda.floating_inverse_dynamics):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_inverse_dynamics"):
            call()
    panda.stop_sim()
    # the forest of two jackals (conf/mppi/multi-jackal.yaml): a text of its own
    two = make_sim(["jackal_a", "jackal_b"], K, [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    assert int(two._c_model.n_extra_bases) == 1
    assert entry(two._ctx, None, 3, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "several moving bases" in said and "fixed base" not in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    two.stop_sim()
    # a null output, unknown bits; the six fixed-base entries keep refusing boxer with their text
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    n, B = boxer.scene.n_dof, int(boxer._c_model.n_rb)
    ctx = boxer._ctx
    assert entry(ctx, None, 3, None) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    for terms in (4, 7, -1, 1 << 16):
        assert entry(ctx, None, terms, ptr(out)) == capi.MPPI_EINVAL and "unknown bits" in lib.mppi_last_error().decode(), terms
    big = torch.full((K * B * 6 * (6 + n),), float("nan"), dtype=torch.float32, device=boxer.device)
    wrench = torch.zeros((K * B * 6,), dtype=torch.float32, device=boxer.device)
    for name, call in (("mppi_sim_jacobian", lambda: lib.mppi_sim_jacobian(ctx, 0, B, ptr(big))),
                       ("mppi_sim_mass_matrix", lambda: lib.mppi_sim_mass_matrix(ctx, ptr(big))),
                       ("mppi_sim_inverse_dynamics", lambda: lib.mppi_sim_inverse_dynamics(ctx, None, 3, ptr(big))),
                       ("mppi_sim_forward_dynamics", lambda: lib.mppi_sim_forward_dynamics(ctx, None, 3, ptr(big))),
                       ("mppi_sim_link_acceleration", lambda: lib.mppi_sim_link_acceleration(ctx, 0, B, None, 2, ptr(big))),
                       ("mppi_sim_wrench_forces", lambda: lib.mppi_sim_wrench_forces(ctx, 0, B, ptr(wrench), ptr(big)))):
        assert call() == capi.MPPI_EUNSUPPORTED, name
        said = lib.mppi_last_error().decode()
        assert said.startswith(name + ": unsupported for a robot with a moving base (the six floating-base columns are not computed); fixed-base robots"), said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(big).all())
    # the context is as healthy as before
    capi.check(lib, entry(ctx, None, 3, ptr(out)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got[:K * (6 + n)]).all() and np.isnan(got[K * (6 + n):]).all()
    boxer.stop_sim()
