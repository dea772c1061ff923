"""mppi_sim_floating_forward_dynamics (csrc/mppi_kernels.hpp k_sim_floating_forward_dynamics) and the wrapper's
floating_forward_dynamics / acquire_floating_free_acceleration_tensor / refresh_floating_free_acceleration_tensors /
floating_inverse_mass_matrix on the GPU, against the fp64 reference at the state the simulator itself holds (its dof and root tensors
read back through mppi_sim_materialise and widened): EVERY env, EVERY row, EVERY call.  Inputs, reference, metrics and tolerances:
floating_forward_dynamics_cases.py (its conditions are checked on the oracle alone by test_floating_forward_dynamics.py); outputs are
NaN-filled before every launch with a guard band of one env behind them that must stay NaN, and every entry must come back finite; the
measured maxima are printed next to the tolerances before anything is asserted.

 1 edges of the staged load and store: boxer (rows of 8 floats) at K = 1, 63, 64, 65, 130; jackal_a (10), albert (15), anymal (18) at
   K = 65 - every env with joint positions, rates, a base pose and a base twist of its own, pushed with mppi_sim_set_states; the eight
   combinations of terms and tau; terms = 0 without tau gives exact zeros, gravity alone free fall; the host build's figures to the
   tolerance
 2 a contact scene with a free and a static actor (boxer + block + obstacle)
 3 live state: after two steps of boxer on the ground the references are taken at the materialised state; the start state's
   references are far off
 4 device against device: mppi_sim_floating_inverse_dynamics of the result returns tau; the columns of M^-1 (terms = 0 on tau = e_c)
   times mppi_sim_floating_mass_matrix give the identity in the column metric; free fall
 5 with every base translated by (420, -310, 0) vd comes out bit for bit the same
 6 the launch inside a captured torch.cuda.graph (one stream), replayed after the states were changed by mppi_sim_set_states:
   bit-equal to a direct call at the new states
 7 the wrapper: the acquired tensor changes on refresh only; floating_inverse_mass_matrix is symmetric bit for bit and meets the
   reference; PerStepOnly on a horizon view; NotImplementedError with the library's text for the Panda
 8 refusals before any launch, the output still all NaN: a fixed-base Panda, the forest of two jackals, a null output, unknown bits;
   mppi_sim_forward_dynamics keeps refusing boxer with its text; the context is healthy afterwards
(No on-demand moving-base tree is built here - its scene unit takes tens of seconds; test_floating_forward_dynamics.py shows that the
plugin units fill the pointer through the same function.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import floating_forward_dynamics_cases as ff
import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BASE_INIT = [[0.0, 0.0, 0.3]]
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
call_name = lambda c: f"{c[0]}{'+tau' if c[1] else ''}"


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(sim, tau, terms, entry="mppi_sim_floating_forward_dynamics"):
    """one raw call into a NaN-filled output with a guard band of one env behind it -> [K][6 + n] (numpy).  tau: numpy [K][6 + n] or None"""
    K, N = sim.num_envs, 6 + sim.scene.n_dof
    out = torch.full(((K + 1) * N,), float("nan"), dtype=torch.float32, device=sim.device)
    tau_t = torch.from_numpy(np.array(tau, np.float32)).to(sim.device) if tau is not None else None
    capi.check(sim._lib, getattr(sim._lib, entry)(sim._ctx, ptr(tau_t), terms, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * N:]).all(), "the guard band behind the output was written"
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


def check_calls(tag, sim, r, tau, tols, calls=ff.ALL_CALLS):
    """every call shape against the reference's -> {call: vd}"""
    got = {c: launch(sim, tau if c[1] else None, c[0]) for c in calls}
    worst = ff.measure(got, r)
    print(f"\n[{tag}] K {sim.num_envs}: e_vd / e_res per call (terms, tau given): " + ", ".join(f"{call_name(c)} {e[0]:.1e} / {e[1]:.1e}" for c, e in worst.items())
          + f"; tol {tols[0]:.0e} / {tols[1]:.0e}, fp32 restatement {r.w32[0]:.1e} / {r.w32[1]:.1e}, Richardson gap {r.gap:.1e}")
    assert r.gap <= fi.RICHARDSON_AGREE
    for call, e in worst.items():
        assert e[0] <= tols[0] and e[1] <= tols[1], f"{tag} {call}: e_vd {e[0]:.3e} (tol {tols[0]:.0e}), e_res {e[1]:.3e} (tol {tols[1]:.0e})"
    return got


def free_fall(sim):
    g = np.array([sim._c_model.gravity[j] for j in range(3)], np.float32)
    return np.tile(np.concatenate([g, np.zeros(3 + sim.scene.n_dof, np.float32)]), (sim.num_envs, 1))


@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_forward_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_forward_dynamics_hostemu.so"))


# ---- 1. edges of the staged load and store ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", ff.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in ff.STORE_EDGES])
def test_store_edges(robot, K, hostemu):
    actors, _, _ = ff.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, tau = ff.inputs(robot)
    held_dof, held_roots = push(sim, dof[:K], roots[:K])
    r = ff.references_at(sim.scene, sim._c_model, held_roots, held_dof, tau[:K])       # at what the simulator holds
    tols = ff.tolerances(robot)
    got = check_calls(f"edges {robot}", sim, r, tau[:K], tols)
    assert not got[0, False].any()                                  # nothing asked for: exact zeros
    assert np.array_equal(got[ff.ID_GRAVITY, False], free_fall(sim))
    # the host build's figures, to the tolerance
    n = sim.scene.n_dof
    host = np.full((K, 6 + n), np.nan, np.float32)
    q, qd = np.ascontiguousarray(held_dof[:, 0::2]), np.ascontiguousarray(held_dof[:, 1::2])
    assert hostemu.emu_floating_forward_dynamics(C.byref(sim._c_model), K, fp(np.ascontiguousarray(held_roots)), fp(q), fp(qd),
                                                 fp(np.ascontiguousarray(tau[:K])), 3, fp(host)) == 0
    e = ff.e_vd(got[ff.FULL], host.astype(np.float64), r.D), ff.e_res(got[ff.FULL], host.astype(np.float64), r.M, r.Dtau)
    print(f"[edges {robot}] against the host build: e_vd {e[0]:.2e}, e_res {e[1]:.2e}")
    assert e[0] <= tols[0] and e[1] <= tols[1]
    sim.stop_sim()


# ---- 2. a contact scene with a free and a static actor ------------------------------------------------------------------------------
def test_contact_scene_with_a_free_and_a_static_actor():
    K = 65
    sim = make_sim(ff.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    dof0, roots0 = fc.draw_inputs(sim.scene, K)
    dof, roots, vd = fi.draw_rates(dof0, roots0, sim.scene.robot_idx)
    held_dof, held_roots = push(sim, dof, roots)
    tau = ff.tau_for(sim.scene, sim._c_model, held_roots, held_dof, vd)
    r = ff.references_at(sim.scene, sim._c_model, held_roots, held_dof, tau)
    tols = ff.tolerances("boxer")
    assert ff.tolerances_from(r.w32) == tols                        # boxer's tolerances fit the scene's inputs
    assert int(sim._c_model.n_actors) == 3 and int(sim._c_model.n_rb) == int(sim._c_model.actors[sim.scene.robot_idx].n_rb) + 2
    check_calls("boxer + block + obstacle", sim, r, tau, tols, ff.CALLS)
    sim.stop_sim()


# ---- 3. live state ------------------------------------------------------------------------------------------------------------------
def test_live_state_after_two_steps():
    K = 65
    sim = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    u = torch.from_numpy(np.random.default_rng(ff.SEED).uniform(-1.0, 1.0, size=(K, sim.scene.nu)).astype(np.float32)).to(sim.device)
    start_dof, start = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    for _ in range(2):
        sim.apply_robot_cmd(u)
        sim.step()
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.abs(held_roots[:, a, 3:7] - start[:, a, 3:7]).max() > 1e-3 and np.abs(held_roots[:, a, 7:13]).max() > 1e-2     # turned and moving
    tau = ff.inputs("boxer")[2][:K]
    r = ff.references_at(sim.scene, sim._c_model, held_roots, held_dof, tau)
    tols = ff.tolerances("boxer")
    got = check_calls("boxer after two steps", sim, r, tau, tols, ff.CALLS)
    # the kernel reads the live per-env base and rates, not x0: the references at the start state are off by hundreds of tolerances
    x0 = ff.references_at(sim.scene, sim._c_model, start, start_dof, tau)
    off = ff.e_vd(got[ff.FULL], x0.ref[ff.FULL], r.D)
    print(f"[boxer after two steps] the start state's references are off by {off:.1e}")
    assert off > 100.0 * tols[0]
    sim.stop_sim()


# ---- 4. device against device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_round_trip_inverse_mass_matrix_and_free_fall_on_the_device(robot):
    K = 65
    actors, _, _ = ff.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, tau = ff.inputs(robot)
    push(sim, dof[:K], roots[:K])
    N = 6 + sim.scene.n_dof
    r = ff.references(robot)
    # the round trip through the device's inverse dynamics: within the sum of the two routines' (b)-tolerances
    vd = launch(sim, tau[:K], 3)
    back = launch(sim, vd, 3, entry="mppi_sim_floating_inverse_dynamics")
    e = float((np.abs(back.astype(np.float64) - tau[:K]) / r.Dtau[None, :]).max())
    bound = ff.tolerances(robot)[1] + fi.tolerance(robot)
    print(f"\n[{robot}] mppi_sim_floating_inverse_dynamics of the result against tau: {e:.2e} of Dtau (bound {bound:.1e})")
    assert e <= bound
    # the columns of M^-1 times the device's M against the identity.  Reported in the column metric, (X M - 1)_jc / sqrt(X_jj / X_cc):
    # X M is dimensionless only up to the units of rows j and c, and sqrt(X_jj), 1 / sqrt(X_cc) carry exactly those.  Bounded entry by
    # entry from the two tolerances: X meets X_ref within tol_X sqrt(X_jj X_ii) and M its reference within tol_M sqrt(M_ii M_cc), so
    # |X M - 1|_jc <= sum_i tol_X sx_j sx_i |M_ic| + |X_ji| tol_M sm_i sm_c + tol_X tol_M sx_j sx_i sm_i sm_c
    M = torch.full((K, N, N), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_floating_mass_matrix(sim._ctx, ptr(M)))
    M = M.cpu().numpy().astype(np.float64)
    X = np.stack([launch(sim, np.tile(np.eye(N, dtype=np.float32)[c], (K, 1)), 0) for c in range(N)], axis=2).astype(np.float64)
    X_ref, tol_X, w32 = ff.Minv_reference(robot)
    X_ref, M_ref = X_ref[:K], r.M[:K]
    eX = ff.e_X(X, X_ref)
    sx, sm = np.sqrt(np.einsum("kii->ki", X_ref)), np.sqrt(np.einsum("kii->ki", M_ref))
    prod = np.einsum("kji,kic->kjc", X, M) - np.eye(N)[None]
    eI = float((np.abs(prod) / (sx[:, :, None] / sx[:, None, :])).max())
    tol_M = fc.tolerances(robot)[1]
    bound = (tol_X * sx[:, :, None] * np.einsum("ki,kic->kc", sx, np.abs(M_ref))[:, None, :]
             + tol_M * np.einsum("kji,ki->kj", np.abs(X_ref), sm)[:, :, None] * sm[:, None, :]
             + tol_X * tol_M * np.einsum("ki,ki->k", sx, sm)[:, None, None] * sx[:, :, None] * sm[:, None, :])
    of_bound = float((np.abs(prod) / bound).max())
    print(f"[{robot}] columns of M^-1 against the reference: e_X {eX:.2e} (tol {tol_X:.0e}, fp32 dense inverse {w32:.1e}); "
          f"times mppi_sim_floating_mass_matrix against the identity: {eI:.2e} in the column metric, {of_bound:.2e} of the entry's bound")
    assert eX <= tol_X and of_bound <= 1.0
    assert np.array_equal(launch(sim, None, ff.ID_GRAVITY), free_fall(sim))
    sim.stop_sim()


# ---- 5. translation independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_result_does_not_depend_on_where_the_base_stands(robot):
    K = 65
    actors, _, _ = ff.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, tau = ff.inputs(robot)
    push(sim, dof[:K], roots[:K])
    vd = launch(sim, tau[:K], 3)
    far = np.array(roots[:K])
    a = sim.scene.robot_idx
    far[:, a, 0:3] += np.asarray(ff.FAR_SHIFT, np.float32)
    sim.set_actor_root_state_tensor(torch.from_numpy(far))
    held = sim._root_state.cpu().numpy()[:, a]
    assert np.abs(held[:, 0] - far[:, a, 0]).max() <= 1e-4 and held[:, 0].min() > 400.0 and np.array_equal(held[:, 3:13], far[:, a, 3:13])
    assert np.array_equal(bits(launch(sim, tau[:K], 3)), bits(vd))
    sim.stop_sim()


# ---- 6. inside a captured graph -----------------------------------------------------------------------------------------------------
def test_the_entry_replays_from_a_captured_graph():
    K = 32
    sim = make_sim(["albert"], K, BASE_INIT)
    dof, roots, tau = ff.inputs("albert")
    push(sim, dof[:K], roots[:K])
    N = 6 + sim.scene.n_dof
    eager = launch(sim, tau[:K], 3)                                 # (also the warm-up outside the capture)
    tau_t = torch.from_numpy(np.array(tau[:K])).to(sim.device)
    vd = torch.full((K, N), float("nan"), dtype=torch.float32, device=sim.device)
    lib, ctx = sim._lib, sim._ctx
    torch.cuda.synchronize()
    g, main = torch.cuda.CUDAGraph(), torch.cuda.current_stream()
    try:
        with torch.cuda.graph(g):      # one stream, one launch: no parallel branches
            capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            capi.check(lib, lib.mppi_sim_floating_forward_dynamics(ctx, ptr(tau_t), 3, ptr(vd)))
    finally:
        capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(main.cuda_stream)))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(vd.cpu().numpy()), bits(eager))
    # the states changed by mppi_sim_set_states: the replay gives what a direct call gives there
    push(sim, np.ascontiguousarray(dof[K:2 * K]), np.ascontiguousarray(roots[K:2 * K]))
    vd.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(bits(vd.cpu().numpy()), bits(eager))
    assert np.array_equal(bits(vd.cpu().numpy()), bits(launch(sim, tau[:K], 3)))
    sim.stop_sim()


# ---- 7. the wrapper -----------------------------------------------------------------------------------------------------------------
def test_wrapper_tensors():
    K = 16
    sim = make_sim(["boxer"], K, BASE_INIT)
    N = 6 + sim.scene.n_dof
    dof, roots, tau = ff.inputs("boxer")
    push(sim, dof[:K], roots[:K])
    t = sim.acquire_floating_free_acceleration_tensor("boxer")
    assert tuple(t.shape) == (K, N) and not t.any() and sim.acquire_floating_free_acceleration_tensor("boxer") is t
    free = launch(sim, None, 3)
    assert not t.any()                                              # zero until refreshed
    sim.refresh_floating_free_acceleration_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(free))
    # M^-1: symmetric bit for bit, the reference's within the column tolerance
    X = sim.floating_inverse_mass_matrix().cpu().numpy()
    X_ref, tol_X, _ = ff.Minv_reference("boxer")
    eX = ff.e_X(X, X_ref[:K])
    print(f"\n[wrapper] floating_inverse_mass_matrix: e_X {eX:.2e} (tol {tol_X:.0e})")
    assert tuple(X.shape) == (K, N, N) and np.array_equal(bits(X), bits(X.transpose(0, 2, 1))) and eX <= tol_X
    # it changes on refresh only
    push(sim, np.ascontiguousarray(dof[K:2 * K]), np.ascontiguousarray(roots[K:2 * K]))
    assert np.array_equal(bits(t.cpu().numpy()), bits(free))
    free2 = launch(sim, None, 3)
    assert not np.array_equal(free2, free)
    sim.refresh_floating_free_acceleration_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(free2))
    # fresh tensors: every combination, one force for all envs or one per env
    assert np.array_equal(bits(sim.floating_forward_dynamics().cpu().numpy()), bits(free2))
    assert np.array_equal(bits(sim.floating_forward_dynamics(tau=torch.from_numpy(np.array(tau[K:2 * K]))).cpu().numpy()), bits(launch(sim, tau[K:2 * K], 3)))
    assert np.array_equal(bits(sim.floating_forward_dynamics(tau=np.array(tau[K]), gravity=False).cpu().numpy()), bits(launch(sim, np.tile(tau[K], (K, 1)), ff.ID_VELOCITY)))
    assert np.array_equal(sim.floating_forward_dynamics(velocity=False).cpu().numpy(), free_fall(sim))
    assert not sim.floating_forward_dynamics(gravity=False, velocity=False).any()
    with pytest.raises(ValueError, match="expected"):
        sim.floating_forward_dynamics(tau=np.zeros(N - 1, np.float32))
    # a horizon view refuses all of them, with wording of their own
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (lambda: sim.acquire_floating_free_acceleration_tensor("boxer"), sim.refresh_floating_free_acceleration_tensors,
                     sim.floating_forward_dynamics, sim.floating_inverse_mass_matrix):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "moving-base forward dynamics" in str(e.value)
    with pytest.raises(ValueError):
        sim.acquire_floating_free_acceleration_tensor("no_such_actor")
    sim.stop_sim()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    lib = panda._lib
    entry = lib.mppi_sim_floating_forward_dynamics
    out = torch.full((K * 32,), float("nan"), dtype=torch.float32, device=panda.device)
    assert entry(panda._ctx, None, 3, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_floating_forward_dynamics" in said and "fixed base" in said and "use mppi_sim_forward_dynamics" in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                             # nothing was launched
    panda.acquire_floating_free_acceleration_tensor("panda")
    for call in (panda.refresh_floating_free_acceleration_tensors, panda.floating_forward_dynamics, panda.floating_inverse_mass_matrix):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_forward_dynamics"):
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
    # a null output, unknown bits; the fixed-base entry keeps refusing boxer with its text
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    n = boxer.scene.n_dof
    ctx = boxer._ctx
    assert entry(ctx, None, 3, None) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    for terms in (4, 7, -1, 1 << 16):
        assert entry(ctx, None, terms, ptr(out)) == capi.MPPI_EINVAL and "unknown bits" in lib.mppi_last_error().decode(), terms
    assert lib.mppi_sim_forward_dynamics(ctx, None, 3, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert said.startswith("mppi_sim_forward_dynamics: unsupported for a robot with a moving base (the six floating-base columns are not computed); fixed-base robots"), said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the context is as healthy as before
    capi.check(lib, entry(ctx, None, 3, ptr(out)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got[:K * (6 + n)]).all() and np.isnan(got[K * (6 + n):]).all()
    boxer.stop_sim()
