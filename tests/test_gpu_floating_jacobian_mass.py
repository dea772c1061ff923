"""mppi_sim_floating_jacobian / mppi_sim_floating_mass_matrix (csrc/mppi_kernels.hpp k_sim_floating_jacobian,
k_sim_floating_mass_matrix) and the wrapper's acquire_floating_jacobian_tensor / acquire_floating_mass_matrix_tensor /
refresh_floating_*_tensors / get_actor_link_floating_jacobian_by_name on the GPU, against the fp64 references at the state the
simulator itself holds (its dof and root tensors read back through mppi_sim_materialise and widened): EVERY env, EVERY rigid body,
EVERY entry.  Inputs, references, metrics and tolerances: floating_jacobian_cases.py (its conditions are checked on the oracle alone by
test_floating_jacobian_mass.py); outputs are NaN-filled before every launch with a guard band behind them that must stay NaN, and every
entry must come back finite; the measured maxima are printed next to the tolerances before anything is asserted.

 1 edges of the staged stores: boxer (rows of 48 / 64 floats) at K = 1, 63, 64, 65, 130; jackal_a (4 joints), albert (9), anymal (12:
   the 18 x 18 tile) at K = 65 - every env with joint positions and a base pose of its own, pushed with mppi_sim_set_states; all bodies
   in one call; the properties of M; equality with the host build's figures to the tolerance; J v against the rb tensor
 2 a contact scene with a free actor (boxer + block + obstacle): robot blocks within tolerance, the others exact zeros, sub-ranges
   bit-equal to the slices
 3 live state: after two steps of boxer on the ground the references are taken at the materialised state
 4 with every base translated by (420, -310, 0) J and M come out bit for bit the same
 5 both entries inside ONE captured torch.cuda.graph (one stream, no parallel branches), replayed after the states were changed by
   mppi_sim_set_states: bit-equal to a direct call at the new states
 6 the wrapper: acquired tensors change on refresh only; one link by name; PerStepOnly on a horizon view; NotImplementedError with the
   library's text for the Panda
 7 refusals before any launch, the output still all NaN: a fixed-base Panda, the forest of two jackals, a null pointer, a range past
   n_rb; the six fixed-base entries keep refusing boxer
(No on-demand moving-base tree is built here - its scene unit takes tens of seconds; test_floating_jacobian_mass.py shows that the
plugin units fill the two pointers through the same function.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import floating_jacobian_cases as fc
import jacobian_cases as jc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BASE_INIT = [[0.0, 0.0, 0.3]]
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch_J(sim, first=0, count=None):
    """one raw call into a NaN-filled output with a guard band of one env behind it -> J [K][count][6][6 + n] (numpy)"""
    K, n = sim.num_envs, sim.scene.n_dof
    count = int(sim._c_model.n_rb) - first if count is None else count
    size = K * count * 6 * (6 + n)
    out = torch.full((size + count * 6 * (6 + n),), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_floating_jacobian(sim._ctx, first, count, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[size:]).all(), "the guard band behind J was written"
    assert np.isfinite(got[:size]).all(), "entries that were never written (or not finite)"
    return got[:size].reshape(K, count, 6, 6 + n)


def launch_M(sim):
    K, n = sim.num_envs, sim.scene.n_dof
    size = K * (6 + n) ** 2
    out = torch.full((size + (6 + n) ** 2,), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_floating_mass_matrix(sim._ctx, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[size:]).all(), "the guard band behind M was written"
    assert np.isfinite(got[:size]).all(), "entries that were never written (or not finite)"
    return got[:size].reshape(K, 6 + n, 6 + n)


def push(sim, dof, roots):
    """the per-env states in through mppi_sim_set_states -> (dof, roots) as the simulator holds them, read back through
    mppi_sim_materialise (the joints and the base orientations exactly the inputs)"""
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    sim.set_actor_root_state_tensor(torch.from_numpy(np.array(roots, np.float32)))
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.array_equal(held_dof, dof) and np.array_equal(held_roots[:, a, 3:13], roots[:, a, 3:13])
    assert np.abs(held_roots[:, a, 0:3] - roots[:, a, 0:3]).max() <= 1e-6       # (x, y pass through the scene's relative coordinates)
    return held_dof, held_roots


def check_M_properties(M, model, tol_M):
    n = M.shape[1] - 6
    total = float(model.base_mass) + sum(float(model.bodies[i].mass) for i in range(n))
    assert np.array_equal(bits(M), bits(M.transpose(0, 2, 1)))     # symmetric bit for bit
    for k in range(len(M)):
        np.linalg.cholesky(M[k].astype(np.float64))
    assert np.abs(M[:, 0:3, 0:3].astype(np.float64) - total * np.eye(3)).max() <= tol_M * total


def check(tag, J, M, r, tols):
    eJ, eM = fc.e_J(J, r.J), fc.e_M(M, r.M)
    print(f"\n[{tag}] K {len(J)}: e_J {eJ:.2e} (tol {tols[0]:.0e}), e_M {eM:.2e} (tol {tols[1]:.0e})")
    assert eJ <= tols[0], f"{tag}: e_J {eJ:.3e} > {tols[0]:.0e}"
    assert eM <= tols[1], f"{tag}: e_M {eM:.3e} > {tols[1]:.0e}"
    check_M_properties(M, r.model, tols[1])
    return eJ, eM


def body_ranges(B):
    return [(0, 1), (B - 1, 1), (B // 3, max(B // 2, 1))]


@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_jacobian")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_jacobian_hostemu.so"))


def host_results(lib, model, roots, q):
    K, n = q.shape
    B = int(model.n_rb)
    roots32, q32 = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(q, np.float32)
    J, M = np.full((K, B, 6, 6 + n), np.nan, np.float32), np.full((K, 6 + n, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_jacobian(C.byref(model), K, fp(roots32), fp(q32), 0, B, fp(J)) == 0
    assert lib.emu_floating_mass_matrix(C.byref(model), K, fp(roots32), fp(q32), fp(M)) == 0
    return J, M


# ---- 1. edges of the staged stores --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", fc.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in fc.STORE_EDGES])
def test_store_edges(robot, K, hostemu):
    actors, actor_name, _ = fc.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots = fc.inputs(robot)
    held_dof, held_roots = push(sim, dof[:K], roots[:K])
    r = fc.references_at(sim.scene, sim._c_model, held_roots, held_dof[:, 0::2])       # at what the simulator holds
    tols = fc.tolerances(robot)
    assert r.w32[0] <= 0.1 * tols[0] and r.w32[1] <= 0.1 * tols[1]
    J, M = launch_J(sim), launch_M(sim)
    check(f"edges {robot}", J, M, r, tols)
    # the host build's figures, to the tolerance
    Jh, Mh = host_results(hostemu, sim._c_model, held_roots, held_dof[:, 0::2])
    eJ, eM = fc.e_J(J, Jh.astype(np.float64)), fc.e_M(M, Mh.astype(np.float64))
    print(f"[edges {robot}] against the host build: e_J {eJ:.2e}, e_M {eM:.2e}")
    assert eJ <= tols[0] and eM <= tols[1]
    # J v against the rb tensor of mppi_sim_materialise: non-zero base twist and joint rates
    vl, va = jc.velocity_tolerances(True)
    v = fc.generalised_velocity(held_dof, held_roots, sim.scene.robot_idx)
    rb = sim._rigid_body_state.cpu().numpy().astype(np.float64)
    gap = np.abs(np.einsum("kbrc,kc->kbr", J.astype(np.float64), v) - rb[:, :, 7:13])
    l1 = np.abs(v).sum(1)[:, None, None]
    assert np.abs(v).min(0).max() > 0.0 and np.abs(rb[:, r.robot_rb, 7:13]).max() > 0.05
    print(f"[edges {robot}] J v against the rb rows: {gap[:, :, 0:3].max():.2e} linear, {gap[:, :, 3:6].max():.2e} angular")
    assert (gap[:, :, 0:3] <= tols[0] * l1 + vl).all() and (gap[:, :, 3:6] <= tols[0] * l1 + va).all()
    sim.stop_sim()


# ---- 2. a contact scene with a free actor -------------------------------------------------------------------------------------------
def test_contact_scene_with_a_free_actor():
    K = 65
    sim = make_sim(fc.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    dof, roots = fc.draw_inputs(sim.scene, K)
    held_dof, held_roots = push(sim, dof, roots)
    r = fc.references_at(sim.scene, sim._c_model, held_roots, held_dof[:, 0::2])
    tols = fc.tolerances("boxer")
    assert r.w32[0] <= 0.1 * tols[0] and r.w32[1] <= 0.1 * tols[1]              # boxer's tolerances fit the scene's inputs
    J, M = launch_J(sim), launch_M(sim)
    check("boxer + block + obstacle", J, M, r, tols)
    assert (~r.robot_rb).sum() == 2 and not bits(J[:, ~r.robot_rb]).any()       # the block's and the obstacle's bodies: exact zeros
    B = int(sim._c_model.n_rb)
    for first, count in body_ranges(B) + [(int(b), 1) for b in np.flatnonzero(~r.robot_rb)]:
        assert np.array_equal(bits(launch_J(sim, first, count)), bits(J[:, first:first + count])), (first, count)
    sim.stop_sim()


# ---- 3. live state ------------------------------------------------------------------------------------------------------------------
def test_live_state_after_two_steps():
    K = 65
    sim = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    u = torch.from_numpy(np.random.default_rng(fc.SEED).uniform(-1.0, 1.0, size=(K, sim.scene.nu)).astype(np.float32)).to(sim.device)
    start = sim._root_state.cpu().numpy()
    for _ in range(2):
        sim.apply_robot_cmd(u)
        sim.step()
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.abs(held_roots[:, a, 3:7] - start[:, a, 3:7]).max() > 1e-3      # the bases have turned, each env by its own command
    r = fc.references_at(sim.scene, sim._c_model, held_roots, held_dof[:, 0::2])
    tols = fc.tolerances("boxer")
    J = launch_J(sim)
    check("boxer after two steps", J, launch_M(sim), r, tols)
    # the kernels read the live per-env base, not x0: the references at the start state are off by hundreds of tolerances
    x0 = fc.references_at(sim.scene, sim._c_model, start, np.zeros_like(held_dof[:, 0::2]))
    off = fc.e_J(J, x0.J)
    print(f"[boxer after two steps] the start state's references are off by {off:.1e} in J")
    assert off > 100.0 * tols[0]
    sim.stop_sim()


# ---- 4. translation independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_results_do_not_depend_on_where_the_base_stands(robot):
    K = 65
    actors, _, _ = fc.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots = fc.inputs(robot)
    push(sim, dof[:K], roots[:K])
    J, M = launch_J(sim), launch_M(sim)
    far = np.array(roots[:K])
    far[:, sim.scene.robot_idx, 0:3] += np.asarray(fc.FAR_SHIFT, np.float32)
    sim.set_actor_root_state_tensor(torch.from_numpy(far))
    held = sim._root_state.cpu().numpy()[:, sim.scene.robot_idx]
    assert np.abs(held[:, 0] - far[:, sim.scene.robot_idx, 0]).max() <= 1e-4 and held[:, 0].min() > 400.0 and np.array_equal(held[:, 3:7], far[:, sim.scene.robot_idx, 3:7])
    assert np.array_equal(bits(launch_J(sim)), bits(J)) and np.array_equal(bits(launch_M(sim)), bits(M))
    sim.stop_sim()


# ---- 5. inside a captured graph -----------------------------------------------------------------------------------------------------
def test_both_entries_replay_from_a_captured_graph():
    K = 32
    sim = make_sim(["albert"], K, BASE_INIT)
    dof, roots = fc.inputs("albert")
    push(sim, dof[:K], roots[:K])
    B, n = int(sim._c_model.n_rb), sim.scene.n_dof
    eager_J, eager_M = launch_J(sim), launch_M(sim)               # (also the warm-up outside the capture)
    J = torch.full((K, B, 6, 6 + n), float("nan"), dtype=torch.float32, device=sim.device)
    M = torch.full((K, 6 + n, 6 + n), float("nan"), dtype=torch.float32, device=sim.device)
    lib, ctx = sim._lib, sim._ctx
    torch.cuda.synchronize()
    g, main = torch.cuda.CUDAGraph(), torch.cuda.current_stream()
    try:
        with torch.cuda.graph(g):      # one stream, the two launches one after the other: no parallel branches
            capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            capi.check(lib, lib.mppi_sim_floating_jacobian(ctx, 0, B, ptr(J)))
            capi.check(lib, lib.mppi_sim_floating_mass_matrix(ctx, ptr(M)))
    finally:
        capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(main.cuda_stream)))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(J.cpu().numpy()), bits(eager_J)) and np.array_equal(bits(M.cpu().numpy()), bits(eager_M))
    # the states changed by mppi_sim_set_states: the replay gives what a direct call gives there
    push(sim, np.ascontiguousarray(dof[K:2 * K]), np.ascontiguousarray(roots[K:2 * K]))
    J.fill_(float("nan"))
    M.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(bits(J.cpu().numpy()), bits(eager_J))
    assert np.array_equal(bits(J.cpu().numpy()), bits(launch_J(sim))) and np.array_equal(bits(M.cpu().numpy()), bits(launch_M(sim)))
    sim.stop_sim()


# ---- 6. the wrapper -----------------------------------------------------------------------------------------------------------------
def test_wrapper_acquire_and_refresh():
    K = 16
    sim = make_sim(fc.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    n = sim.scene.n_dof
    first, L = sim._actor_rb_range("boxer")
    Jt, Mt = sim.acquire_floating_jacobian_tensor("boxer"), sim.acquire_floating_mass_matrix_tensor("boxer")
    Jb = sim.acquire_floating_jacobian_tensor("block")
    assert tuple(Jt.shape) == (K, L, 6, 6 + n) and tuple(Mt.shape) == (K, 6 + n, 6 + n) and tuple(Jb.shape) == (K, 1, 6, 6 + n)
    assert not Jt.any() and not Mt.any()                           # zero until refreshed
    assert sim.acquire_floating_jacobian_tensor("boxer") is Jt and sim.acquire_floating_mass_matrix_tensor("boxer") is Mt
    J, M = launch_J(sim), launch_M(sim)
    assert not Jt.any() and not Mt.any()
    sim.refresh_floating_jacobian_tensors()
    sim.refresh_floating_mass_matrix_tensors()
    assert np.array_equal(bits(Jt.cpu().numpy()), bits(J[:, first:first + L])) and np.array_equal(bits(Mt.cpu().numpy()), bits(M))
    assert not Jb.any()                                            # the block: a zero block, refreshed
    # they change on refresh only
    dof, roots = fc.draw_inputs(sim.scene, K)
    a = sim.scene.robot_idx
    now = sim._root_state.cpu().numpy()
    now[:, a] = roots[:, a]
    sim.set_dof_state_tensor(torch.from_numpy(dof))
    sim.set_actor_root_state_tensor(torch.from_numpy(now))
    assert np.array_equal(bits(Jt.cpu().numpy()), bits(J[:, first:first + L])) and np.array_equal(bits(Mt.cpu().numpy()), bits(M))
    J2, M2 = launch_J(sim), launch_M(sim)
    assert not np.array_equal(J2, J) and not np.array_equal(M2, M)
    sim.refresh_floating_jacobian_tensors()
    assert np.array_equal(bits(Jt.cpu().numpy()), bits(J2[:, first:first + L])) and np.array_equal(bits(Mt.cpu().numpy()), bits(M))
    sim.refresh_floating_mass_matrix_tensors()
    assert np.array_equal(bits(Mt.cpu().numpy()), bits(M2))
    # one link by name
    last = sim.scene.robot_model["links"][-1]["name"]
    rb = sim.scene.rigid_body_index("boxer", last)
    one = sim.get_actor_link_floating_jacobian_by_name("boxer", last)
    assert tuple(one.shape) == (K, 6, 6 + n) and np.array_equal(bits(one.cpu().numpy()), bits(J2[:, rb]))
    # a horizon view refuses all of them, with wording of their own
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (lambda: sim.acquire_floating_jacobian_tensor("boxer"), lambda: sim.acquire_floating_mass_matrix_tensor("boxer"),
                     sim.refresh_floating_jacobian_tensors, sim.refresh_floating_mass_matrix_tensors,
                     lambda: sim.get_actor_link_floating_jacobian_by_name("boxer", last)):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "moving-base link Jacobians" in str(e.value)
    with pytest.raises(ValueError):
        sim.acquire_floating_jacobian_tensor("no_such_actor")
    sim.stop_sim()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    lib = panda._lib
    n, B = panda.scene.n_dof, int(panda._c_model.n_rb)
    out = torch.full((K * B * 6 * (6 + n),), float("nan"), dtype=torch.float32, device=panda.device)
    assert lib.mppi_sim_floating_jacobian(panda._ctx, 0, B, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_floating_jacobian" in said and "fixed base" in said and "use mppi_sim_jacobian" in said
    assert lib.mppi_sim_floating_mass_matrix(panda._ctx, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_floating_mass_matrix" in said and "fixed base" in said and "use mppi_sim_mass_matrix" in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())                            # nothing was launched
    panda.acquire_floating_jacobian_tensor("panda")
    panda.acquire_floating_mass_matrix_tensor("panda")
    for call in (panda.refresh_floating_jacobian_tensors, panda.refresh_floating_mass_matrix_tensors,
                 lambda: panda.get_actor_link_floating_jacobian_by_name("panda", "panda_link7")):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_"):
            call()
    panda.stop_sim()
    # the forest of two jackals (conf/mppi/multi-jackal.yaml): a text of its own
    two = make_sim(["jackal_a", "jackal_b"], K, [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    assert int(two._c_model.n_extra_bases) == 1
    n, B = two.scene.n_dof, int(two._c_model.n_rb)
    out = torch.full((K * B * 6 * (6 + n),), float("nan"), dtype=torch.float32, device=two.device)
    for rc in (lib.mppi_sim_floating_jacobian(two._ctx, 0, B, ptr(out)), lib.mppi_sim_floating_mass_matrix(two._ctx, ptr(out))):
        assert rc == capi.MPPI_EUNSUPPORTED
        said = lib.mppi_last_error().decode()
        assert "several moving bases" in said and "fixed base" not in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    two.stop_sim()
    # a null pointer, a range past n_rb; the fixed-base entries keep refusing boxer with their text
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    n, B = boxer.scene.n_dof, int(boxer._c_model.n_rb)
    ctx = boxer._ctx
    out = torch.full((K * B * 6 * (6 + n),), float("nan"), dtype=torch.float32, device=boxer.device)
    assert lib.mppi_sim_floating_jacobian(ctx, 0, B, None) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    assert lib.mppi_sim_floating_mass_matrix(ctx, None) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    for first, count in ((0, B + 1), (B, 1), (B - 1, 2), (-1, 1), (0, 0), (1, (1 << 31) - 1)):
        assert lib.mppi_sim_floating_jacobian(ctx, first, count, ptr(out)) == capi.MPPI_EINVAL, (first, count)
        assert "outside [0, " in lib.mppi_last_error().decode()
    assert lib.mppi_sim_jacobian(ctx, 0, B, ptr(out)) == capi.MPPI_EUNSUPPORTED and "the six floating-base columns are not computed" in lib.mppi_last_error().decode()
    assert lib.mppi_sim_mass_matrix(ctx, ptr(out)) == capi.MPPI_EUNSUPPORTED and "the six floating-base columns are not computed" in lib.mppi_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # the context is as healthy as before
    capi.check(lib, lib.mppi_sim_floating_jacobian(ctx, 0, B, ptr(out)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    boxer.stop_sim()
