"""mppi_sim_floating_link_acceleration / mppi_sim_floating_wrench_forces (csrc/mppi_kernels.hpp k_sim_floating_link_acceleration,
k_sim_floating_wrench_forces) and the wrapper's floating_link_accelerations / get_actor_link_floating_acceleration_by_name /
acquire_floating_link_bias_acceleration_tensor / refresh_floating_link_bias_acceleration_tensors / floating_forces_from_wrenches /
floating_forces_from_link_wrench on the GPU, against the fp64 references at the state the simulator itself holds (its dof and root
tensors read back and widened): EVERY env, EVERY rigid body, EVERY entry, the four acceleration calls and the wrench call.  Inputs,
references, metrics and tolerances: floating_link_acceleration_cases.py (its conditions are checked on the oracle alone by
test_floating_link_acceleration.py); outputs are NaN-filled before every launch with a guard band of one env behind them that must
stay NaN, and every entry must come back finite; the measured maxima are printed next to the tolerances before anything is asserted.

 1 edges of the staged loads and stores: boxer at K = 1, 63, 64, 65, 130; jackal_a, albert, anymal at K = 65 - every env with joint
   positions, rates, a base pose and a base twist of its own, pushed with mppi_sim_set_states; terms = 0 without vd gives exact zeros;
   a one-body range and a middle range (rb_first > 0) are the rows of the full call bit for bit (for the wrenches: the full call on
   wrenches that are zero outside the range)
 2 a contact scene with a free and a static actor (boxer + block + obstacle): exact zero acceleration rows for the block and the
   obstacle, their wrench rows filled with NaN reach nothing
 3 device against device: terms = 0 on vd = e_c against mppi_sim_floating_jacobian column by column and unit wrenches against its rows,
   within one tolerance (the recursion sums the lever arms in another order than the Jacobian's walk; exact zeros where the Jacobian is
   zero); J vd + the wrapper's bias tensor against the full call
 4 composition with the dynamics: mppi_sim_floating_forward_dynamics(tau + sum J^T w) minus the call without w equals M^-1 sum J^T w from
   floating_inverse_mass_matrix, within the sum of the forward-dynamics and the wrench tolerance
 5 live state: after two steps of boxer on the ground the references are taken at the materialised state; the start state's are far off
 6 with every base translated by (420, -310, 0) both results come out bit for bit the same
 7 both launches inside a captured torch.cuda.graph (one stream, no parallel branches), replayed after the states were changed by
   mppi_sim_set_states: bit-equal to direct calls at the new states
 8 refusals before any launch, the outputs still all NaN: a fixed-base Panda (text naming the fixed entry to use), the forest of two
   jackals, null pointers, ranges outside [0, n_rb), bits other than MPPI_ID_VELOCITY; the context is healthy afterwards
 9 the wrapper: shapes, the acquired tensor changes on refresh only, PerStepOnly on a horizon view, NotImplementedError for the Panda,
   ValueError texts; the fixed wrapper methods still raise for boxer."""
import ctypes as C

import numpy as np
import pytest
import torch

import floating_forward_dynamics_cases as ff
import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
import floating_link_acceleration_cases as fl
import link_acceleration_cases as lc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
BASE_INIT = [[0.0, 0.0, 0.3]]
call_name = lambda c: f"{c[0]}{'+vd' if c[1] else ''}"


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _guarded(sim, shape):
    """a NaN-filled output of K envs with a guard band of one env behind it"""
    per_env = int(np.prod(shape))
    return torch.full(((sim.num_envs + 1) * per_env,), float("nan"), dtype=torch.float32, device=sim.device), per_env


def _unguard(sim, out, per_env, shape):
    got = out.cpu().numpy()
    K = sim.num_envs
    assert np.isnan(got[K * per_env:]).all(), "the guard band behind the output was written"
    assert np.isfinite(got[:K * per_env]).all(), "entries that were never written (or not finite)"
    return got[:K * per_env].reshape((K,) + tuple(shape))


def launch_acc(sim, vd, terms, rb_first=0, rb_count=None):
    """one raw call -> [K][rb_count][6] (numpy).  vd: numpy [K][6 + n] or None"""
    rb_count = int(sim._c_model.n_rb) - rb_first if rb_count is None else rb_count
    out, per_env = _guarded(sim, (rb_count, 6))
    vd_t = torch.from_numpy(np.array(vd, np.float32)).to(sim.device) if vd is not None else None
    capi.check(sim._lib, sim._lib.mppi_sim_floating_link_acceleration(sim._ctx, rb_first, rb_count, ptr(vd_t), terms, ptr(out)))
    return _unguard(sim, out, per_env, (rb_count, 6))


def launch_tau(sim, w, rb_first=0, rb_count=None):
    """one raw call -> [K][6 + n] (numpy).  w: numpy [K][rb_count][6]"""
    rb_count = int(sim._c_model.n_rb) - rb_first if rb_count is None else rb_count
    N = 6 + sim.scene.n_dof
    out, per_env = _guarded(sim, (N,))
    w = np.array(w, np.float32)                                     # (a writable copy)
    assert w.shape == (sim.num_envs, rb_count, 6)
    w_t = torch.from_numpy(w).to(sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_floating_wrench_forces(sim._ctx, rb_first, rb_count, ptr(w_t), ptr(out)))
    return _unguard(sim, out, per_env, (N,))


def launch_J(sim):
    B, N = int(sim._c_model.n_rb), 6 + sim.scene.n_dof
    out, per_env = _guarded(sim, (B, 6, N))
    capi.check(sim._lib, sim._lib.mppi_sim_floating_jacobian(sim._ctx, 0, B, ptr(out)))
    return _unguard(sim, out, per_env, (B, 6, N))


def launch_fd(sim, tau, terms=3):
    N = 6 + sim.scene.n_dof
    out, per_env = _guarded(sim, (N,))
    tau_t = torch.from_numpy(np.array(tau, np.float32)).to(sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_floating_forward_dynamics(sim._ctx, ptr(tau_t), terms, ptr(out)))
    return _unguard(sim, out, per_env, (N,))


def push(sim, dof, roots):
    """the per-env states in through mppi_sim_set_states -> (dof, roots) as the simulator holds them"""
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    sim.set_actor_root_state_tensor(torch.from_numpy(np.array(roots, np.float32)))
    held_dof, held_roots = sim._dof_state.cpu().numpy(), sim._root_state.cpu().numpy()
    a = sim.scene.robot_idx
    assert np.array_equal(held_dof, dof) and np.array_equal(held_roots[:, a, 3:13], roots[:, a, 3:13])
    assert np.abs(held_roots[:, a, 0:3] - roots[:, a, 0:3]).max() <= 1e-6       # (x, y pass through the scene's relative coordinates)
    return held_dof, held_roots


def check_calls(tag, sim, r, vd, w, tols):
    """the four acceleration calls and the wrench call against the references -> ({call: acc}, tau)"""
    acc = {c: launch_acc(sim, vd if c[1] else None, c[0]) for c in fl.ACC_CALLS}
    tau = launch_tau(sim, w)
    worst, et = fl.measure(acc, tau, r)
    print(f"\n[{tag}] K {sim.num_envs}: e_lin / e_ang per call (terms, vd given): " + ", ".join(f"{call_name(c)} {e[0]:.1e} / {e[1]:.1e}" for c, e in worst.items())
          + f"; e_tau {et:.1e}; tol {tols[0]:.0e} / {tols[1]:.0e} / {tols[2]:.0e}, fp32 restatement {r.w32[0]:.1e} / {r.w32[1]:.1e} / {r.w32[2]:.1e}, "
          f"Richardson gap {r.parts['gap']:.1e}")
    for call, e in worst.items():
        assert e[0] <= tols[0] and e[1] <= tols[1], f"{tag} {call}: e_lin {e[0]:.3e} (tol {tols[0]:.0e}), e_ang {e[1]:.3e} (tol {tols[1]:.0e})"
    assert et <= tols[2], f"{tag}: e_tau {et:.3e} (tol {tols[2]:.0e})"
    assert not acc[0, False].any()                                  # nothing asked for: exact zeros
    for c in fl.ACC_CALLS:                                          # rows the reference has exactly zero are exact zeros
        assert not acc[c][:, r.zero].any()
    return acc, tau


# ---- 1. edges of the staged loads and stores ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", fl.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in fl.STORE_EDGES])
def test_store_edges(robot, K):
    actors, _, _ = fl.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, vd, w = (a[:K] for a in fl.inputs(robot))
    held_dof, held_roots = push(sim, dof, roots)
    whole = fl.references(robot)
    # at what the simulator holds; measured against the scales of the robot's whole input set (these envs are its first K)
    r = fl.references_at(sim.scene, sim._c_model, held_roots, held_dof, vd, w, scales=(whole.D, whole.Dj))
    tols = fl.tolerances(robot)
    assert all(x <= y for x, y in zip(fl.tolerances_from(r.w32), tols))             # (fewer envs: the restatement's worst can only be smaller)
    acc, tau = check_calls(f"edges {robot}", sim, r, vd, w, tols)
    # a one-body range and a middle range: the rows of the full call, bit for bit
    B = int(sim._c_model.n_rb)
    for first, count in ((B - 1, 1), (2, 1), (1, B - 2)):
        assert np.array_equal(bits(launch_acc(sim, vd, fl.ID_VELOCITY, first, count)), bits(acc[fl.FULL][:, first:first + count])), (first, count)
        assert np.array_equal(bits(launch_acc(sim, None, fl.ID_VELOCITY, first, count)), bits(acc[fl.ID_VELOCITY, False][:, first:first + count]))
        only = np.zeros_like(w)
        only[:, first:first + count] = w[:, first:first + count]
        # (zero wrenches add +-0 to the sums: the same values; a sign of zero may differ)
        assert np.array_equal(launch_tau(sim, w[:, first:first + count], first, count), launch_tau(sim, only)), (first, count)
    sim.stop_sim()


# ---- 2. a contact scene with a free and a static actor ------------------------------------------------------------------------------
def test_contact_scene_with_a_free_and_a_static_actor():
    K = 65
    sim = make_sim(fl.PUSH_SCENE, K, [[0.0, 2.5, 0.05]])
    dof0, roots0 = fc.draw_inputs(sim.scene, K)
    dof, roots, vd = fi.draw_rates(dof0, roots0, sim.scene.robot_idx)
    held_dof, held_roots = push(sim, dof, roots)
    w = lc.wrenches(K, int(sim._c_model.n_rb))
    r = fl.references_at(sim.scene, sim._c_model, held_roots, held_dof, vd, w)
    tols = fl.tolerances("boxer")
    assert all(x <= 0.2 * t for x, t in zip(r.w32, tols))           # boxer's tolerances fit the scene's inputs
    assert int(sim._c_model.n_actors) == 3 and int(sim._c_model.n_rb) == int(sim._c_model.actors[sim.scene.robot_idx].n_rb) + 2
    assert r.zero.sum() == 2 and not r.zero[r.first:r.first + r.L].any()
    acc, tau = check_calls("boxer + block + obstacle", sim, r, vd, w, tols)
    for c in fl.ACC_CALLS:
        assert not bits(acc[c][:, r.zero]).any()                    # +0.0 everywhere
    for b in np.flatnonzero(r.zero):
        assert not bits(launch_acc(sim, vd, fl.ID_VELOCITY, int(b), 1)).any()
    poisoned = np.array(w)
    poisoned[:, r.zero] = np.nan
    assert np.array_equal(bits(launch_tau(sim, poisoned)), bits(tau))
    poisoned[:, r.zero] = np.inf
    assert np.array_equal(bits(launch_tau(sim, poisoned)), bits(tau))
    for b in np.flatnonzero(r.zero):                                # such a body alone: exact zeros
        assert not launch_tau(sim, np.full((K, 1, 6), np.nan, np.float32), int(b), 1).any()
    sim.stop_sim()


# ---- 3. device against device -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_unit_rows_unit_wrenches_and_the_bias_tensor_against_the_device_itself(robot):
    K = 65
    actors, name, _ = fl.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, vd, w = (a[:K] for a in fl.inputs(robot))
    push(sim, dof, roots)
    B, N = int(sim._c_model.n_rb), 6 + sim.scene.n_dof
    tols = fl.tolerances(robot)
    J = launch_J(sim).astype(np.float64)
    cols = np.stack([launch_acc(sim, np.tile(np.eye(N, dtype=np.float32)[c], (K, 1)), 0) for c in range(N)], axis=3)
    scale = np.array([max(1.0, np.abs(J[:, :, 0:3]).max())] * 3 + [1.0] * 3)[None, None, :, None]
    e_cols = float((np.abs(cols - J) / scale).max())
    # unit wrenches: one launch per row index, the same unit wrench on ONE body per env (body k mod B of env k), all bodies over the envs
    rows, want = np.zeros((6, K, N)), np.zeros((6, K, N))
    for j in range(6):
        unit = np.zeros((K, B, 6), np.float32)
        unit[np.arange(K), np.arange(K) % B, j] = 1.0
        rows[j] = launch_tau(sim, unit)
        want[j] = J[np.arange(K), np.arange(K) % B, j, :]
    e_rows = float((np.abs(rows - want) / scale[0, 0, 0, 0]).max())
    print(f"\n[{robot}] terms = 0 on vd = e_c against mppi_sim_floating_jacobian: {e_cols:.1e}; unit wrenches against its rows: {e_rows:.1e} "
          f"(of max(1, largest lever arm) = {scale[0, 0, 0, 0]:.2f}); tol {min(tols):.0e}")
    assert e_cols <= min(tols) and e_rows <= min(tols) and K >= B
    assert not cols[J == 0.0].any() and not rows[want == 0.0].any()
    # J vd + the bias tensor against the full call: two roundings of the sum apart, within the tolerances
    bias = sim.acquire_floating_link_bias_acceleration_tensor(name)
    assert not bias.any()
    sim.refresh_floating_link_bias_acceleration_tensors()
    first, L = sim._actor_rb_range(name)
    full, lin_part = launch_acc(sim, vd, fl.ID_VELOCITY), launch_acc(sim, vd, 0)
    assert np.array_equal(bits(bias.cpu().numpy()), bits(launch_acc(sim, None, fl.ID_VELOCITY)[:, first:first + L]))
    r = fl.references(robot)
    e = fl.e_acc(lin_part[:, first:first + L].astype(np.float64) + bias.cpu().numpy().astype(np.float64), full[:, first:first + L].astype(np.float64), r.D)
    via_J = np.einsum("kbri,ki->kbr", J, vd.astype(np.float64))
    eJ = fl.e_acc(via_J, lin_part.astype(np.float64), r.D)
    print(f"[{robot}] J vd (terms = 0) + the bias tensor against the full call: e_lin {e[0]:.1e}, e_ang {e[1]:.1e}; mppi_sim_floating_jacobian times vd against "
          f"the terms = 0 call: {eJ[0]:.1e}, {eJ[1]:.1e}")
    assert e[0] <= tols[0] and e[1] <= tols[1] and eJ[0] <= tols[0] and eJ[1] <= tols[1]
    sim.stop_sim()


# ---- 4. composition with the dynamics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_wrench_forces_compose_with_the_forward_dynamics(robot):
    K = 65
    actors, name, _ = fl.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, tau = (a[:K] for a in ff.inputs(robot))
    w = fl.inputs(robot)[3][:K]
    push(sim, dof, roots)
    Jw = launch_tau(sim, w)
    with_w, without = launch_fd(sim, tau + Jw), launch_fd(sim, tau)
    X = sim.floating_inverse_mass_matrix().cpu().numpy().astype(np.float64)
    want = np.einsum("kji,ki->kj", X, Jw.astype(np.float64))
    D = ff.references(robot).D
    e = float((np.abs(with_w.astype(np.float64) - without - want) / D[None, :]).max())
    bound = ff.tolerances(robot)[0] + fl.tolerances(robot)[2]
    moved = float((np.abs(want) / D[None, :]).max())
    print(f"\n[{robot}] forward dynamics of tau + sum J^T w minus the call without w against M^-1 sum J^T w: {e:.1e} of D_j (bound {bound:.1e}; the wrenches move vd by {moved:.1e})")
    assert e <= bound and moved >= 100.0 * bound
    sim.stop_sim()


# ---- 5. live state ------------------------------------------------------------------------------------------------------------------
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
    _, _, vd, w = (x[:K] for x in fl.inputs("boxer"))
    r = fl.references_at(sim.scene, sim._c_model, held_roots, held_dof, vd, w)
    tols = fl.tolerances("boxer")
    acc, tau = check_calls("boxer after two steps", sim, r, vd, w, tols)
    # the kernels read the live per-env base and rates, not x0: the references at the start state are off by hundreds of tolerances
    x0 = fl.references_at(sim.scene, sim._c_model, start, start_dof, vd, w)
    off = fl.e_acc(acc[fl.FULL], fl.combine(x0.parts, *fl.FULL), r.D), fl.e_tau(tau, x0.tau_ref, r.Dj)
    print(f"[boxer after two steps] the start state's references are off by {off[0][0]:.1e} / {off[0][1]:.1e} / {off[1]:.1e}")
    assert off[0][0] > 100.0 * tols[0] and off[0][1] > 100.0 * tols[1] and off[1] > 100.0 * tols[2]
    sim.stop_sim()


# ---- 6. translation independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["boxer", "anymal"])
def test_results_do_not_depend_on_where_the_base_stands(robot):
    K = 65
    actors, _, _ = fl.ROBOTS[robot]
    sim = make_sim(actors, K, BASE_INIT)
    dof, roots, vd, w = (a[:K] for a in fl.inputs(robot))
    push(sim, dof, roots)
    acc, tau = launch_acc(sim, vd, fl.ID_VELOCITY), launch_tau(sim, w)
    far = np.array(roots)
    a = sim.scene.robot_idx
    far[:, a, 0:3] += np.asarray(fl.FAR_SHIFT, np.float32)
    far[:, a, 7:10] += np.float32(5.0)
    sim.set_actor_root_state_tensor(torch.from_numpy(far))
    held = sim._root_state.cpu().numpy()[:, a]
    assert np.abs(held[:, 0] - far[:, a, 0]).max() <= 1e-4 and held[:, 0].min() > 400.0 and np.array_equal(held[:, 3:13], far[:, a, 3:13])
    assert np.array_equal(bits(launch_acc(sim, vd, fl.ID_VELOCITY)), bits(acc)) and np.array_equal(bits(launch_tau(sim, w)), bits(tau))
    sim.stop_sim()


# ---- 7. inside a captured graph -----------------------------------------------------------------------------------------------------
def test_both_entries_replay_from_a_captured_graph():
    K = 32
    sim = make_sim(["albert"], K, BASE_INIT)
    dof, roots, vd, w = fl.inputs("albert")
    push(sim, dof[:K], roots[:K])
    B, N = int(sim._c_model.n_rb), 6 + sim.scene.n_dof
    eager_acc, eager_tau = launch_acc(sim, vd[:K], fl.ID_VELOCITY), launch_tau(sim, w[:K])     # (also the warm-up outside the capture)
    vd_t, w_t = torch.from_numpy(np.array(vd[:K])).to(sim.device), torch.from_numpy(np.array(w[:K])).to(sim.device)
    acc = torch.full((K, B, 6), float("nan"), dtype=torch.float32, device=sim.device)
    tau = torch.full((K, N), float("nan"), dtype=torch.float32, device=sim.device)
    lib, ctx = sim._lib, sim._ctx
    torch.cuda.synchronize()
    g, main = torch.cuda.CUDAGraph(), torch.cuda.current_stream()
    try:
        with torch.cuda.graph(g):      # one stream, two launches one after the other: no parallel branches
            capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            capi.check(lib, lib.mppi_sim_floating_link_acceleration(ctx, 0, B, ptr(vd_t), fl.ID_VELOCITY, ptr(acc)))
            capi.check(lib, lib.mppi_sim_floating_wrench_forces(ctx, 0, B, ptr(w_t), ptr(tau)))
    finally:
        capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(main.cuda_stream)))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(acc.cpu().numpy()), bits(eager_acc)) and np.array_equal(bits(tau.cpu().numpy()), bits(eager_tau))
    # the states changed by mppi_sim_set_states: the replay gives what direct calls give there
    push(sim, np.ascontiguousarray(dof[K:2 * K]), np.ascontiguousarray(roots[K:2 * K]))
    acc.fill_(float("nan"))
    tau.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(bits(acc.cpu().numpy()), bits(eager_acc)) and not np.array_equal(bits(tau.cpu().numpy()), bits(eager_tau))
    assert np.array_equal(bits(acc.cpu().numpy()), bits(launch_acc(sim, vd[:K], fl.ID_VELOCITY)))
    assert np.array_equal(bits(tau.cpu().numpy()), bits(launch_tau(sim, w[:K])))
    sim.stop_sim()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    lib = panda._lib
    acc_entry, tau_entry = lib.mppi_sim_floating_link_acceleration, lib.mppi_sim_floating_wrench_forces
    out = torch.full((K * 256,), float("nan"), dtype=torch.float32, device=panda.device)
    wr = torch.zeros((K * 64 * 6,), dtype=torch.float32, device=panda.device)

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(out).all())
    assert acc_entry(panda._ctx, 0, 1, None, 2, ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_floating_link_acceleration" in said and "fixed base" in said and "use mppi_sim_link_acceleration" in said
    assert tau_entry(panda._ctx, 0, 1, ptr(wr), ptr(out)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_floating_wrench_forces" in said and "fixed base" in said and "use mppi_sim_wrench_forces" in said
    assert untouched()                                              # nothing was launched
    panda.acquire_floating_link_bias_acceleration_tensor("panda")
    L = panda._actor_rb_range("panda")[1]
    for call in (panda.refresh_floating_link_bias_acceleration_tensors, lambda: panda.floating_link_accelerations("panda"),
                 lambda: panda.get_actor_link_floating_acceleration_by_name("panda", "panda_link7")):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_link_acceleration"):
            call()
    for call in (lambda: panda.floating_forces_from_wrenches("panda", np.zeros((L, 6), np.float32)),
                 lambda: panda.floating_forces_from_link_wrench("panda", "panda_link7", np.zeros(6, np.float32))):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_wrench_forces"):
            call()
    panda.stop_sim()
    # the forest of two jackals (conf/mppi/multi-jackal.yaml): a text of its own
    two = make_sim(["jackal_a", "jackal_b"], K, [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    assert int(two._c_model.n_extra_bases) == 1
    for rc in (acc_entry(two._ctx, 0, 1, None, 2, ptr(out)), tau_entry(two._ctx, 0, 1, ptr(wr), ptr(out))):
        said = lib.mppi_last_error().decode()
        assert rc == capi.MPPI_EUNSUPPORTED and "several moving bases" in said and "fixed base" not in said
    assert untouched()
    two.stop_sim()
    # null pointers, ranges outside [0, n_rb), bits other than MPPI_ID_VELOCITY
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    n, B = boxer.scene.n_dof, int(boxer._c_model.n_rb)
    ctx = boxer._ctx
    assert acc_entry(ctx, 0, B, None, 2, None) == capi.MPPI_EINVAL and "null output" in lib.mppi_last_error().decode()
    assert tau_entry(ctx, 0, B, None, ptr(out)) == capi.MPPI_EINVAL and "null wrenches" in lib.mppi_last_error().decode()
    assert tau_entry(ctx, 0, B, ptr(wr), None) == capi.MPPI_EINVAL and "null output" in lib.mppi_last_error().decode()
    for first, count in ((-1, 1), (0, 0), (B, 1), (0, B + 1), (B - 1, 2), (1, 2 ** 31 - 1)):
        assert acc_entry(ctx, first, count, None, 2, ptr(out)) == capi.MPPI_EINVAL and f"outside [0, {B})" in lib.mppi_last_error().decode(), (first, count)
        assert tau_entry(ctx, first, count, ptr(wr), ptr(out)) == capi.MPPI_EINVAL and f"outside [0, {B})" in lib.mppi_last_error().decode(), (first, count)
    for terms in (1, 3, 4, -1, 1 << 16):
        assert acc_entry(ctx, 0, B, None, terms, ptr(out)) == capi.MPPI_EINVAL and "unknown bits" in lib.mppi_last_error().decode(), terms
    assert untouched()
    # no change elsewhere: the fixed-base entries and the fixed wrapper methods keep refusing boxer
    assert lib.mppi_sim_link_acceleration(ctx, 0, B, None, 2, ptr(out)) == capi.MPPI_EUNSUPPORTED
    assert lib.mppi_last_error().decode().startswith("mppi_sim_link_acceleration: unsupported for a robot with a moving base")
    assert lib.mppi_sim_wrench_forces(ctx, 0, B, ptr(wr), ptr(out)) == capi.MPPI_EUNSUPPORTED
    assert lib.mppi_last_error().decode().startswith("mppi_sim_wrench_forces: unsupported for a robot with a moving base")
    assert untouched()
    for call in (lambda: boxer.link_accelerations("boxer"), lambda: boxer.joint_forces_from_wrenches("boxer", np.zeros((B, 6), np.float32))):
        with pytest.raises(NotImplementedError, match="moving base"):
            call()
    # the context is as healthy as before
    capi.check(lib, acc_entry(ctx, 0, B, None, 2, ptr(out)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got[:K * B * 6]).all() and np.isnan(got[K * B * 6:]).all()
    out.fill_(float("nan"))
    capi.check(lib, tau_entry(ctx, 0, B, ptr(wr), ptr(out)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not got[:K * (6 + n)].any() and np.isnan(got[K * (6 + n):]).all()    # zero wrenches: exact zeros
    boxer.stop_sim()


# ---- 9. the wrapper -----------------------------------------------------------------------------------------------------------------
def test_wrapper_tensors():
    K = 16
    sim = make_sim(["boxer"], K, BASE_INIT)
    N = 6 + sim.scene.n_dof
    dof, roots, vd, w = fl.inputs("boxer")
    push(sim, dof[:K], roots[:K])
    first, L = sim._actor_rb_range("boxer")
    link = sim.scene.robot_model["links"][L - 1]["name"]
    rb = sim.scene.rigid_body_index("boxer", link)
    t = sim.acquire_floating_link_bias_acceleration_tensor("boxer")
    assert tuple(t.shape) == (K, L, 6) and not t.any() and sim.acquire_floating_link_bias_acceleration_tensor("boxer") is t
    bias = launch_acc(sim, None, fl.ID_VELOCITY)
    assert not t.any()                                              # zero until refreshed
    sim.refresh_floating_link_bias_acceleration_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(bias[:, first:first + L]))
    # it changes on refresh only
    push(sim, np.ascontiguousarray(dof[K:2 * K]), np.ascontiguousarray(roots[K:2 * K]))
    assert np.array_equal(bits(t.cpu().numpy()), bits(bias[:, first:first + L]))
    bias2 = launch_acc(sim, None, fl.ID_VELOCITY)
    assert not np.array_equal(bias2, bias)
    sim.refresh_floating_link_bias_acceleration_tensors()
    assert np.array_equal(bits(t.cpu().numpy()), bits(bias2[:, first:first + L]))
    # fresh tensors: every combination, one row for all envs or one per env
    full = launch_acc(sim, vd[K:2 * K], fl.ID_VELOCITY)
    got = sim.floating_link_accelerations("boxer", vd=torch.from_numpy(np.array(vd[K:2 * K])))
    assert tuple(got.shape) == (K, L, 6) and np.array_equal(bits(got.cpu().numpy()), bits(full[:, first:first + L]))
    assert np.array_equal(bits(sim.floating_link_accelerations("boxer").cpu().numpy()), bits(bias2[:, first:first + L]))
    assert np.array_equal(bits(sim.floating_link_accelerations("boxer", vd=np.array(vd[K]), velocity=False).cpu().numpy()),
                          bits(launch_acc(sim, np.tile(vd[K], (K, 1)), 0)[:, first:first + L]))
    assert not sim.floating_link_accelerations("boxer", velocity=False).any()
    one = sim.get_actor_link_floating_acceleration_by_name("boxer", link, vd=np.array(vd[K:2 * K]))
    assert tuple(one.shape) == (K, 6) and np.array_equal(bits(one.cpu().numpy()), bits(full[:, rb]))
    wK = np.array(w[K:2 * K, first:first + L])
    tau = sim.floating_forces_from_wrenches("boxer", wK)
    assert tuple(tau.shape) == (K, N) and np.array_equal(bits(tau.cpu().numpy()), bits(launch_tau(sim, wK, first, L)))
    assert np.array_equal(bits(sim.floating_forces_from_wrenches("boxer", wK[0]).cpu().numpy()), bits(launch_tau(sim, np.tile(wK[0], (K, 1, 1)), first, L)))
    tau1 = sim.floating_forces_from_link_wrench("boxer", link, wK[:, L - 1])
    assert tuple(tau1.shape) == (K, N) and np.array_equal(bits(tau1.cpu().numpy()), bits(launch_tau(sim, wK[:, L - 1:L], rb, 1)))
    assert tuple(sim.floating_forces_from_link_wrench("boxer", link, wK[0, L - 1]).shape) == (K, N)
    with pytest.raises(ValueError, match=rf"vd has shape \({N - 1},\): expected \[{N}\] or \[{K}, {N}\]"):
        sim.floating_link_accelerations("boxer", vd=np.zeros(N - 1, np.float32))
    with pytest.raises(ValueError, match=rf"wrenches have shape \({K}, 6\): expected \[{L}, 6\] or \[{K}, {L}, 6\]"):
        sim.floating_forces_from_wrenches("boxer", np.zeros((K, 6), np.float32))
    with pytest.raises(ValueError, match=rf"wrenches have shape \(3,\): expected \[6\] or \[{K}, 6\]"):
        sim.floating_forces_from_link_wrench("boxer", link, np.zeros(3, np.float32))
    # a horizon view refuses all of them, with wording of their own
    with sim._horizon_view(dict(sim._state_t_own), K):
        for call in (lambda: sim.acquire_floating_link_bias_acceleration_tensor("boxer"), sim.refresh_floating_link_bias_acceleration_tensors,
                     lambda: sim.floating_link_accelerations("boxer"), lambda: sim.get_actor_link_floating_acceleration_by_name("boxer", link),
                     lambda: sim.floating_forces_from_wrenches("boxer", wK), lambda: sim.floating_forces_from_link_wrench("boxer", link, wK[0, 0])):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "moving-base link accelerations and wrench forces" in str(e.value)
    with pytest.raises(ValueError):
        sim.acquire_floating_link_bias_acceleration_tensor("no_such_actor")
    sim.stop_sim()
