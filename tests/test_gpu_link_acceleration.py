"""mppi_sim_link_acceleration / mppi_sim_wrench_forces (csrc/mppi_kernels.hpp k_sim_link_acceleration, k_sim_wrench_forces) and the
wrapper's link_accelerations / get_actor_link_acceleration_by_name / acquire_link_bias_acceleration_tensor /
refresh_link_bias_acceleration_tensors / joint_forces_from_wrenches / joint_forces_from_link_wrench on the GPU, against the fp64
references at the joint positions and rates the simulator itself holds: EVERY env, EVERY rigid body, EVERY entry.  Inputs, references,
metrics and tolerances: link_acceleration_cases.py (its conditions are checked on the oracle alone by test_link_acceleration.py);
outputs are NaN-filled before every launch and every entry must come back finite; the measured maxima are printed next to the
tolerances before anything is asserted.

 1 edges of the staged loads and stores: Panda (qdd / tau rows of 7 floats) at K = 1, 63, 64, 65, 130; gripper Panda (9, branched,
   prismatic fingers), point robot and heijn (3), the mobile manipulator (12) at K = 65.  Per row the four acceleration calls and the
   wrench call on the whole range of rigid bodies, one body at the first and at the last rigid body and a middle range; a guard row
   behind each output stays NaN; the wrapper's calls are the raw calls; the bias-acceleration tensor is zero until refreshed
 2 the Panda's base away from the origin, yawed AND rolled; the mobile manipulator with its prismatic base joints 420 m out - at the
   tolerance of its origin row; the gripper scene (a contact-scene context with a fixed-base robot): the block's and the table's bodies
   get zero rows and their wrenches are ignored
 3 two point robots in one forest: a robot's links do not move with the other robot's qdd, a wrench on one gives zeros in the other's joints
 4 against the device's own tensors: with qd = 0 acc = (mppi_sim_jacobian) qdd; the wrench forces are the contraction of the device
   Jacobian with the wrenches; tau . qd = sum w . (columns 7:13 of the rb rows of mppi_sim_materialise)
 5 both entries inside a captured torch.cuda.graph (one stream, no parallel branches) replay to the same bits
 6 refusals before any launch: a moving base (MPPI_EUNSUPPORTED, NotImplementedError), null pointers, a range past n_rb, MPPI_ID_GRAVITY
   or bit 4 in terms (MPPI_EINVAL), PerStepOnly on a horizon view, wrong shapes; the context serves a valid call afterwards
 7 a tree built on demand ([-1,0,1,1,3]) carries both kernels - in a process of its own, for the reason given in
   test_gpu_forward_dynamics.py"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inverse_dynamics_cases as ic
import jacobian_cases as jc
import link_acceleration_cases as lc
from mppiisaac.backend import capi
from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
from mppiisaac.utils.config_store import load_config

pytestmark = pytest.mark.gpu
V = lc.ID_VELOCITY
NAMES = {lc.FULL: "full", (V, False): "Jdot qd", (0, True): "J qdd", (0, False): "nothing"}


def make_sim(actors, K, init_positions=None):
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    return IsaacGymWrapper(icfg, actors=list(actors), init_positions=init_positions, num_envs=K)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(sim, a):
    return torch.from_numpy(np.array(a, np.float32)).to(sim.device)


def kernel_info(sim):
    buf = C.create_string_buffer(512)
    capi.check(sim._lib, sim._lib.mppi_kernel_info(sim._ctx, buf, 512))
    return buf.value.decode()


def launch_acc(sim, qdd, terms, first=0, count=None):
    """one raw call into a NaN-filled output with a guard row behind row K - 1 -> acc [K][count][6] (numpy); qdd: a device tensor or None"""
    K = sim.num_envs
    count = int(sim._c_model.n_rb) - first if count is None else count
    out = torch.full(((K + 1) * count * 6,), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_link_acceleration(sim._ctx, first, count, ptr(qdd), terms, ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * count * 6:]).all(), "the guard row behind acc was written"
    assert np.isfinite(got[:K * count * 6]).all(), "entries that were never written (or not finite)"
    return got[:K * count * 6].reshape(K, count, 6)


def launch_tau(sim, w, first=0):
    """one raw call on the wrenches w [K][count][6] (a device tensor) into a NaN-filled output with a guard row -> tau [K][n] (numpy)"""
    K, n = sim.num_envs, sim.scene.n_dof
    out = torch.full(((K + 1) * n,), float("nan"), dtype=torch.float32, device=sim.device)
    capi.check(sim._lib, sim._lib.mppi_sim_wrench_forces(sim._ctx, first, int(w.shape[1]), ptr(w), ptr(out)))
    got = out.cpu().numpy()
    assert np.isnan(got[K * n:]).all(), "the guard row behind tau was written"
    assert np.isfinite(got[:K * n]).all(), "entries that were never written (or not finite)"
    return got[:K * n].reshape(K, n)


def all_calls(sim, qdd, w):
    qdd_dev = dev(sim, qdd)
    return {call: launch_acc(sim, qdd_dev if call[1] else None, call[0]) for call in lc.ACC_CALLS}, launch_tau(sim, dev(sim, w))


def check(tag, sim, acc, tau, parts, D, tau_ref, Dj, zero, tols):
    """prints the measured maxima next to the tolerances, then asserts them, the exact zeros and that the partial calls sum to the full one"""
    K = sim.num_envs
    e = {c: lc.e_acc(acc[c], lc.combine(parts, *c)[:K], D) for c in acc}
    et = lc.e_tau(tau, tau_ref[:K], Dj)
    sl, sa = lc.e_acc(acc[(V, False)].astype(np.float64) + acc[(0, True)], acc[lc.FULL].astype(np.float64), D)
    print(f"\n[{tag}] K {K}: e_lin / e_ang " + " | ".join(f"{NAMES[c]} {a:.2e} / {b:.2e}" for c, (a, b) in e.items()) + f" (tol {tols[0]:.0e} / {tols[1]:.0e})"
          f" | parts - full {sl:.2e} / {sa:.2e} | e_tau {et:.2e} (tol {tols[2]:.0e})")
    wl, wa = max(a for a, _ in e.values()), max(b for _, b in e.values())
    assert wl <= tols[0], f"{tag}: e_lin {wl:.3e} > {tols[0]:.0e}"
    assert wa <= tols[1], f"{tag}: e_ang {wa:.3e} > {tols[1]:.0e}"
    assert et <= tols[2], f"{tag}: e_tau {et:.3e} > {tols[2]:.0e}"
    assert sl <= 2.0 * tols[0] and sa <= 2.0 * tols[1]
    assert not acc[(0, False)].any()                               # nothing asked for: exact zeros
    assert zero.any() and all(not a[:, zero].any() for a in acc.values())      # bodies without a Jacobian: exact zero rows
    return wl, wa, et


def set_inputs(sim, dof):
    sim.set_dof_state_tensor(torch.from_numpy(np.array(dof, np.float32)))
    got = sim._dof_state.cpu().numpy()
    assert np.array_equal(got, dof), "the simulator holds other joint states than the inputs"     # (the references were taken at these)
    return got


def place_base(sim, actor_name, pos, ori):
    row = np.zeros(13, np.float32)
    row[0:3], row[3:7] = pos, ori
    sim.set_root_state_tensor_by_actor_idx(torch.from_numpy(row), sim.scene.actor_index(actor_name))


def body_ranges(B):
    return [(0, 1), (B - 1, 1), (B // 3, max(B // 2, 1)), (0, B)]


# ---- 1. edges of the staged loads and stores ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,K", lc.STORE_EDGES, ids=[f"{r}-K{K}" for r, K in lc.STORE_EDGES])
def test_load_and_store_edges(robot, K):
    actors, actor_name, _, _ = lc.ROBOTS[robot]
    r = lc.references(robot)
    sim = make_sim(actors, K, [[0.0, 0.0, 0.0]])
    assert np.array_equal(sim._root_state[0].cpu().numpy(), r.root.astype(np.float32))
    dof, qdd, w = lc.inputs(robot)
    set_inputs(sim, dof[:K])
    B, n = int(sim._c_model.n_rb), sim.scene.n_dof
    assert B == r.J.shape[1]
    acc, tau = all_calls(sim, qdd[:K], w[:K])
    tols = lc.tolerances(robot)
    check(f"edges {robot}", sim, acc, tau, r.parts, r.D, r.tau_ref, r.Dj, r.zero, tols)
    # body ranges: one body at the first and the last rigid body, a middle range, the whole range
    qdd_dev, w_dev = dev(sim, qdd[:K]), dev(sim, w[:K])
    for first, count in body_ranges(B):
        assert np.array_equal(launch_acc(sim, qdd_dev, V, first, count), acc[lc.FULL][:, first:first + count])
        assert np.array_equal(launch_acc(sim, None, V, first, count), acc[(V, False)][:, first:first + count])
        t = launch_tau(sim, w_dev[:, first:first + count].contiguous(), first)
        assert lc.e_tau(t, lc.wrench_reference(r.J[:K, first:first + count], w[:K, first:first + count]), r.Dj) <= tols[2]
    # the wrapper: its calls are the raw calls; the bias-acceleration tensor is zero until refreshed
    afirst, L = sim._actor_rb_range(actor_name)
    links = slice(afirst, afirst + L)
    bias = sim.acquire_link_bias_acceleration_tensor(actor_name)
    assert tuple(bias.shape) == (K, L, 6) and not bias.any()
    assert sim.acquire_link_bias_acceleration_tensor(actor_name) is bias
    sim.refresh_link_bias_acceleration_tensors()
    assert np.array_equal(bias.cpu().numpy(), acc[(V, False)][:, links])
    assert np.array_equal(sim.link_accelerations(actor_name).cpu().numpy(), acc[(V, False)][:, links])
    assert np.array_equal(sim.link_accelerations(actor_name, qdd_dev).cpu().numpy(), acc[lc.FULL][:, links])
    assert np.array_equal(sim.link_accelerations(actor_name, qdd_dev, velocity=False).cpu().numpy(), acc[(0, True)][:, links])
    assert not sim.link_accelerations(actor_name, velocity=False).any()
    last = sim.scene.robot_model["links"][-1]["name"]
    rb = sim.scene.rigid_body_index(actor_name, last)
    one = sim.get_actor_link_acceleration_by_name(actor_name, last, qdd_dev)
    assert tuple(one.shape) == (K, 6) and np.array_equal(one.cpu().numpy(), acc[lc.FULL][:, rb])
    assert np.array_equal(sim.joint_forces_from_wrenches(actor_name, w_dev[:, links].contiguous()).cpu().numpy(), launch_tau(sim, w_dev[:, links].contiguous(), afirst))
    same = sim.joint_forces_from_wrenches(actor_name, w_dev[0, links])
    assert tuple(same.shape) == (K, n) and np.array_equal(same[0].cpu().numpy(), launch_tau(sim, w_dev[:, links].contiguous(), afirst)[0])
    t1 = sim.joint_forces_from_link_wrench(actor_name, last, w_dev[:, rb])
    assert np.array_equal(t1.cpu().numpy(), launch_tau(sim, w_dev[:, rb:rb + 1].contiguous(), rb))
    assert np.array_equal(sim.joint_forces_from_link_wrench(actor_name, last, w_dev[0, rb])[0].cpu().numpy(), t1[0].cpu().numpy())
    sim.stop_sim()


# ---- 2. tilted, far, the gripper scene ----------------------------------------------------------------------------------------------
def test_base_yawed_and_rolled():
    K = 65
    r = lc.references("franka_panda", "tilted")
    sim = make_sim(["panda"], K, [jc.OFFSET_POS])
    place_base(sim, "panda", jc.OFFSET_POS, ic.TILT_ORI)
    assert np.array_equal(sim._root_state[0].cpu().numpy(), r.root.astype(np.float32))
    dof, qdd, w = lc.inputs("franka_panda", "tilted")
    set_inputs(sim, dof[:K])
    acc, tau = all_calls(sim, qdd[:K], w[:K])
    tols = lc.tolerances("franka_panda")
    check("tilted franka_panda", sim, acc, tau, r.parts, r.D, r.tau_ref, r.Dj, r.zero, tols)
    # the row cannot pass by ignoring the base pose: the upright base's references are off by hundreds of tolerances
    up = lc.references("franka_panda")
    assert lc.e_acc(acc[lc.FULL], lc.combine(up.parts, *lc.FULL)[:K], r.D)[0] > 100.0 * tols[0] and lc.e_tau(tau, up.tau_ref[:K], r.Dj) > 100.0 * tols[2]
    sim.stop_sim()


def test_mobile_manipulator_far_from_the_origin():
    K = 65
    r, origin = lc.references("omnipanda", "far"), lc.references("omnipanda", "origin")
    sim = make_sim(["omnipanda"], K, [[0.0, 0.0, 0.0]])
    dof, qdd, w = lc.inputs("omnipanda", "far")
    set_inputs(sim, dof[:K])
    pos = sim._rigid_body_state.cpu().numpy()[:, -1, 0:2]
    assert np.abs(pos).min() > ic.FAR - 5.0                       # the arm does stand 420 m out, in x and in y
    tols = lc.tolerances_from(origin.w32)                         # the tolerance of the origin row alone
    assert all(a <= b for a, b in zip(tols, lc.tolerances("omnipanda")))
    acc, tau = all_calls(sim, qdd[:K], w[:K])
    check("far omnipanda, at the tolerance of origin", sim, acc, tau, r.parts, r.D, r.tau_ref, r.Dj, r.zero, tols)
    sim.stop_sim()


def test_contact_scene_context(oracle64):
    K = 65
    r = lc.references("panda_gripper")
    sim = make_sim(jc.GRIPPER_SCENE, K, [[0.0, 0.0, 0.0]])
    assert " step=scene" in kernel_info(sim), kernel_info(sim)
    assert np.array_equal(sim._root_state[0, sim.scene.robot_idx].cpu().numpy(), r.root[0].astype(np.float32))
    dof, qdd, _ = lc.inputs("panda_gripper")
    set_inputs(sim, dof[:K])
    model, root = sim._c_model, sim._root_state[0].cpu().numpy().astype(np.float64)
    B = int(model.n_rb)
    first, L = sim._actor_rb_range("panda")
    assert B > L
    w = lc.wrenches(K, B)
    J, parts = lc.reference_parts(oracle64, model, root, dof[:K, 0::2], dof[:K, 1::2], qdd[:K])
    zero = lc.zero_bodies(J)
    others = np.ones(B, bool)
    others[first:first + L] = False
    assert zero[others].all() and zero.sum() == others.sum() + r.zero.sum()      # the block's and the table's bodies, and the welded link
    tau_ref = lc.wrench_reference(J, w)
    acc, tau = all_calls(sim, qdd[:K], w)
    check("contact scene panda_gripper", sim, acc, tau, parts, r.D, tau_ref, np.abs(tau_ref).max(0), zero, lc.tolerances("panda_gripper"))
    poisoned = np.array(w)
    poisoned[:, zero] = np.nan
    assert np.array_equal(launch_tau(sim, dev(sim, poisoned)), tau)            # the wrenches on the block and the table are ignored
    sim.stop_sim()


# ---- 3. two point robots in one forest ----------------------------------------------------------------------------------------------
def test_two_point_robots_are_one_forest(oracle64):
    K = 65
    actors, init = jc.two_point_robot_actors()
    sim = make_sim(actors, K, init)
    n = sim.scene.n_dof
    assert n == 6
    rng = np.random.default_rng(lc.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(-2.0, 2.0, size=(K, n)), rng.uniform(-ic.QD_AMP, ic.QD_AMP, size=(K, n))
    qdd = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, n)).astype(np.float32)
    set_inputs(sim, dof)
    model, root = sim._c_model, sim._root_state[0].cpu().numpy().astype(np.float64)
    w = lc.wrenches(K, int(model.n_rb))
    J, parts = lc.reference_parts(oracle64, model, root, dof[:, 0::2], dof[:, 1::2], qdd)
    tau_ref = lc.wrench_reference(J, w)
    D, Dj, zero = lc.scales(parts), np.abs(tau_ref).max(0), lc.zero_bodies(J)
    tols = lc.tolerances("point_robot")
    acc, tau = all_calls(sim, qdd, w)
    check("two point robots", sim, acc, tau, parts, D, tau_ref, Dj, zero, tols)
    of_first = ~np.abs(J[:, :, :, 3:]).max((0, 2, 3)).astype(bool) & ~zero
    of_second = ~np.abs(J[:, :, :, :3]).max((0, 2, 3)).astype(bool) & ~zero
    assert of_first.any() and of_second.any() and not (of_first & of_second).any()
    other = np.array(qdd)
    other[:, 3:] = -other[:, 3:]
    again = launch_acc(sim, dev(sim, other), V)
    assert np.array_equal(again[:, of_first], acc[lc.FULL][:, of_first])         # the first robot's links: bit for bit
    assert np.abs(again[:, of_second] - acc[lc.FULL][:, of_second]).max((1, 2)).min() > 100.0 * tols[0] * D[0]     # the second robot's: every env moved
    only = np.zeros_like(w)
    only[:, of_first] = w[:, of_first]
    t1 = launch_tau(sim, dev(sim, only))
    assert not t1[:, 3:].any() and np.abs(t1[:, :3]).max(1).min() > 0.0        # a wrench on one robot: zeros in the other's joints
    sim.stop_sim()


# ---- 4. against the device's own tensors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["franka_panda", "omnipanda"])
def test_against_the_devices_own_tensors(robot):
    K = 65
    actors, actor_name, _, _ = lc.ROBOTS[robot]
    r = lc.references(robot)
    sim = make_sim(actors, K, [[0.0, 0.0, 0.0]])
    dof, qdd, w = lc.inputs(robot)
    tl, ta, tt = lc.tolerances(robot)
    tol_J = jc.tolerances(robot)[0]
    B = int(sim._c_model.n_rb)
    first, L = sim._actor_rb_range(actor_name)
    assert (first, L) == (0, B)
    Jt = sim.acquire_jacobian_tensor(actor_name)
    # the wrench forces against the contraction of the device Jacobian with the wrenches
    set_inputs(sim, dof[:K])
    sim.refresh_jacobian_tensors()
    Jd = Jt.cpu().numpy().astype(np.float64)
    tau = launch_tau(sim, dev(sim, w[:K]))
    gap = np.abs(tau - np.einsum("kbri,kbr->ki", Jd, w[:K].astype(np.float64)))
    bound = tol_J * np.abs(w[:K]).sum((1, 2))[:, None] + tt * r.Dj[None, :]
    print(f"\n[{robot}] wrench forces against J_dev^T w: worst gap / bound {(gap / bound).max():.3f}")
    assert (gap <= bound).all()
    # tau . qd against sum w . (columns 7:13 of the rb rows of mppi_sim_materialise)
    vl, va = jc.velocity_tolerances(False)
    rb = sim._rigid_body_state.cpu().numpy().astype(np.float64)
    qd = dof[:K, 1::2].astype(np.float64)
    gap = np.abs(np.einsum("ki,ki->k", tau.astype(np.float64), qd) - np.einsum("kbr,kbr->k", w[:K].astype(np.float64), rb[:, :, 7:13]))
    bound = vl * np.abs(w[:K, :, 0:3]).sum((1, 2)) + va * np.abs(w[:K, :, 3:6]).sum((1, 2)) + tt * np.abs(qd) @ r.Dj
    print(f"[{robot}] tau . qd against sum w . v of the rb rows: worst gap / bound {(gap / bound).max():.3f}")
    assert (gap <= bound).all()
    # with qd = 0: acc = (mppi_sim_jacobian) qdd
    still = np.array(dof[:K])
    still[:, 1::2] = 0.0
    set_inputs(sim, still)
    acc = launch_acc(sim, dev(sim, qdd[:K]), V)
    want = np.einsum("kbri,ki->kbr", Jd, qdd[:K].astype(np.float64))
    gap = np.abs(acc - want)
    l1 = np.abs(qdd[:K]).sum(1)[:, None, None]
    assert (gap[:, :, 0:3] <= tol_J * l1 + tl * r.D[0]).all() and (gap[:, :, 3:6] <= tol_J * l1 + ta * r.D[1]).all()
    print(f"[{robot}] qd = 0: acc against J_dev qdd: {gap.max():.2e}")
    sim.stop_sim()


# ---- 5. inside a captured graph -----------------------------------------------------------------------------------------------------
def test_both_entries_replay_from_a_captured_graph():
    K = 65
    sim = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    dof, qdd, w = lc.inputs("franka_panda")
    set_inputs(sim, dof[:K])
    B, n = int(sim._c_model.n_rb), sim.scene.n_dof
    qdd_dev, w_dev = dev(sim, qdd[:K]), dev(sim, w[:K])
    eager_acc, eager_tau = launch_acc(sim, qdd_dev, V), launch_tau(sim, w_dev)      # (also the warm-up outside the capture)
    acc = torch.full((K, B, 6), float("nan"), dtype=torch.float32, device=sim.device)
    tau = torch.full((K, n), float("nan"), dtype=torch.float32, device=sim.device)
    lib, ctx = sim._lib, sim._ctx
    torch.cuda.synchronize()
    g, main = torch.cuda.CUDAGraph(), torch.cuda.current_stream()
    try:
        with torch.cuda.graph(g):      # one stream, the two launches one after the other: no parallel branches
            capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            capi.check(lib, lib.mppi_sim_link_acceleration(ctx, 0, B, ptr(qdd_dev), V, ptr(acc)))
            capi.check(lib, lib.mppi_sim_wrench_forces(ctx, 0, B, ptr(w_dev), ptr(tau)))
    finally:
        capi.check(lib, lib.mppi_set_stream(ctx, C.c_void_p(main.cuda_stream)))
    for _ in range(2):
        acc.fill_(float("nan"))
        tau.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(acc.cpu().numpy(), eager_acc) and np.array_equal(tau.cpu().numpy(), eager_tau)
    # the replay follows the envs' current state: at other joint states it gives what the eager call gives there
    set_inputs(sim, np.ascontiguousarray(dof[K:2 * K]))
    g.replay()
    torch.cuda.synchronize()
    assert not np.array_equal(acc.cpu().numpy(), eager_acc)
    assert np.array_equal(acc.cpu().numpy(), launch_acc(sim, qdd_dev, V)) and np.array_equal(tau.cpu().numpy(), launch_tau(sim, w_dev))
    sim.stop_sim()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    K = 8
    boxer = make_sim(["boxer"], K, [[0.0, 0.0, 0.05]])
    lib = boxer._lib
    n, B = boxer.scene.n_dof, int(boxer._c_model.n_rb)
    out = torch.full((K, B, 6), float("nan"), dtype=torch.float32, device=boxer.device)
    tout = torch.full((K, n), float("nan"), dtype=torch.float32, device=boxer.device)
    qdd = torch.zeros((K, n), dtype=torch.float32, device=boxer.device)
    w = torch.zeros((K, B, 6), dtype=torch.float32, device=boxer.device)
    for a in (qdd, None):
        assert lib.mppi_sim_link_acceleration(boxer._ctx, 0, B, ptr(a), V, ptr(out)) == capi.MPPI_EUNSUPPORTED
        said = lib.mppi_last_error().decode()
        assert "mppi_sim_link_acceleration" in said and "moving base" in said and "unsupported" in said
    assert lib.mppi_sim_wrench_forces(boxer._ctx, 0, B, ptr(w), ptr(tout)) == capi.MPPI_EUNSUPPORTED
    said = lib.mppi_last_error().decode()
    assert "mppi_sim_wrench_forces" in said and "moving base" in said and "unsupported" in said
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(tout).all())      # nothing was launched
    boxer.acquire_link_bias_acceleration_tensor("boxer")
    link = boxer.scene.robot_model["links"][-1]["name"]
    for call in (lambda: boxer.link_accelerations("boxer"), lambda: boxer.link_accelerations("boxer", qdd), lambda: boxer.get_actor_link_acceleration_by_name("boxer", link),
                 boxer.refresh_link_bias_acceleration_tensors, lambda: boxer.joint_forces_from_wrenches("boxer", w[:, :boxer._actor_rb_range("boxer")[1]]),
                 lambda: boxer.joint_forces_from_link_wrench("boxer", link, w[0, 0])):
        with pytest.raises(NotImplementedError, match="moving base"):
            call()
    boxer.stop_sim()
    panda = make_sim(["panda"], K, [[0.0, 0.0, 0.0]])
    n, B = panda.scene.n_dof, int(panda._c_model.n_rb)
    out = torch.full((K, B, 6), float("nan"), dtype=torch.float32, device=panda.device)
    tout = torch.full((K, n), float("nan"), dtype=torch.float32, device=panda.device)
    qdd = torch.zeros((K, n), dtype=torch.float32, device=panda.device)
    w = torch.zeros((K, B, 6), dtype=torch.float32, device=panda.device)
    ctx = panda._ctx
    assert lib.mppi_sim_link_acceleration(ctx, 0, B, ptr(qdd), V, None) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    assert lib.mppi_sim_wrench_forces(ctx, 0, B, None, ptr(tout)) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    assert lib.mppi_sim_wrench_forces(ctx, 0, B, ptr(w), None) == capi.MPPI_EINVAL and "null" in lib.mppi_last_error().decode()
    for first, count in ((0, B + 1), (B, 1), (B - 1, 2), (-1, 1), (0, 0), (1, (1 << 31) - 1)):
        assert lib.mppi_sim_link_acceleration(ctx, first, count, ptr(qdd), V, ptr(out)) == capi.MPPI_EINVAL, (first, count)
        assert "outside [0, " in lib.mppi_last_error().decode()
        assert lib.mppi_sim_wrench_forces(ctx, first, count, ptr(w), ptr(tout)) == capi.MPPI_EINVAL, (first, count)
        assert "outside [0, " in lib.mppi_last_error().decode()
    for terms in (lc.ID_GRAVITY, lc.ID_GRAVITY | V, 16, 16 | V, 4, -1, 1 << 30):       # gravity has no part in it; bit 4; other bits
        assert lib.mppi_sim_link_acceleration(ctx, 0, B, ptr(qdd), terms, ptr(out)) == capi.MPPI_EINVAL, terms
        assert "unknown bits" in lib.mppi_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(tout).all())
    # a horizon view refuses all of them
    bias = panda.acquire_link_bias_acceleration_tensor("panda")
    with panda._horizon_view(dict(panda._state_t_own), K):
        for call in (lambda: panda.link_accelerations("panda"), lambda: panda.get_actor_link_acceleration_by_name("panda", "panda_link7"),
                     lambda: panda.acquire_link_bias_acceleration_tensor("panda"), panda.refresh_link_bias_acceleration_tensors,
                     lambda: panda.joint_forces_from_wrenches("panda", w), lambda: panda.joint_forces_from_link_wrench("panda", "panda_link7", w[0, 0])):
            with pytest.raises(RuntimeError, match="per-step only") as e:
                call()
            assert isinstance(e.value, PerStepOnly) and "link accelerations" in str(e.value)
    # wrong shapes name the expected ones
    for wrong in (torch.zeros(n + 1), torch.zeros(K, n + 1), torch.zeros(K + 1, n), torch.zeros(1, n), torch.zeros(())):
        with pytest.raises(ValueError, match=rf"qdd has shape .* expected \[{n}\] or \[{K}, {n}\]"):
            panda.link_accelerations("panda", wrong)
    for wrong in (torch.zeros(B, 5), torch.zeros(K, B + 1, 6), torch.zeros(K + 1, B, 6), torch.zeros(6), torch.zeros(())):
        with pytest.raises(ValueError, match=rf"wrenches have shape .* expected \[{B}, 6\] or \[{K}, {B}, 6\]"):
            panda.joint_forces_from_wrenches("panda", wrong)
    for wrong in (torch.zeros(5), torch.zeros(K, 5), torch.zeros(K + 1, 6), torch.zeros(K, 1, 6)):
        with pytest.raises(ValueError, match=rf"wrenches have shape .* expected \[6\] or \[{K}, 6\]"):
            panda.joint_forces_from_link_wrench("panda", "panda_link7", wrong)
    with pytest.raises(ValueError):
        panda.link_accelerations("no_such_actor")
    # the context is as healthy as before
    capi.check(lib, lib.mppi_sim_link_acceleration(ctx, 0, B, ptr(qdd), V, ptr(out)))
    capi.check(lib, lib.mppi_sim_wrench_forces(ctx, 0, B, ptr(w), ptr(tout)))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(tout).all()) and not bias.any()
    panda.stop_sim()


# ---- 7. a tree built on demand ------------------------------------------------------------------------------------------------------
def on_demand_tree(tmp):
    """runs in a process of its own (see the module docstring): builds the tree [-1,0,1,1,3] into an empty cache under tmp and checks
    both kernels of the plugin against the references"""
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
    rng = np.random.default_rng(lc.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(lo, hi, size=(K, n)), rng.uniform(-ic.QD_AMP, ic.QD_AMP, size=(K, n))
    qdd = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, n)).astype(np.float32)
    set_inputs(sim, dof)
    w = lc.wrenches(K, int(sim._c_model.n_rb))
    r = lc.references_of(sim.scene, dof, qdd, w)      # the rule of the cases file on these inputs
    assert np.array_equal(sim._root_state[0].cpu().numpy(), np.asarray(r.root, np.float32))
    acc, tau = all_calls(sim, qdd, w)
    check("on-demand tree [-1,0,1,1,3]", sim, acc, tau, r.parts, r.D, r.tau_ref, r.Dj, r.zero, lc.tolerances_from(r.w32))
    sim.stop_sim()


def test_tree_built_on_demand(tmp_path):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp_path)], env=env, capture_output=True, text=True)
    print(run.stdout[-2000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "[on-demand tree [-1,0,1,1,3]]" in run.stdout


if __name__ == "__main__":
    on_demand_tree(sys.argv[1])
