"""Per-env states into the batched simulator - mppi_sim_set_states, mppi_sim_set_states_indexed, mppi_sim_reset_indexed
(k_sim_set_states, k_sim_set_states_scene of csrc/mppi_kernels.hpp) - through the raw C-ABI, and the wrapper surface on top of them
(IsaacGymWrapper.set_dof_state_tensor, set_actor_root_state_tensor, their _indexed forms, reset_envs):
 1  round trip set -> mppi_sim_materialise without a step: the rows come back in bits, the shared rows are x0's, cf is zero
 2  steps from per-env starts with per-env commands against the fp64 oracle's orc_envs_step, per env, every step, every column,
    under each of the four step kernels (`lane`, `quad`, `scene`, `scene-quad`, asserted by name)
 3  partial inputs: dof alone leaves the roots at x0, root alone leaves the dof at x0
 4  indexed calls: touched envs take their rows, untouched envs keep every bit, ids outside [0, K) change nothing, the steps that
    follow match the oracle; mppi_sim_reset_indexed returns the listed envs to x0 and zeroes their cost accumulators
 5  the existing entry points afterwards: mppi_sim_reset restores x0 everywhere, a planner's command does not see the scatter
 6  the wrapper: the reference's in-place-edit idiom, the refusals, reset_envs
Inputs and their conditions: per_env_states.py, test_per_env_states.py.  Tolerances: test_gpu_step_matrix.TOL, unchanged.

Measured on the MI355X, test 2 (worst env, step and column over the cases of a scene, next to TOL):
  panda    q 6.3e-07 (1e-05) | qd 8.3e-08 (5e-05) | pos 4.2e-07 (5e-06) | quat 4.7e-07 (1e-05) | lin 8.3e-07 (5e-05) | ang 9.3e-07 (5e-05) | cf 0 (0)
  boxer    q 1.3e-06 (2e-05) | qd 2.5e-05 (2e-04) | pos 7.6e-07 (1e-05) | quat 1.0e-06 (2e-05) | lin 3.3e-05 (5e-04) | ang 9.9e-05 (1e-03) | cf 3.8e-02 (5e-01)
  pick     q 5.0e-07 (2e-05) | qd 1.9e-07 (2e-04) | pos 2.4e-07 (1e-05) | quat 7.9e-07 (2e-05) | lin 5.8e-07 (5e-04) | ang 5.5e-05 (1e-03) | cf 1.3e-08 (5e-01)
  jackals  q 2.6e-08 (2e-05) | qd 4.5e-07 (2e-04) | pos 5.9e-07 (1e-05) | quat 9.1e-08 (2e-05) | lin 1.5e-06 (5e-04) | ang 7.1e-06 (1e-03) | cf 4.5e-04 (5e-01)
(`scene` and `scene-quad` agree on the pushing scene to the digits shown.)

Not covered: an env of 3-4 free actors (its kernels are built on demand, 12-35 s); the two-slot scenes with one free actor exercise
the zero-filled slot that `free_slots` sizes."""
import ctypes as C

import numpy as np
import pytest

from mppiisaac.backend import capi
from per_env_states import (INDEXED, ROUND_TRIP, SEED_OTHER, STEP_CASES, STEP_IDS, mixed_starts, per_env_actors, reference, reference_mixed, scene_case, starts,
                            touched)
from scenes import panda_reach
from test_gpu_rollout_matrix import AUTO, Gpu
from test_gpu_step_matrix import Tensors, build, commands, compare, open_context, stacked

pytestmark = pytest.mark.gpu
NAN = np.float32("nan")


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return capi.load_library()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # (a contiguous copy: the shared inputs are read-only)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def hidden(root, m):
    """the root input with the rows that are not per env made NaN: the kernels must not read them"""
    out = root.copy()
    out[:, [a for a in range(m.n_actors) if a not in per_env_actors(m)]] = NAN
    return out


def expected_root(root, b):
    """what comes back: the per-env rows of the input, the shared rows of x0"""
    out = np.tile(b.root.reshape(1, b.m.n_actors, 13), (len(root), 1, 1))
    mine = per_env_actors(b.m)
    out[:, mine] = root[:, mine]
    return out


def context(lib, scene, K, env=(), step=""):
    import dataclasses
    case = dataclasses.replace(scene_case(scene, K), env=env, step=step)
    b = build(case)
    g = open_context(lib, case, b) if step else Gpu(lib, b, AUTO)
    g.call("mppi_sim_reset")
    return case, b, g


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits(got, want, msg):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,K", ROUND_TRIP, ids=[f"{s}-K{K}" for s, K in ROUND_TRIP])
def test_round_trip_without_a_step(scene, K, lib):
    case, b, g = context(lib, scene, K)
    _, dof, root = starts(scene)
    d_dof, d_root = dev(dof[:K]), dev(hidden(root[:K], b.m))
    g.call("mppi_sim_set_states", ptr(d_dof), ptr(d_root))
    got = Tensors(b.m, K).fill(g, "mppi_sim_materialise")
    g.close()
    assert_bits(got["dof"], dof[:K], f"{case.name}: dof rows")
    assert_bits(got["root"], expected_root(root[:K], b), f"{case.name}: root rows (per-env rows from the input, shared rows from x0)")
    assert not got["cf"].any() and np.isfinite(got["rb"]).all()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def step_and_compare(g, case, b, u, want, tag):
    T, rows = Tensors(b.m, case.K), []
    d_u = dev(u)
    for t in range(case.N):
        g.call("mppi_sim_step", ptr(d_u[t]), 0)
        rows.append(T.fill(g, "mppi_sim_materialise"))
    got = stacked(rows)
    fails, worst = compare(tag, got, want, case.klass)
    if case.klass != "contact":
        assert not got["cf"].any(), "contact forces of a contact-free scene"
    return fails


@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_steps_from_per_env_starts_match_the_oracle(case, lib, oracle64):
    b = build(case)
    try:
        g = open_context(lib, case, b)        # (asserts ` step=<name> ` of mppi_kernel_info)
    except capi.MppiHipError as e:
        # the one-lane kernels keep 64 envs' rows in LDS per wavefront: a scene that needs more than 160 KiB for them is refused
        assert case.may_refuse and "libmppi_hip error -3" in str(e) and "160 KiB" in str(e), (case.name, e)
        print(f"{case.name}: mppi_create refuses the one-lane kernels of this scene ({e})")
        return
    _, dof, root = starts(case.scene)
    K = case.K
    d_dof, d_root = dev(dof[:K]), dev(hidden(root[:K], b.m))
    g.call("mppi_sim_reset")
    g.call("mppi_sim_set_states", ptr(d_dof), ptr(d_root))
    fails = step_and_compare(g, case, b, commands(case, b.cfg.nu), reference(oracle64, case.scene, K), f"{case.name} step={case.step}")
    g.close()
    assert not fails, "\n".join(fails)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,K", [("panda", 65), ("boxer", 17), ("boxer", 65), ("jackals", 5)])
def test_partial_inputs_leave_the_other_part_at_x0(scene, K, lib):
    case, b, g = context(lib, scene, K)
    _, dof, root = starts(scene)
    m, T = b.m, Tensors(b.m, K)
    d_dof, d_root = dev(dof[:K]), dev(hidden(root[:K], m))
    # another x0 than the one the envs hold, pending until the reset
    dof1 = (b.dof + 0.05 * np.cos(np.arange(b.dof.size))).astype(np.float32)
    root1 = b.root.copy().reshape(m.n_actors, 13)
    root1[:, 0:2] += np.float32(0.125) * (1 + np.arange(m.n_actors, dtype=np.float32))[:, None]
    x0 = type(b)(root=root1, m=m)
    for part in ("dof", "root"):
        g.call("mppi_sim_set_states", ptr(d_dof), ptr(d_root))      # (something else than x0 in every env)
        g.call("mppi_set_state", capi.fptr(dof1), capi.fptr(root1))
        g.call("mppi_sim_reset")
        g.call("mppi_sim_set_states", ptr(d_dof) if part == "dof" else None, ptr(d_root) if part == "root" else None)
        got = T.fill(g, "mppi_sim_materialise")
        assert_bits(got["dof"], dof[:K] if part == "dof" else np.tile(dof1[None], (K, 1)), f"{case.name}: dof rows after a {part}-only call")
        assert_bits(got["root"], expected_root(root[:K], x0) if part == "root" else np.tile(root1[None], (K, 1, 1)), f"{case.name}: root rows after a {part}-only call")
        assert not got["cf"].any()
    assert lib.mppi_sim_set_states(g.ctx, None, None) == capi.MPPI_EINVAL
    assert lib.mppi_sim_set_states_indexed(g.ctx, None, 0, None, None) == capi.MPPI_EINVAL
    assert lib.mppi_sim_set_states_indexed(g.ctx, None, 3, ptr(d_dof), None) == capi.MPPI_EINVAL
    assert lib.mppi_sim_reset_indexed(g.ctx, None, -1) == capi.MPPI_EINVAL
    g.close()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,K", INDEXED, ids=[f"{s}-K{K}" for s, K in INDEXED])
def test_indexed_calls_touch_the_listed_envs_only(scene, K, lib, oracle64):
    import torch
    case, b, g = context(lib, scene, K)
    m, T = b.m, Tensors(b.m, K)
    _, dof, root = starts(scene)
    ids, dofm, rootm = mixed_starts(scene, K)
    assert ids == touched(K)
    d_dof, d_root = dev(dof[:K]), dev(hidden(root[:K], m))
    g.call("mppi_sim_set_states", ptr(d_dof), ptr(d_root))
    before = T.fill(g, "mppi_sim_materialise")
    # ids outside [0, K) alone: nothing changes (their rows are NaN: a write anywhere would show)
    junk = dev(np.array([-1, K, K + 63, -2 ** 31], np.int32))
    j_dof, j_root = dev(np.full((4, 2 * m.n_bodies), NAN, np.float32)), dev(np.full((4, m.n_actors, 13), NAN, np.float32))
    g.call("mppi_sim_set_states_indexed", ptr(junk), 4, ptr(j_dof), ptr(j_root))
    g.call("mppi_sim_reset_indexed", ptr(junk), 4)
    after = T.fill(g, "mppi_sim_materialise")
    for key in before:
        assert_bits(after[key], before[key], f"{case.name}: {key} after calls with ids outside [0, K) only")
    # the listed envs in a shuffled order, an id of -1 and an id of K among them (rows of NaN)
    lst = [ids[0], -1] + ids[1:3] + [K] + ids[3:]
    rows_dof = np.full((len(lst), 2 * m.n_bodies), NAN, np.float32)
    rows_root = np.full((len(lst), m.n_actors, 13), NAN, np.float32)
    for j, k in enumerate(lst):
        if 0 <= k < K:
            rows_dof[j], rows_root[j] = dofm[k], rootm[k]
    d_ids, d_rd, d_rr = dev(np.array(lst, np.int32)), dev(rows_dof), dev(hidden(rows_root, m))
    g.call("mppi_sim_set_states_indexed", ptr(d_ids), len(lst), ptr(d_rd), ptr(d_rr))
    got = T.fill(g, "mppi_sim_materialise")
    rest = [k for k in range(K) if k not in ids]
    assert_bits(got["dof"][ids], dofm[ids], f"{case.name}: dof rows of the touched envs")
    assert_bits(got["root"][ids], expected_root(rootm[ids], b), f"{case.name}: root rows of the touched envs")
    assert not got["cf"].any()
    for key in before:
        assert_bits(got[key][rest], before[key][rest], f"{case.name}: {key} of the untouched envs")
    # the steps from there
    fails = step_and_compare(g, case, b, commands(case, b.cfg.nu), reference_mixed(oracle64, scene, K), f"{case.name} indexed")
    assert not fails, "\n".join(fails)
    # cost accumulators that are not zero: S = (k + 1) / 128, a control cost from one mode-2 step under a nominal that is not zero
    g.call("mppi_set_nominal", capi.fptr(np.full((b.cfg.horizon, b.cfg.nu), 0.5, np.float32)))
    S0 = (1.0 + np.arange(K, dtype=np.float32)) / np.float32(128.0)
    cost = dev(S0)
    g.call("mppi_sim_accumulate_cost", 0, ptr(cost))
    g.call("mppi_sim_step_horizon", 0)
    before = T.fill(g, "mppi_sim_materialise")
    half = [k for k in range(K) if k % 2 == 0]
    keep = [k for k in range(K) if k % 2 == 1]
    d_half = dev(np.array(half[::-1] + [K, -1], np.int32))
    g.call("mppi_sim_reset_indexed", ptr(d_half), len(half) + 2)
    got = T.fill(g, "mppi_sim_materialise")
    assert_bits(got["dof"][half], np.tile(b.dof.reshape(1, -1), (len(half), 1)), f"{case.name}: dof rows of the reset envs")
    assert_bits(got["root"][half], np.tile(b.root.reshape(1, m.n_actors, 13), (len(half), 1, 1)), f"{case.name}: root rows of the reset envs")
    assert not got["cf"][half].any()
    for key in before:
        assert_bits(got[key][keep], before[key][keep], f"{case.name}: {key} of the envs that were not reset")
    g.call("mppi_sim_finish")
    S1 = g.get("mppi_get_costs", (K,))
    g.call("mppi_sim_finish")
    S2 = g.get("mppi_get_costs", (K,))
    g.close()
    ctrl = S2.astype(np.float64) - S1       # (the control-cost accumulator: mppi_sim_finish adds it once more)
    print(f"{case.name}: control cost of the envs that were not reset in [{ctrl[keep].min():.3g}, {ctrl[keep].max():.3g}], median size {np.median(np.abs(ctrl[keep])):.3g}")
    assert not S1[half].any() and not S2[half].any(), "cost accumulators of the reset envs"
    # S1 = fp32(S0 + ctrl), S2 = fp32(S1 + ctrl): two roundings at the size of S2; a control cost that shows is a hundred times that
    ulp = float(np.spacing(np.abs(S2[keep]).max().astype(np.float32)))
    assert (ctrl[keep] != 0).all() and np.median(np.abs(ctrl[keep])) > 100 * ulp, "the control cost of the other envs is there"
    np.testing.assert_allclose(S1[keep], S0[keep] + ctrl[keep], rtol=0, atol=2 * ulp, err_msg="cost accumulators of the other envs")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,K", [("panda", 65), ("boxer", 65)])
def test_sim_reset_restores_x0_after_a_scatter(scene, K, lib):
    case, b, g = context(lib, scene, K)
    _, dof, root = starts(scene)
    d_dof, d_root = dev(dof[:K]), dev(hidden(root[:K], b.m))
    g.call("mppi_sim_set_states", ptr(d_dof), ptr(d_root))
    d_u = dev(commands(case, b.cfg.nu))
    g.call("mppi_sim_step", ptr(d_u[0]), 0)
    g.call("mppi_sim_reset")
    got = Tensors(b.m, K).fill(g, "mppi_sim_materialise")
    g.close()
    assert_bits(got["dof"], np.tile(b.dof.reshape(1, -1), (K, 1)), "dof rows after mppi_sim_reset")
    assert_bits(got["root"], np.tile(b.root.reshape(1, b.m.n_actors, 13), (K, 1, 1)), "root rows after mppi_sim_reset")
    assert not got["cf"].any()


def test_planner_command_does_not_see_the_scatter(lib):
    """mppi_command rolls every sample out from x0: bit-equal costs and action on a context whose envs hold other states"""
    import types
    K = 65
    scene, m, cfg, cost, dof0, root0 = panda_reach(K=K, H=6)
    b = types.SimpleNamespace(m=m, cfg=cfg, cost=cost, dof=np.array(dof0, np.float32), root=np.array(root0, np.float32),
                              U0=np.zeros((6, cfg.nu), np.float32), prior=None)
    _, dof, root = starts("panda")
    out = []
    for scattered in (False, True):
        g = Gpu(lib, b, AUTO)
        if scattered:
            d_dof, d_root = dev(dof[:K]), dev(root[:K])
            g.call("mppi_sim_reset")
            g.call("mppi_sim_set_states", ptr(d_dof), ptr(d_root))
            d_u = dev(commands(scene_case("panda", K), cfg.nu))
            g.call("mppi_sim_step", ptr(d_u[0]), 0)
        action = np.zeros(cfg.nu, np.float32)
        g.call("mppi_command", capi.fptr(action))
        out.append((action, g.get("mppi_get_costs", (K,))))
        g.close()
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0]).max() > 0 and np.ptp(out[0][1]) > 0
    assert_bits(out[1][0], out[0][0], "action")
    assert_bits(out[1][1], out[0][1], "costs")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def wrapper(scene, K):
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    from mppiisaac.utils.config_store import load_config
    icfg = load_config({"defaults": [{"isaacgym": "normal"}]}).isaacgym
    actors, pos = {"panda": (["panda_stick", "goal"], [[0.0, 0.0, 0.0]]),
                   "boxer": (["boxer", "block", "paper_obst1", "paper_obst2", "goal"], [[0.0, 2.5, 0.05]])}[scene]
    return IsaacGymWrapper(icfg, actors=actors, init_positions=pos, num_envs=K, randomize_seed=-1)


def test_wrapper_sets_per_env_states_in_place(lib, oracle64):
    """the reference's idiom: edit `_dof_state` / `_root_state`, hand the tensor of all envs to the set call"""
    import torch
    K, scene = 17, "boxer"
    case = scene_case(scene, K)
    b, dof, root = starts(scene)
    sim = wrapper(scene, K)
    m = sim._c_model
    assert per_env_actors(m) == per_env_actors(b.m) == sim._per_env_actors()
    # x0 as the step matrix has it (on its wheels, the block in front): its broadcast is still pending when the set call comes and is
    # carried out first - a dof-only call leaves the roots at the new x0
    sim.set_state_from_env0(torch.from_numpy(b.dof[None]), torch.from_numpy(b.root.reshape(1, m.n_actors, 13)))
    assert sim._needs_reset
    sim.set_dof_state_tensor(dev(dof[K:2 * K]))
    assert not sim._needs_reset and sim._stale
    assert_bits(sim._root_state.cpu().numpy(), np.tile(b.root.reshape(1, m.n_actors, 13), (K, 1, 1)), "_root_state after a dof-only call")
    assert_bits(sim._dof_state.cpu().numpy(), dof[K:2 * K], "_dof_state after a dof-only call")
    # the in-place idiom: both tensors edited, then pushed
    sim._dof_state[:] = dev(dof[:K])
    for a in per_env_actors(m):
        sim._root_state[:, a] = dev(root[:K, a])
    sim.set_dof_state_tensor()
    sim.set_actor_root_state_tensor()
    assert sim._stale
    assert_bits(sim.get_dof_state().cpu().numpy(), dof[:K], "get_dof_state() after the set calls")
    assert_bits(sim._root_state.cpu().numpy(), root[:K], "_root_state after the set calls")
    assert not sim._net_contact_force.cpu().numpy().any()
    u = commands(case, b.cfg.nu)
    rows = []
    for t in range(case.N):
        sim.apply_robot_cmd(dev(u[t]))
        sim.step()
        rows.append({"dof": sim._dof_state, "root": sim._root_state, "rb": sim._rigid_body_state, "cf": sim._net_contact_force})
        rows[-1] = {k: v.cpu().numpy().copy() for k, v in rows[-1].items()}
    fails, _ = compare(f"wrapper {scene} K={K}", stacked(rows), reference(oracle64, scene, K), case.klass)
    assert not fails, "\n".join(fails)
    # explicit tensors (any float dtype, any device), indexed forms, reset_envs
    ids, dofm, rootm = [16, 0, 5], *starts(scene, SEED_OTHER)[1:]
    now = {k: getattr(sim, "_" + k).cpu().numpy().copy() for k in ("dof_state", "root_state")}
    sim.set_dof_state_tensor_indexed(torch.from_numpy(dofm[ids].astype(np.float64)), ids)
    sim.set_actor_root_state_tensor_indexed(rootm[ids], torch.tensor(ids, device="cuda"))
    rest = [k for k in range(K) if k not in ids]
    assert_bits(sim._dof_state.cpu().numpy()[ids], dofm[ids], "dof rows of the indexed envs")
    assert_bits(sim._root_state.cpu().numpy()[ids], rootm[ids], "root rows of the indexed envs")
    assert_bits(sim._dof_state.cpu().numpy()[rest], now["dof_state"][rest], "dof rows of the other envs")
    assert_bits(sim._root_state.cpu().numpy()[rest], now["root_state"][rest], "root rows of the other envs")
    sim.reset_envs([1, 16])
    assert_bits(sim._dof_state.cpu().numpy()[[1, 16]], np.tile(b.dof[None], (2, 1)), "dof rows after reset_envs")
    assert_bits(sim._root_state.cpu().numpy()[[1, 16]], np.tile(b.root.reshape(1, m.n_actors, 13), (2, 1, 1)), "root rows after reset_envs")
    assert_bits(sim._dof_state.cpu().numpy()[[0, 5]], dofm[[0, 5]], "dof rows of the envs that were not reset")
    # refusals
    obst = sim.scene.actor_index("paper_obst1")
    moved = torch.from_numpy(root[:K].copy())
    moved[3, obst, 0] += 0.5
    with pytest.raises(ValueError, match="paper_obst1.*set_actor_position_by_name"):
        sim.set_actor_root_state_tensor(moved)
    with pytest.raises(ValueError, match="shape"):
        sim.set_dof_state_tensor(torch.zeros(K, 2 * m.n_bodies + 1))
    with pytest.raises(ValueError, match="shape"):
        sim.set_actor_root_state_tensor_indexed(torch.zeros(2, m.n_actors, 13), [0, 1, 2])
    for bad in ([0, K], [-1]):
        with pytest.raises(ValueError, match="env ids"):
            sim.set_dof_state_tensor_indexed(torch.zeros(len(bad), 2 * m.n_bodies), bad)
        with pytest.raises(ValueError, match="env ids"):
            sim.reset_envs(bad)
    assert_bits(sim._dof_state.cpu().numpy()[[0, 5]], dofm[[0, 5]], "a refused call changes nothing")
    # the existing single-state setters still broadcast
    sim.set_actor_dof_state(torch.from_numpy(b.dof))
    assert_bits(sim._dof_state.cpu().numpy(), np.tile(b.dof[None], (K, 1)), "set_actor_dof_state broadcasts one state")
    sim.stop_sim()


def test_wrapper_on_a_fixed_base_scene_and_the_single_env_world(lib):
    """contact-free scene: every root row is shared (a changed one is refused, the robot's included); K = 1: the host mirror of the
    state tensors follows a set call as it follows a step"""
    import torch
    from mppiisaac.utils.transport import torch_to_bytes, bytes_to_torch
    K = 17
    _, dof, root = starts("panda")
    sim = wrapper("panda", K)
    assert sim._per_env_actors() == []
    sim.set_dof_state_tensor(dof[:K])
    assert_bits(sim.get_dof_state().cpu().numpy(), dof[:K], "get_dof_state() after set_dof_state_tensor")
    sim.set_actor_root_state_tensor()            # (the wrapper's own rows: the shared state)
    moved = sim._root_state.clone()
    moved[2, sim.scene.robot_idx, 1] += 0.1
    with pytest.raises(ValueError, match="panda.*set_actor_position_by_name"):
        sim.set_actor_root_state_tensor(moved)
    sim.stop_sim()
    world = wrapper("panda", 1)
    before = bytes_to_torch(torch_to_bytes(world._dof_state)).cpu().numpy().copy()
    world._dof_state[0] = dev(dof[3])
    world.set_dof_state_tensor()
    assert_bits(bytes_to_torch(torch_to_bytes(world._dof_state)).cpu().numpy(), dof[3:4], "the K = 1 state blob after a set call")
    assert (before != dof[3:4]).any()
    world.stop_sim()
