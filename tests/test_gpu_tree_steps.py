"""The env-step kernels (k_sim_step `lane`, k_sim_step_quad `quad`), k_materialise and the trajectory dump with its materialise
kernels on the branching and mixed trees of tests/test_gpu_tree_matrix.py (TREES there), against the fp64 oracle's batched env step
(orc_envs_step) PER ENV, EVERY ENV, EVERY STEP, EVERY COLUMN of the four reference-layout tensors - the rb rows of both fingers and
of the links past index 8 among them.  The machinery is that of tests/test_gpu_step_matrix.py, which runs the 7-body chain and the
point robot only.

STEP CASES per tree: K = 1 (`quad`, and `lane` under MPPI_WORLD_STEP=lane), K = 17 (`lane`), K = 65 (`quad`); the kernel is asserted
by name.  N = 6 steps with commands drawn per (step, env, column) from the seeded generator of the step matrix (within the -+0.5
of the tree matrix; the effort trees reach their torques through cmd_coef), mppi_sim_materialise after every step.
TRAJECTORY CASES per tree: K = 17 and 65, under the default rollout kernel and under MPPI_ROLLOUT=quad: mppi_rollout_trajectory +
mppi_materialise_trajectory, all H * K rows of the four tensors.  The dump forms its controls itself (nominal + noise, clamped), so
its reference is the oracle stepped with U + du of the noise the device sampled (checked against oracle.sample at 1e-6; du against
the clamp formula at 1e-6).  mppi_materialise_trajectory_link is called twice per case - on the branching trees for a finger and for
a link of index >= 8 - and must give the rb rows of that link bit for bit.

TOLERANCES: the rule of the step matrix for its `free` class, per tree - 10 x the worst deviation of the fp32 oracle from the fp64
one over the tree's cases (ORACLE32, re-measured and printed by test_tree_step_cases_are_well_posed), rounded up to 1-2-5, never
above CAP["free"] of the step matrix (q 1e-5, qd 2e-4, pos 2e-5).

test_tree_step_cases_are_well_posed (no GPU): everything finite, the fp32 oracle within a tenth of every tolerance, every env told
apart from its neighbour and from env 0 by more than 100 x a tolerance, the drive mode changes the result (the same commands under
another drive mode end elsewhere in more than half the envs), the two fingers end apart by more than 100 x the position tolerance
in at least half the envs.
test_host_build_steps_match_the_oracle_per_env: the same commands through emu_step + emu_rigid_body_state of tests/hostemu (the
one-lane device routines of every tree compiled for the CPU) at the same tolerances."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from mppiisaac.backend import capi
from test_gpu_rollout_matrix import AUTO, QUAD, Gpu
from test_gpu_step_matrix import CAP, DU_TOL, KEYS, Case, Tensors, commands, compare, deviations, differs_in, horizon_controls, lib  # noqa: F401
from test_gpu_step_matrix import open_context, oracle_steps, round_up_125, stacked, told_apart
from test_gpu_tree_matrix import MAKE, TREES, UMAX

N, KG = 6, 65                      # steps of every case; the K at which the oracle runs once per tree (envs are independent)
# the two links of mppi_materialise_trajectory_link: (owner or "" for the scene's robot, link)
LINKS = {"panda_gripper": (("", "panda_rightfinger"), ("", "panda_ee")), "panda_gripper_pos": (("", "panda_leftfinger"), ("", "panda_hand")),
         "omnipanda": (("", "panda_leftfinger"), ("", "panda_link5")), "omnipanda_effort": (("", "panda_rightfinger"), ("", "panda_link7")),
         "heijn": (("", "front_link"), ("", "base_link")), "panda_effort": (("", "panda_link7"), ("", "panda_link4")),
         "point_forest": (("point_robot2", "base_link"), ("point_robot", "base_link"))}

STEP_CASES, TRAJ_CASES = [], []
for _t in TREES:
    STEP_CASES += [Case(f"{_t}-K1", _t, 1, "quad", N=N), Case(f"{_t}-K1-world-lane", _t, 1, "lane", N=N, env=(("MPPI_WORLD_STEP", "lane"),)),
                   Case(f"{_t}-K17", _t, 17, "lane", N=N), Case(f"{_t}-K65", _t, 65, "quad", N=N)]
    for _K in (17, 65):
        TRAJ_CASES += [Case(f"{_t}-dump-K{_K}", _t, _K, "", route="horizon", N=N), Case(f"{_t}-dump-K{_K}-quad", _t, _K, "", route="horizon", N=N, env=(("MPPI_ROLLOUT", QUAD),))]
STEP_IDS, TRAJ_IDS = [c.name for c in STEP_CASES], [c.name for c in TRAJ_CASES]

# worst fp32-against-fp64 oracle deviation per tree over its step and trajectory cases (printed by the well-posedness test)
ORACLE32 = {
    "panda_gripper": {"q": 8.05e-07, "qd": 3.36e-07, "pos": 4.69e-07, "quat": 4.40e-07, "lin": 3.17e-07, "ang": 5.49e-07, "cf": 0.0},
    "panda_gripper_pos": {"q": 6.11e-08, "qd": 1.25e-06, "pos": 2.08e-07, "quat": 1.54e-07, "lin": 1.01e-06, "ang": 1.55e-06, "cf": 0.0},
    "omnipanda": {"q": 6.18e-07, "qd": 1.76e-07, "pos": 3.28e-07, "quat": 3.46e-07, "lin": 4.70e-07, "ang": 5.03e-07, "cf": 0.0},
    "omnipanda_effort": {"q": 6.48e-07, "qd": 3.42e-07, "pos": 4.30e-07, "quat": 4.78e-07, "lin": 4.07e-07, "ang": 9.17e-07, "cf": 0.0},
    "heijn": {"q": 1.65e-08, "qd": 4.77e-08, "pos": 4.05e-08, "quat": 5.09e-08, "lin": 9.86e-08, "ang": 4.77e-08, "cf": 0.0},
    "panda_effort": {"q": 8.40e-07, "qd": 1.68e-05, "pos": 3.68e-07, "quat": 4.93e-07, "lin": 7.42e-06, "ang": 1.66e-05, "cf": 0.0},
    "point_forest": {"q": 1.70e-08, "qd": 7.15e-08, "pos": 1.17e-07, "quat": 4.98e-08, "lin": 8.29e-08, "ang": 3.67e-08, "cf": 0.0},
}
# -> e.g. panda_gripper: q 1e-5  qd 5e-6  pos 5e-6  quat 5e-6  lin 5e-6  ang 1e-5  cf 0 (exact zeros);
#         panda_effort (the damper is 10, not 600: velocities answer the torque rounding): qd 2e-4  lin 1e-4  ang 2e-4;
#         heijn: q 2e-7  qd 5e-7  pos 5e-7.  No cap binds (q of three trees and qd of panda_effort land ON theirs).
TOL = {t: {k: min(round_up_125(10.0 * v), CAP["free"].get(k, np.inf)) for k, v in d.items()} for t, d in ORACLE32.items()}


def build(case):
    """-> what Gpu() of the rollout matrix takes (m, cfg, cost = None, dof, root, U0, prior) and the scene"""
    scene, m, cfg, _, dof, root = MAKE[case.scene](K=case.K, H=N)
    U0 = np.zeros((N, cfg.nu), np.float32)
    if case.route == "horizon":
        U0 = (0.05 * UMAX * np.random.default_rng(0).normal(size=(N, cfg.nu))).astype(np.float32)
        if TREES[case.scene].finger_u0:
            U0[:, -2:] += np.float32(TREES[case.scene].finger_u0)
    return types.SimpleNamespace(case=case, scene=scene, m=m, cfg=cfg, cost=None, dof=np.array(dof, np.float32), root=np.array(root, np.float32), U0=U0, prior=None)


_REFS = {}


def reference(o, case, b):
    """the oracle's states of a step case: one run per tree at K = 65 (env k of a smaller case is env k of that run), kept unchanged"""
    key = (o.dtype, case.scene)
    if key not in _REFS:
        big = dataclasses.replace(case, K=KG)
        _REFS[key] = oracle_steps(o, build(big), commands(big, b.m.nu, KG), 0)
        for v in _REFS[key].values():
            v.setflags(write=False)
    return {k: v[:, :case.K] for k, v in _REFS[key].items()}


def other_drive(m):
    """the same model under another drive mode, at the gains the shipped robots of that mode have"""
    if m.drive_mode == capi.DRIVE_VELOCITY:
        m.drive_mode, m.drive_kp, m.drive_kd = capi.DRIVE_EFFORT, 0.0, 10.0
    else:
        m.drive_mode, m.drive_kp, m.drive_kd = capi.DRIVE_VELOCITY, 0.0, 600.0
    return m


def finger_rows(b):
    return [b.scene.rigid_body_index(b.scene.robot.name, f) for f in TREES[b.case.scene].fingers]


# ---- the conditions on the inputs, on the oracle alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES + TRAJ_CASES, ids=STEP_IDS + TRAJ_IDS)
def test_tree_step_cases_are_well_posed(case, oracle64, oracle32):
    assert (STEP_IDS + TRAJ_IDS).count(case.name) == 1 and case.N == N and case.K <= KG
    b, tol = build(case), TOL[case.scene]
    assert not oracle64.is_scene(b.m)
    if case.route == "horizon":
        du, u, clamped = horizon_controls(b, oracle64.sample(b.cfg))
        print(f"{case.name}: {100 * clamped:.1f} % of the controls at the clamp")
        assert 0.01 <= clamped <= 0.80 and np.abs(b.U0).min() > 0
        r64, r32 = oracle_steps(oracle64, b, u, 0), oracle_steps(oracle32, b, u, 0)
    else:
        u = commands(case, b.m.nu)
        r64, r32 = reference(oracle64, case, b), reference(oracle32, case, b)
    assert all(np.isfinite(v).all() for v in r64.values()) and all(np.isfinite(v).all() for v in r32.values())
    dev = deviations(r32, r64)
    print(f"{case.name}: fp32 oracle vs fp64 oracle: " + " | ".join(f"{k} {dev[k].max():.2e} (tol/10 {tol[k] / 10:.0e})" for k in KEYS))
    for k in KEYS:
        assert dev[k].max() <= tol[k] / 10.0, f"{k}: the fp32 oracle leaves the fp64 one by more than a tenth of the tolerance"
    for k in range(1, case.K):
        assert told_apart(r64, tol, k, k - 1) and told_apart(r64, tol, k, 0), f"env {k} is not told apart from env {k - 1} / env 0"
    other = build(case)
    other_drive(other.m)
    frac = differs_in(r64, oracle_steps(oracle64, other, u, 0), tol)
    print(f"{case.name}: differs from the same tree under another drive mode in {100 * frac:.0f} % of the envs")
    assert frac > 0.5
    if TREES[case.scene].fingers and case.K > 1:
        f0, f1 = finger_rows(b)
        apart = np.mean(np.abs(r64["rb"][-1, :, f0, 0:3] - r64["rb"][-1, :, f1, 0:3]).max(axis=1) > 100.0 * tol["pos"])
        print(f"{case.name}: after the last step the fingers are more than 100 x {tol['pos']:.0e} apart in {100 * apart:.0f} % of the envs")
        assert apart >= 0.5


# ---- the host build of the device routines -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", sorted(TREES))
def test_host_build_steps_match_the_oracle_per_env(tree, hostemu, oracle64):
    """emu_step (cmd_map + step of csrc/mppi_device.hpp) and emu_rigid_body_state for the 65 envs of the tree's largest step case"""
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    case = next(c for c in STEP_CASES if c.scene == tree and c.K == KG)
    b = build(case)
    u, want, m = commands(case, b.m.nu), reference(oracle64, case, b), b.m
    n, root = m.n_bodies, f32(b.root)
    got = {k: np.zeros(v.shape) for k, v in want.items()}
    for k in range(case.K):
        q, qd = f32(b.dof[0::2]).copy(), f32(b.dof[1::2]).copy()
        for t in range(N):
            assert hostemu.emu_step(C.byref(m), fp(root), fp(q), fp(qd), fp(f32(u[t, k]))) == 0
            rb, cf = np.zeros((m.n_rb, 13), np.float32), np.ones((m.n_rb, 3), np.float32)
            assert hostemu.emu_rigid_body_state(C.byref(m), fp(root), fp(q), fp(qd), fp(rb), fp(cf)) == 0
            got["dof"][t, k, 0::2], got["dof"][t, k, 1::2], got["root"][t, k], got["rb"][t, k], got["cf"][t, k] = q, qd, root, rb, cf
    fails, _ = compare(f"{tree} host build, K={case.K}", got, want, TOL[tree])
    assert not got["cf"].any() and not fails, "\n".join(fails)


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_tree_step_kernels_match_the_oracle_per_env(case, lib, oracle64):
    import torch
    b = build(case)
    g = open_context(lib, case, b)                           # (asserts ` step=<name> `)
    T = Tensors(b.m, case.K)
    dev_u = torch.from_numpy(commands(case, b.cfg.nu)).cuda().contiguous()
    g.call("mppi_sim_reset")
    rows = []
    for t in range(N):
        g.call("mppi_sim_step", C.c_void_p(dev_u[t].data_ptr()), 0)
        rows.append(T.fill(g, "mppi_sim_materialise"))
    g.close()
    got = stacked(rows)
    fails, _ = compare(f"{case.name} K={case.K} step={case.step}", got, reference(oracle64, case, b), TOL[case.scene])
    assert not got["cf"].any(), "contact forces of a contact-free scene"
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TRAJ_CASES, ids=TRAJ_IDS)
def test_tree_trajectory_dump_matches_the_oracle_per_row(case, lib, oracle64):
    import torch
    b = build(case)
    K, m, kernel = case.K, b.m, dict(case.env).get("MPPI_ROLLOUT", AUTO)
    g = Gpu(lib, b, kernel)
    assert f"rollout={'quad' if kernel == QUAD else 'oct-pair'} " in g.info, g.info
    np.testing.assert_allclose(g.eps, oracle64.sample(b.cfg), atol=1e-6)
    du, u, _ = horizon_controls(b, g.eps)
    want = oracle_steps(oracle64, b, u, 0)
    g.call("mppi_rollout_trajectory")
    T = Tensors(m, N * K)
    got = {k: v.reshape((N, K) + v.shape[1:]).astype(np.float64) for k, v in T.fill(g, "mppi_materialise_trajectory").items()}
    tag = f"{case.name} K={K} rollout={kernel} trajectory dump"
    fails, _ = compare(tag, got, want, TOL[case.scene])
    du_dev = g.get("mppi_get_perturbations", (N, b.cfg.nu, K))
    print(f"{tag}: du {np.abs(du_dev - du).max():.1e} ({DU_TOL:.0e})")
    fails += [f"{tag}: du"] * (not np.abs(du_dev - du).max() <= DU_TOL)
    assert not got["cf"].any(), "contact forces of a contact-free scene"
    rb = T.t["rb"].cpu().numpy()
    for owner, name in LINKS[case.scene]:                    # the rows of one link alone are the rb rows of that link, bit for bit
        link = b.scene.rigid_body_index(owner or b.scene.robot.name, name)
        out = torch.full((N * K, 13), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g.call("mppi_materialise_trajectory_link", link, C.c_void_p(out.data_ptr()))
        g.call("mppi_synchronize")
        np.testing.assert_array_equal(out.cpu().numpy(), rb[:, link, :], err_msg=f"{tag}: rows of {name}")
    g.close()
    assert not fails, "\n".join(fails)
