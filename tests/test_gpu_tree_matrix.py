"""The contact-free rollout kernels of the branching and mixed kinematic trees - `lane`, `quad`, `oct`, `oct-pair` and whatever
mppi_create selects by itself, one generated topo_<i>.hip unit per tree - against the fp64 oracle PER SAMPLE, EVERY SAMPLE, with the
machinery of tests/test_gpu_rollout_matrix.py (which runs the 7-body chain and the 3-body point robot only).

TREES
  panda_gripper        [-1,0,1,2,3,4,5,6,6]: two prismatic fingers on one hand (a branch), velocity drive
  panda_gripper_pos    the same tree under dof_mode "position" (teleport, then the stiffness drive)
  omnipanda            [-1,0,..,8,9,9]: prismatic x, prismatic y, revolute base, the arm, the branch at body 9 - 12 bodies, more than
                       an octet has lanes, 12 commands, the only shipped unit compiled with MPPI_DPP_LEAD_WAIT
  omnipanda_effort     the same tree under the effort drive
  heijn                prismatic, prismatic, revolute; the cost link (front_link) is not the last body's own link
  panda_effort         the 7-body chain under the effort drive
  point_forest         [-1,0,1,-1,3,4]: two point robots in one env.  mppi_create (csrc/mppi_hip.hip) takes the contact-free
                       branch whenever the model has no candidate pair (is_scene); with the robot-against-robot pairs switched off
                       (Scene.ROBOT_ROBOT_PAIRS, what MPPI_ROBOT_ROBOT_PAIRS=0 sets) the two fixed-base robots leave none, so the
                       forest's contact-free instantiation runs and is included; its cost link belongs to the SECOND robot.
Every tree gets a `goal` actor and the reach cost of test_more_robots_rollout on the link that test uses; the visualised link is
never the cost link - a finger (body index >= 8 on the 12-body tree) on the branching trees.

SHAPES per tree, the smallest that reach every path: (K, H) = (9, 3) one octet in the second owner wavefront, (17, 12) a second
workgroup with a dead owner, (65, 12) a ragged fifth workgroup, (33, 32) the full 32-row control table of the helper kernel;
(17, 12) with use_priors + sample_null_action and a prior sequence; 33 samples as shards of 16 + 17 combined by mppi_update.
Every case runs all five kernels; each is asserted by name and wavefront count, `oct` and `oct-pair` are compared for EQUALITY.

INPUTS.  Controls within -+0.5, noise_sigma = u_max^2 I, a nominal of 0.05 u_max N(0, 1) (seed 0), lambda_ = 2.  The limit is 0.5
on every tree because the project's bound on du, 1e-6, is absolute and the fp32 oracle must stay within a tenth of it: fp32 holds
U + eps to 3e-8 below 1 and to 2e-6 at the 40 N m of panda_effort.  The effort trees reach their torques through the command map
instead (cmd_coef = twice the u_max of test_more_robots_rollout: -+0.5 commands -+40 N m / -+10 N m) - which also takes these
trees through the general map.  Position-driven fingers get a nominal opening of 0.1 on top (with a nominal around zero both
fingers are teleported onto their closed stop in half the samples and coincide) and lambda_ = 0.5, which keeps the control-cost
term of that nominal from pulling costs across zero.

TOLERANCES come from the oracle and the project, never from the kernels: per tree and per quantity 10 x the worst deviation of
Oracle("f32") from Oracle("f64") over the tree's cases (ORACLE32 below, re-measured and printed by test_tree_cases_are_well_posed;
test_oracle32_table_gives_the_measured_tolerances fails when the table has gone stale), rounded up to the next 1-2-5 value, never
above what the suite already asserts: S 1e-4 relative, du 1e-6, visualisation rows 1e-4, U and action 1e-3 |u_max|, (beta, eta) 2e-3.

test_tree_cases_are_well_posed (no GPU) asserts the conditions of test_matrix_cases_are_well_posed with the fp32 oracle within a
tenth of EVERY tolerance, and on the branching trees that the two fingers receive different commands (by more than 100 x the
du tolerance in at least half the entries) and end apart in space by more than 100 x the visualisation tolerance in at least half
the samples (a swap of the siblings cannot pass).  It prints per case how many joint-steps of the fp64 rollout end on a joint stop, at vmax, or in the effort-saturated second
solve (information, not a condition).

test_host_build_matches_the_oracle_per_sample runs the same cases through tests/hostemu (the `lane` and `quad` arithmetic of every
tree compiled for the CPU) at the same tolerances; profiles/r16a_planted_defects.txt records which of its rows catch four defects
planted in scratch copies of the shared device code."""
import ctypes as C
import dataclasses
import os
import tempfile

import numpy as np
import pytest

import lane_scalar_cases as L
from mppiisaac.backend import capi
from scenes import build_scene
from test_gpu_rollout_matrix import AUTO, FOUR, OCT, PAIR, PRIOR, Case, build, compare, device, run_gpu, run_oracle  # noqa: F401
from test_gpu_step_matrix import round_up_125

CAP = {"S": 1e-4, "du": 1e-6, "viz": 1e-4, "U": 1e-3, "action": 1e-3, "beta_eta": 2e-3}     # (U, action: times |u_max|)
QUANTITIES = tuple(CAP)
UMAX = 0.5


@dataclasses.dataclass(frozen=True)
class Tree:
    actors: tuple
    link: str                    # cost link (tests/test_gpu_parity.py test_more_robots_rollout)
    viz: str                     # visualised link
    over: tuple = ()             # robot overrides
    gain: float = 1.0            # cmd_coef of every body
    fingers: tuple = ()          # link names of the two siblings (the last two bodies)
    finger_u0: float = 0.0       # added to the siblings' columns of the nominal
    lambda_: float = 2.0
    forest: bool = False


FINGERS = ("panda_leftfinger", "panda_rightfinger")
TREES = {
    "panda_gripper": Tree(("panda_gripper", "goal"), "panda_hand", "panda_rightfinger", fingers=FINGERS),
    "panda_gripper_pos": Tree(("panda_gripper", "goal"), "panda_hand", "panda_leftfinger", over=(("dof_mode", "position"),),
                              fingers=FINGERS, finger_u0=0.1, lambda_=0.5),
    "omnipanda": Tree(("omnipanda", "goal"), "panda_hand", "panda_leftfinger", fingers=FINGERS),
    "omnipanda_effort": Tree(("omnipanda_effort", "goal"), "panda_hand", "panda_rightfinger", gain=20.0, fingers=FINGERS),
    "heijn": Tree(("heijn", "goal"), "front_link", "base_link"),
    "panda_effort": Tree(("panda_effort", "goal"), "panda_link7", "panda_link4", gain=80.0),
    "point_forest": Tree(("point_robot", "point_robot2", "goal"), "base_link", "base_link", forest=True),
}


def forest_scene():
    """two point robots in one env with the robot-against-robot pairs off: no candidate pair is left, the scene is contact-free"""
    import yaml
    from mppiisaac.planner.isaacgym_wrapper import Scene
    with tempfile.TemporaryDirectory() as d:
        second = os.path.join(d, "point_robot2.yaml")
        with open(second, "w") as f:
            yaml.safe_dump({"type": "robot", "name": "point_robot2", "fixed": True, "urdf_file": "point_robot.urdf"}, f)
        old, Scene.ROBOT_ROBOT_PAIRS = Scene.ROBOT_ROBOT_PAIRS, False
        try:
            return build_scene(["point_robot", second, "goal"], [[0.0, 0.0, 0.05], [1.0, -0.5, 0.05]])
        finally:
            Scene.ROBOT_ROBOT_PAIRS = old


def tree_reach(name):
    """-> make(K, H, **mppi_over) as scenes.panda_reach: scene, model, config, cost, dof, root of the tree's reach task"""
    tree = TREES[name]

    def make(K=64, H=12, **mppi_over):
        from mppiisaac.planner.mppi import MPPIConfig, make_config
        scene = forest_scene() if tree.forest else build_scene(list(tree.actors), [[0.0, 0.0, 0.0]], robot_overrides=dict(tree.over) or None)
        m = scene.to_c()
        nu = scene.nu
        for i in range(m.n_bodies):
            m.cmd_coef[i][0] *= tree.gain
        kw = dict(num_samples=K, horizon=H, noise_sigma=(UMAX * UMAX * np.eye(nu)).tolist(), lambda_=tree.lambda_, u_min=[-UMAX], u_max=[UMAX],
                  sample_null_action=True)
        kw.update(mppi_over)
        cfg = make_config(MPPIConfig(**kw), viz_link=scene.viz_link_index())
        cost = capi.Cost()
        cost.kind = capi.COST_PANDA_REACH
        # (the forest: the base of the SECOND robot, so that the second tree and its three commands carry the cost)
        cost.link[0] = scene.rigid_body_index("point_robot2" if tree.forest else scene.robot.name, tree.link)
        cost.actor[0] = scene.actor_index("goal")
        cost.w[0], cost.w[1] = 1.0, 0.1
        dof, root = scene.initial_state()
        root[scene.actor_index("goal"), 0:3] = [0.6, 0.3, 0.5]
        return scene, m, cfg, cost, dof, root
    make.__name__ = f"tree_reach_{name}"
    return make


MAKE = {name: tree_reach(name) for name in TREES}
FIVE = FOUR + (AUTO,)
CASES = []
for _name, _tree in TREES.items():
    _kw = dict(viz=_tree.viz, u0=0.05)
    for _K, _H in ((9, 3), (17, 12), (65, 12), (33, 32)):
        CASES.append(Case(f"{_name}-K{_K}-H{_H}", MAKE[_name], _K, _H, FIVE, **_kw))
    CASES.append(Case(f"{_name}-prior-K17-H12", MAKE[_name], 17, 12, FIVE, prior=True, over=tuple(sorted(PRIOR["over"].items())), **_kw))
    CASES.append(Case(f"{_name}-shards16+17-H12", MAKE[_name], 33, 12, FIVE, shards=(16, 17), **_kw))
IDS = [c.name for c in CASES]


def tree_of(case):
    return next(n for n in sorted(TREES, key=len, reverse=True) if case.name.startswith(n + "-"))


def build_tree(case, cus):
    """build() of the rollout matrix; the nominal of position-driven fingers is an opening within their range, not zero"""
    b, tree = build(case, cus), TREES[tree_of(case)]
    if tree.finger_u0:
        b.U0[:, [b.m.cmd_col[b.m.n_bodies - 2][0], b.m.cmd_col[b.m.n_bodies - 1][0]]] += np.float32(tree.finger_u0)
    return b


# worst deviation of Oracle("f32") from Oracle("f64") per tree over its six cases (S, beta_eta relative; U, action in units of |u_max|)
ORACLE32 = {
    "panda_gripper": {"S": 5.51e-07, "du": 4.46e-08, "viz": 7.59e-07, "U": 3.28e-07, "action": 3.25e-07, "beta_eta": 7.31e-07},
    "panda_gripper_pos": {"S": 5.06e-07, "du": 4.46e-08, "viz": 2.11e-07, "U": 8.73e-07, "action": 9.26e-07, "beta_eta": 1.85e-06},
    "omnipanda": {"S": 8.43e-07, "du": 4.46e-08, "viz": 8.51e-07, "U": 4.01e-07, "action": 2.69e-07, "beta_eta": 4.74e-07},
    "omnipanda_effort": {"S": 7.12e-07, "du": 4.46e-08, "viz": 7.04e-07, "U": 4.73e-07, "action": 4.92e-07, "beta_eta": 5.75e-07},
    "heijn": {"S": 3.86e-07, "du": 4.46e-08, "viz": 5.41e-07, "U": 1.35e-07, "action": 1.65e-07, "beta_eta": 5.08e-07},
    "panda_effort": {"S": 6.66e-07, "du": 4.44e-08, "viz": 3.28e-07, "U": 2.82e-07, "action": 2.08e-07, "beta_eta": 4.20e-07},
    "point_forest": {"S": 3.39e-07, "du": 4.43e-08, "viz": 1.17e-07, "U": 4.55e-07, "action": 3.72e-07, "beta_eta": 8.98e-07},
}
# -> TOL  S 1e-5 (heijn, point_forest 5e-6) | du 5e-7 | viz 1e-5 (panda_gripper_pos, panda_effort 5e-6; point_forest 2e-6)
#         U, action 5e-6 |u_max| (panda_gripper_pos 1e-5, heijn 2e-6) | (beta, eta) 1e-5 (panda_gripper_pos 2e-5; omnipanda,
#         panda_effort 5e-6): no cap binds
TOL = {t: {k: min(round_up_125(10.0 * v), CAP[k]) for k, v in d.items()} for t, d in ORACLE32.items()}


# ---- the conditions on the inputs, on the oracle alone -----------------------------------------------------------------------------
def oracle_deviation(a, c, umax):
    """per quantity the worst deviation of run c from run a, in the units compare() asserts in"""
    out = {}
    for key in QUANTITIES:
        x, y = np.asarray(a[key], np.float64), np.asarray(c[key], np.float64)
        out[key] = float(np.max(np.abs(y - x) / np.abs(x)) if key in ("S", "beta_eta") else np.max(np.abs(y - x)) / (umax if key in ("U", "action") else 1.0))
    return out


_MEASURED = {}


def measured(case, oracle64, oracle32):
    """(inputs, noise, fp64 outputs, fp32-oracle deviations) of a case, computed once"""
    if case.name not in _MEASURED:
        b = build_tree(case, 256)
        eps = oracle64.sample(b.cfg)
        o64, o32 = run_oracle(oracle64, b, eps), run_oracle(oracle32, b, eps)
        assert len(o64) == 1
        _MEASURED[case.name] = (b, eps, o64[0], oracle_deviation(o64[0], o32[0], b.umax))
    return _MEASURED[case.name]


def link_positions(o, b, q, names):
    """world positions [K][3] of the links `names` at the joint positions q [n][K]"""
    rows = [b.scene.rigid_body_index(b.scene.robot.name, n) for n in names]
    out = np.zeros((len(names), q.shape[1], 3))
    for k in range(q.shape[1]):
        rb, _ = o.rigid_body_state(b.m, b.root, q[:, k], np.zeros(q.shape[0]))
        out[:, k] = rb[rows, 0:3]
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tree_cases_are_well_posed(case, oracle64, oracle32):
    assert IDS.count(case.name) == 1
    name = tree_of(case)
    tree, tol = TREES[name], TOL[name]
    b, eps, a, dev = measured(case, oracle64, oracle32)
    cfg, K, m = b.cfg, b.cfg.num_samples, b.m
    assert not oracle64.is_scene(m) and b.umax == UMAX and cfg.want_rollouts and cfg.viz_link != b.cost.link[0]
    assert not case.shards or sum(case.shards) == K
    S, eta = a["S"], a["beta_eta"][1]
    assert np.isfinite(S).all() and ((S > 0).all() or (S < 0).all()), "costs finite and of one sign"
    print(f"{case.name}: S in [{S.min():.3f}, {S.max():.3f}], eta {eta:.3f}, the heaviest sample has {1.0 / eta:.2f} of the weight at most")
    print(f"{case.name}: fp32 oracle vs fp64 oracle: " + " | ".join(f"{k} {dev[k]:.2e} (tol/10 {tol[k] / 10:.0e})" for k in QUANTITIES))
    for k in QUANTITIES:
        assert dev[k] <= tol[k] / 10.0, f"{k}: the fp32 oracle leaves the fp64 one by more than a tenth of the tolerance"
    assert 1.0 / eta <= 0.9, "one sample carries more than 0.9 of the weight: the update hides the row sums"
    assert np.abs(b.U0).min() > 0
    lo, hi = np.array([cfg.u_min[j] for j in range(cfg.nu)]), np.array([cfg.u_max[j] for j in range(cfg.nu)])
    u = b.U0[:, :, None].astype(np.float64) + a["du"]              # the controls the samples apply
    clamped = np.mean((u == hi[None, :, None]) | (u == lo[None, :, None]))
    print(f"{case.name}: {100 * clamped:.1f} % of the controls on the clamp")
    assert 0.01 <= clamped <= 0.80
    if case.prior:
        assert cfg.use_priors and cfg.sample_null_action
        far = lambda d: np.abs(d).max(axis=1).min() > 0.05 * b.umax
        assert far(b.prior) and far(b.prior - b.U0) and far(np.diff(b.prior, axis=0))
        np.testing.assert_allclose(a["du"][:, :, K - 2], np.clip(b.prior, lo, hi) - b.U0, atol=1e-12)
        np.testing.assert_allclose(a["du"][:, :, K - 1], np.clip(0.0, lo, hi) - b.U0, atol=1e-12)
    # the paths of the fp64 rollout: joint-steps that end on a stop / at vmax, substeps that take the saturated second solve
    q, qd, logs = L.oracle_paths(oracle64, m, cfg, b.cost, b.dof, b.root, b.U0, eps, prior=b.prior)
    stops, vmax = L.path_counts(m, q, qd)
    sat = sum(bin(int(w)).count("1") for w in logs.ravel())
    print(f"{case.name}: of {q.size} joint-steps {stops} end on a joint stop, {vmax} at vmax; {sat} joint-substeps of {logs.size * m.n_bodies} "
          f"in the effort-saturated second solve")
    if tree.fingers:
        # the siblings: different commands, and apart at the end of the rollout - a swap of the two cannot pass
        f0, f1 = m.n_bodies - 2, m.n_bodies - 1
        assert m.bodies[f0].parent == m.bodies[f1].parent and m.bodies[f0].jtype == m.bodies[f1].jtype
        c0, c1 = m.cmd_col[f0][0], m.cmd_col[f1][0]
        assert c0 != c1
        differ = np.mean(np.abs(u[:, c0, :] - u[:, c1, :]) > 100.0 * tol["du"])
        pos = link_positions(oracle64, b, q[-1], tree.fingers)
        apart_q = np.mean(np.abs(q[-1, f0] - q[-1, f1]) > 100.0 * tol["viz"])
        apart_x = np.mean(np.abs(pos[0] - pos[1]).max(axis=1) > 100.0 * tol["viz"])
        print(f"{case.name}: the fingers' commands differ by more than 100 x {tol['du']:.0e} in {100 * differ:.0f} % of the (step, sample) entries; after the last step their joint "
              f"positions differ by more than 100 x {tol['viz']:.0e} in {100 * apart_q:.0f} % of the samples, their link positions in {100 * apart_x:.0f} %")
        assert differ >= 0.5 and apart_x >= 0.5


def test_oracle32_table_gives_the_measured_tolerances(oracle64, oracle32):
    """ORACLE32 is what the oracle gives today: the tolerance that follows from the re-measured deviations is the table's"""
    for name in TREES:
        worst = {k: max(measured(c, oracle64, oracle32)[3][k] for c in CASES if tree_of(c) == name) for k in QUANTITIES}
        print(f'    "{name}": {{' + ", ".join(f'"{k}": {v:.2e}' for k, v in worst.items()) + "},")
        for k in QUANTITIES:
            assert min(round_up_125(10.0 * worst[k]), CAP[k]) == TOL[name][k], (name, k, worst[k], TOL[name][k])
    print("tolerances: " + "; ".join(f"{n}: " + " ".join(f"{k} {v:.0e}" for k, v in TOL[n].items()) for n in TREES))


# ---- the host build of the device routines (tests/hostemu): `lane` and `quad` arithmetic of every tree, on the CPU --------------------
def emu(lib, which, b, eps):
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float)) if x is not None else None
    cfg = b.cfg
    S, du = np.zeros(cfg.num_samples, np.float32), np.zeros(eps.shape, np.float32)
    viz = np.zeros((cfg.horizon, cfg.num_samples, 3), np.float32)
    prior = f32(b.prior) if b.prior is not None else None
    rc = getattr(lib, which)(C.byref(b.m), C.byref(cfg), C.byref(b.cost), fp(f32(b.dof)), fp(f32(b.root)), fp(f32(b.U0)), fp(f32(eps)), fp(prior),
                             fp(S), fp(du), fp(viz))
    assert rc == 0, (which, rc)
    return {"S": S, "du": du, "viz": viz}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_build_matches_the_oracle_per_sample(case, hostemu, oracle64, oracle32):
    """emu_rollout (one lane per sample) and emu_rollout_quad (a 4-lane quad per sample; NaN marks lanes that disagree) on the
    oracle's own noise: S, du and the visualisation rows of every sample at the tolerances of the GPU test"""
    name = tree_of(case)
    b, eps, a, _ = measured(case, oracle64, oracle32)
    want = dict(a, U=None, action=None, beta_eta=None)
    fails = []
    for which in ("emu_rollout", "emu_rollout_quad"):
        fails += compare(f"{case.name} host build {which}", emu(hostemu, which, b, eps.astype(np.float32)), want, b.umax, TOL[name])
    assert not fails, "\n".join(fails)


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tree_kernels_match_the_oracle_per_sample(case, device, oracle64):
    lib, cus = device
    name = tree_of(case)
    b = build_tree(case, cus)
    runs, fails, want = {}, [], None
    for kernel in case.kernels:
        ran, eps, outs = run_gpu(lib, b, kernel, cus)          # (asserts the kernel's name and wavefront count)
        if want is None:                    # the oracle runs once per case, on the noise the device sampled
            np.testing.assert_allclose(eps, oracle64.sample(b.cfg), atol=1e-6)
            eps0, want = eps, run_oracle(oracle64, b, eps)
        np.testing.assert_array_equal(eps, eps0)
        assert len(outs) == len(want) == 1
        fails += compare(f"{case.name} K={b.cfg.num_samples} H={case.H} asked {kernel} ran {ran}", outs[0], want[0], b.umax, TOL[name])
        runs.setdefault(ran, outs[0])
    assert set(runs) == {"lane", "quad", "oct", "oct-pair"}
    for key, ref in runs[OCT].items():      # the helpers issue the same operations on the same values in the same order
        if ref is not None and runs[PAIR].get(key) is not None:
            np.testing.assert_array_equal(runs[PAIR][key], ref, err_msg=f"{case.name}: oct-pair vs oct, {key}")
    assert not fails, "\n".join(fails)
