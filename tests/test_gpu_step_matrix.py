"""Every env-step and materialise kernel of the batched simulator behind mppi_sim_* - k_sim_step (`lane`), k_sim_step_quad (`quad`),
k_sim_step_scene (`scene`), k_sim_step_scene_quad (`scene-quad`), k_materialise, k_materialise_scene, k_materialise_link,
k_sim_reset, k_sim_reset_scene (csrc/mppi_kernels.hpp) - against the fp64 oracle's batched env step (orc_envs_step), PER ENV, EVERY
ENV, EVERY STEP, EVERY COLUMN of the four reference-layout tensors: dof (q | qd), root and rb (position | quaternion up to sign |
linear | angular velocity), cf.

ONE table (CASES).  Per case: mppi_create with K envs through the raw C-ABI, mppi_set_state, mppi_sim_reset, N steps with commands
that differ from env to env (drawn per (step, env, column) from a seeded generator), mppi_sim_materialise after every step; the
oracle is driven with the same commands.  The step kernel that ran is asserted by exact name from mppi_kernel_info (` step=<name> `).
 A  selection and ragged env counts (K = 1 and K >= 64: `quad`, between: `lane`; MPPI_WORLD_STEP=lane, MPPI_ROLLOUT=lane)
 B  command routes: [K][nu] (mode 0), one shared device row (mode 1), mppi_sim_step_host through its 64-slot ring for 70 steps
 C  mppi_sim_step_horizon (mode 2): du against the clamp formula, the states against the oracle driven with U + du, the control-cost
    accumulator (mppi_sim_finish with no cost accumulated) against lambda sum U Sigma^-1 du in fp64; prior / null sample, absolute
    control cost, a mixed command map, two shards of one K_total.  (The shards run at K = 17 / 16: mppi_create gives every
    contact-free context of 2 .. 63 envs the `lane` kernel and offers no switch for `quad` there - `lane` only.)
    The same inputs through mppi_rollout_trajectory + mppi_materialise_trajectory (+ _link) on a second context: all H * K rows.
 D  the rare branches of the dynamics: drives at their effort limit, effort and position drive modes
 E  contact scenes: pushing scene, gripper scene at its recorded closed-loop state, per-env randomised actors (also as a shard: the
    draws follow the global index), a forest of two moving bases
 F  mppi_sim_reset after the steps and each of the four output pointers requested alone

TOLERANCES come from the oracle and the project, never from the kernels: per quantity class 10 x the worst deviation of the fp32
build of the oracle from the fp64 one over the class's cases (ORACLE32 below: measured by test_step_cases_are_well_posed, which
prints them per case), rounded up to the next 1-2-5 value, never above what the suite already asserts for that quantity (CAP).
Where a cap binds (q of the contact-free class, angular velocity of the contact class) the tenth of the tolerance that the fp32
oracle must stay within is a condition on the INPUTS: the seed of the command generator (SEED) is one of those, among the sixteen
tried on the oracle, that meet it - 12 of them leave the chassis' angular velocity of the pushing scene at 1.1e-4 .. 2.5e-4 after
four steps, against the 1e-3 the suite asserts for it.

Three inputs are not the obvious ones, for the same reason:
 * the two jackals start ON their wheels (z = 0.0616; dropped from the 0.1 m of test_check_build_on_a_forest_of_moving_bases the fp32
   oracle lands 1.8e-3 rad/s away from the fp64 one);
 * mode 2 on the pushing scene scales the sampled noise by 0.03 and takes a nominal of 0.02: commands of about +-0.1 like the rest
   of E.  With the 0.3 of the open-floor COST tests (commands up to 1.7 rad/s) the fp32 oracle reaches 0.27 of the cf bound and
   6e-4 rad/s after four steps - not a case in which a state tolerance means anything.  The row's u_min / u_max are narrowed to
   -+0.1, where the commands of E end, so that the clamp works as in every mode-2 row (11 % of its controls end on it);
 * the gripper scene runs N = 4 steps like every contact scene.

test_step_cases_are_well_posed (no GPU) checks on the oracle alone that a pass means something: everything finite, the fp32 oracle
within a TENTH of every tolerance on every env at every compared step, every env told apart from its neighbour and from env 0 by
more than 100 x a tolerance (an index mix-up cannot pass), the effort limits / drive modes / randomised actors change the result,
mode-2 controls reach the clamp in some but not all entries."""
import ctypes as C
import dataclasses
import os
import types

import numpy as np
import pytest

from mppiisaac.backend import capi
from scenes import boxer_push, build_scene, panda_pick, panda_reach, point_reach
from test_gpu_rollout_matrix import AUTO, PRIOR, Gpu, P, environment
from test_gpu_rollout_matrix import build as build_rollout_case

GOLDEN_STATES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "closed_loop_states.npz")
KEYS = ("q", "qd", "pos", "quat", "lin", "ang", "cf")
# what the suite already asserts (tests/test_gpu_parity.py: test_rollout_trajectory_states_match_oracle_stepping,
# test_world_sim_matches_oracle_and_reference_layouts, test_boxer_generic_mode_and_world); cf in units of (5 N + 5e-3 |cf|)
CAP = {"free": {"q": 1e-5, "qd": 2e-4, "pos": 2e-5},
       "ring": {"q": 1e-4, "qd": 5e-4},
       "contact": {"q": 1e-3, "pos": 1e-4, "quat": 1e-4, "lin": 1e-3, "ang": 1e-3, "cf": 1.0}}
# worst fp32-against-fp64 oracle deviation of each class (printed by test_step_cases_are_well_posed; cf: of 5 N + 5e-3 |cf|)
ORACLE32 = {"free": {"q": 8.33e-7, "qd": 4.59e-6, "pos": 4.58e-7, "quat": 5.28e-7, "lin": 2.27e-6, "ang": 4.37e-6, "cf": 0.0},
            "ring": {"q": 1.16e-6, "qd": 3.11e-8, "pos": 8.01e-7, "quat": 9.54e-7, "lin": 1.60e-6, "ang": 1.81e-6, "cf": 0.0},
            "contact": {"q": 1.58e-6, "qd": 1.96e-5, "pos": 8.30e-7, "quat": 1.02e-6, "lin": 3.68e-5, "ang": 8.92e-5, "cf": 3.49e-2}}
# -> TOL free:    q 1e-5 (cap)  qd 5e-5  pos 5e-6  quat 1e-5  lin 5e-5  ang 5e-5  cf 0 (exact zeros)
#        ring:    q 2e-5        qd 5e-7  pos 1e-5  quat 1e-5  lin 2e-5  ang 2e-5  cf 0
#        contact: q 2e-5        qd 2e-4  pos 1e-5  quat 2e-5  lin 5e-4  ang 1e-3 (cap)  cf 0.5 x (5 N + 5e-3 |cf|)


def round_up_125(x):
    if x <= 0.0:
        return 0.0
    e = int(np.floor(np.log10(x)))
    return next(float(f"{m}e{e}") for m in (1, 2, 5, 10) if x <= float(f"{m}e{e}"))


TOL = {kl: {k: min(round_up_125(10.0 * v), CAP[kl].get(k, np.inf)) for k, v in d.items()} for kl, d in ORACLE32.items()}
DU_TOL, CTRL_REL = 1e-6, 1e-5          # the project's bound on du; control cost: H * nu <= 42 fp32 additions -> 1e-5 * sum |terms|
KMAX = 80                              # the whole workload of a case: nothing larger
SEED = 15                              # of the command generator (see the module docstring)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    scene: str                   # panda | point | boxer | pick | jackals
    K: int
    step: str                    # the step kernel mppi_kernel_info must name
    route: str = "mode0"         # mode0: u [K][nu] | mode1: one shared device row | host: mppi_sim_step_host | horizon: mode 2
    N: int = 6
    env: tuple = ()              # environment of mppi_create, as (name, value) pairs
    tweak: str = ""              # effort-limits | drive-effort | drive-position
    seed: int = -1               # randomize_seed of the scene
    k_offset: int = 0
    variant: str = ""            # horizon route: plain | abs-cost | prior | cmd-map | shard-hi | shard-lo
    compared: tuple = ()         # steps (1-based) that are materialised and compared; default: all
    extras: bool = False         # F: partial outputs, reset
    may_refuse: bool = False     # mppi_create may refuse the one-lane kernels of this scene (LDS)

    @property
    def klass(self):
        return "ring" if self.route == "host" else ("free" if self.scene in ("panda", "point") else "contact")

    @property
    def steps(self):
        return self.compared or tuple(range(1, self.N + 1))

    def group(self):
        """cases of one group differ in K and in the kernel only: one oracle run at the largest K serves them all"""
        return (self.scene, self.route if self.route in ("mode1", "host") else "per-env", self.N, self.tweak, self.seed, self.k_offset)


AMP = {"panda": 1.0, "point": 2.0, "boxer": 0.1, "pick": 0.5, "jackals": 0.1, "effort-limits": 2.0, "drive-effort": 20.0, "drive-position": 1.0}
# the trees of tests/test_gpu_tree_steps.py (its cases name their tree as `scene`): the control range of tests/test_gpu_tree_matrix.py
AMP.update({t: 0.5 for t in ("panda_gripper", "panda_gripper_pos", "omnipanda", "omnipanda_effort", "heijn", "panda_effort", "point_forest")})
CASES = []
# A. selection and ragged counts: K = 1 the world (one quad), 2 .. 63 one lane per env, from 64 a quad per env (65: the last
#    workgroup holds one live quad of sixteen); MPPI_WORLD_STEP=lane; MPPI_ROLLOUT=lane at K = 65: one live lane in the second wavefront
for K in (1, 2, 15, 16, 17, 63, 64, 65, 80):
    CASES.append(Case(f"A-panda-K{K}", "panda", K, "quad" if K == 1 or K >= 64 else "lane"))
for K in (1, 17, 64, 65):
    CASES.append(Case(f"A-point-K{K}", "point", K, "quad" if K == 1 or K >= 64 else "lane"))
CASES += [Case("A-panda-K1-world-lane", "panda", 1, "lane", env=(("MPPI_WORLD_STEP", "lane"),)),
          Case("A-panda-K65-rollout-lane", "panda", 65, "lane", env=(("MPPI_ROLLOUT", "lane"),))]
# B. command routes
for K in (17, 65):
    CASES += [Case(f"B-mode0-K{K}", "panda", K, "lane" if K < 64 else "quad"), Case(f"B-mode1-K{K}", "panda", K, "lane" if K < 64 else "quad", route="mode1")]
for K in (1, 5):   # the ring has 64 slots: 70 steps wrap it and pass the back-pressure wait
    CASES.append(Case(f"B-host-K{K}", "panda", K, "quad" if K == 1 else "lane", route="host", N=70, compared=(1, 64, 65, 70)))
# C. mode 2
for K in (17, 65):
    for v in ("plain", "abs-cost", "prior", "cmd-map"):
        CASES.append(Case(f"C-{v}-K{K}", "panda", K, "lane" if K < 64 else "quad", route="horizon", variant=v))
CASES += [Case("C-shard-hi-K17", "panda", 17, "lane", route="horizon", variant="shard-hi", k_offset=16),     # prior and null at local 15, 16
          Case("C-shard-lo-K16", "panda", 16, "lane", route="horizon", variant="shard-lo")]                  # neither in the shard
# D. dynamics branches
for K in (17, 65):
    for tw in ("effort-limits", "drive-effort", "drive-position"):
        CASES.append(Case(f"D-{tw}-K{K}", "panda", K, "lane" if K < 64 else "quad", tweak=tw))
# E. contact scenes
for sc in ("boxer", "pick"):
    for K in (1, 7, 17, 65):
        CASES.append(Case(f"E-{sc}-K{K}", sc, K, "scene-quad", N=4))
    for K in (7, 65):
        CASES.append(Case(f"E-{sc}-K{K}-rollout-lane", sc, K, "scene", N=4, env=(("MPPI_ROLLOUT", "lane"),), may_refuse=sc == "pick"))
CASES += [Case("E-boxer-random-K65", "boxer", 65, "scene-quad", N=4, seed=3), Case("E-boxer-random-shard-K65", "boxer", 65, "scene-quad", N=4, seed=3, k_offset=16),
          Case("E-jackals-K5", "jackals", 5, "scene", N=4), Case("E-jackals-K65", "jackals", 65, "scene", N=4),
          Case("E-boxer-horizon-K17", "boxer", 17, "scene-quad", N=4, route="horizon", variant="scaled")]
# F. reset and partial outputs
CASES += [Case("F-panda-K65", "panda", 65, "quad", extras=True), Case("F-boxer-K65", "boxer", 65, "scene-quad", N=4, extras=True)]
IDS = [c.name for c in CASES]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def build(case):
    """-> what Gpu() of the rollout matrix takes (m, cfg, cost = None, dof, root, U0, prior) and the scene"""
    K, H = case.K, case.N if case.route == "horizon" else 6
    prior = None
    if case.scene == "panda" and case.route == "horizon":
        kw = {"plain": {}, "abs-cost": dict(over=dict(noise_abs_cost=True)), "prior": PRIOR, "shard-hi": PRIOR, "shard-lo": PRIOR,
              "cmd-map": dict(cmd_map=True, over=dict(noise_sigma=(0.1 * np.eye(5)).tolist()))}[case.variant]
        r = build_rollout_case(P(case.name, 33 if case.variant.startswith("shard") else K, H, (AUTO,), **kw), 256)
        scene, m, cfg, dof, root, U0, prior = r.scene, r.m, r.cfg, r.dof, r.root, r.U0, r.prior
        if case.variant.startswith("shard"):
            assert cfg.k_total == 33
            cfg.num_samples, cfg.k_offset = K, case.k_offset
    elif case.scene == "jackals":
        from mppiisaac.planner.mppi import MPPIConfig, make_config
        scene = build_scene(["jackal_a", "jackal_b", "goal"], [[0.0, 0.0, 0.1], [0.5, -2.0, 0.1]])
        cfg = make_config(MPPIConfig(num_samples=K, horizon=H, noise_sigma=np.eye(4).tolist(), lambda_=0.01, u_min=[-1.5], u_max=[1.5],
                                     sample_null_action=True), viz_link=scene.viz_link_index())
        dof, root = scene.initial_state()
        root[0:2, 2] = 0.0616            # on their wheels (dropped from 0.1 they come to rest at 0.06159)
    else:
        make = {"panda": panda_reach, "point": point_reach, "boxer": boxer_push, "pick": panda_pick}[case.scene]
        scene, _, cfg, _, dof, root = make(K=K, H=H)
    dof, root = np.array(dof, np.float32), np.array(root, np.float32)
    if case.scene == "boxer":            # on its wheels, the block in front of it
        root[0, 2] = 0.019
        root[scene.actor_index("block"), 0:3] = [0.0, 1.9, 0.0923]
    if case.scene == "pick":             # the recorded closed-loop state
        Z = np.load(GOLDEN_STATES)
        dof, root = Z["panda_pick_recorded_dof"].astype(np.float32), Z["panda_pick_recorded_root"].astype(np.float32)
    if case.seed >= 0:
        scene.randomize_seed = case.seed
    if not (case.scene == "panda" and case.route == "horizon"):
        m = scene.to_c()
    if case.route != "horizon" and case.k_offset:
        cfg.k_offset, cfg.k_total = case.k_offset, case.k_offset + K
    if case.tweak == "effort-limits":    # as test_effort_saturated_drives_match_oracle
        for i in range(m.n_bodies):
            m.bodies[i].effort = 4.0 if i < 4 else 2.0
    elif case.tweak == "drive-effort":
        m.drive_mode, m.drive_kd = capi.DRIVE_EFFORT, 10.0
    elif case.tweak == "drive-position":
        m.drive_mode, m.drive_kp, m.drive_kd = capi.DRIVE_POSITION, 400.0, 40.0
    if case.route != "horizon":
        U0 = np.zeros((H, cfg.nu), np.float32)
    elif case.scene == "boxer":          # a small nominal, so that the control cost is not zero; the clamp where the commands of E end
        U0 = (0.02 * np.random.default_rng(0).normal(size=(H, cfg.nu))).astype(np.float32)
        for j in range(cfg.nu):
            cfg.u_min[j], cfg.u_max[j] = -AMP["boxer"], AMP["boxer"]
    return types.SimpleNamespace(case=case, scene=scene, m=m, cfg=cfg, cost=None, dof=dof, root=root, U0=U0, prior=prior)


def commands(case, nu, K=None):
    """[N][K][nu], one draw per (step, env, column): an env's commands do not depend on how many envs there are"""
    amp = AMP[case.tweak or case.scene]
    u = np.random.default_rng(SEED).uniform(-amp, amp, size=(case.N, KMAX, nu))
    if case.route in ("mode1", "host"):      # one row for every env, a new row every step
        u[:] = u[:, :1]
    return np.ascontiguousarray(u[:, :K or case.K].astype(np.float32))


def horizon_controls(b, eps):
    """mode 2 in numpy: -> (du [H][nu][K] by the clamp formula, u [H][K][nu] = U + du), fp64"""
    cfg, K = b.cfg, b.cfg.num_samples
    nu = cfg.nu
    lo, hi = np.array([cfg.u_min[j] for j in range(nu)]), np.array([cfg.u_max[j] for j in range(nu)])
    U = b.U0.astype(np.float64)
    v = U[:, :, None] + eps.astype(np.float64)
    g = cfg.k_offset + np.arange(K)
    if cfg.sample_null_action:
        v[:, :, g == cfg.k_total - 1] = 0.0
    if cfg.use_priors and b.prior is not None:
        v[:, :, g == cfg.k_total - 2] = b.prior.astype(np.float64)[:, :, None]
    v = np.clip(v, lo[None, :, None], hi[None, :, None])
    return v - U[:, :, None], np.ascontiguousarray(v.transpose(0, 2, 1)), np.mean((v == lo[None, :, None]) | (v == hi[None, :, None]))


def control_cost(b, du):
    """lambda sum_t U Sigma^-1 du per env in fp64 and the sum of the absolute terms (the bound's scale)"""
    cfg = b.cfg
    inv = np.array([1.0 / cfg.noise_sigma_diag[j] for j in range(cfg.nu)])
    terms = cfg.lambda_ * b.U0.astype(np.float64)[:, :, None] * inv[None, :, None] * du
    return (np.abs(terms) if cfg.noise_abs_cost else terms).sum((0, 1)), np.abs(terms).sum((0, 1))


def noise_scale(case):
    return np.float32(0.03) if case.variant == "scaled" else np.float32(1.0)


# ---- the oracle side ---------------------------------------------------------------------------------------------------------------
def oracle_steps(o, b, u, g0):
    """orc_envs_step from (dof, root) of b with u [N][K][nu] -> the four tensors after every step, [N][K]..."""
    m, f = b.m, o.dtype
    N, K = u.shape[0], u.shape[1]
    n, A, B = m.n_bodies, m.n_actors, m.n_rb
    dof = np.tile(b.dof.astype(f).reshape(1, -1), (K, 1))
    root = np.tile(b.root.astype(f).reshape(1, A, 13), (K, 1, 1))
    rb, cf = np.zeros((K, B, 13), f), np.zeros((K, B, 3), f)
    out = {"dof": [], "root": [], "rb": [], "cf": []}
    for t in range(N):
        ut = np.ascontiguousarray(u[t], f)
        o.lib.orc_envs_step(C.byref(m), C.c_int(K), C.c_int(g0), o.p(ut), o.p(dof), o.p(root), o.p(rb), o.p(cf))
        for k, v in (("dof", dof), ("root", root), ("rb", rb), ("cf", cf)):
            out[k].append(v.copy())
    return {k: np.stack(v).astype(np.float64) for k, v in out.items()}


_REFS = {}


def reference(o, case, b, u=None):
    """the oracle's states of `case` at its compared steps; per-env and shared-command cases of one group share one run at the
    group's largest K (envs are independent: env k of a smaller case is env k of the larger one), kept unchanged"""
    if u is not None:                        # mode 2: the commands depend on K (prior / null sample)
        full = oracle_steps(o, b, u, b.cfg.k_offset)
    else:
        key = (o.dtype, case.group())
        if key not in _REFS:
            Kg = max(c.K for c in CASES if c.group() == case.group() and c.route != "horizon")
            _REFS[key] = oracle_steps(o, b, commands(case, b.m.nu, Kg), case.k_offset)
            for v in _REFS[key].values():
                v.setflags(write=False)
        full = {k: v[:, :case.K] for k, v in _REFS[key].items()}
    sel = [s - 1 for s in case.steps]
    return {k: v[sel] for k, v in full.items()}


def deviations(a, b):
    """per quantity class the deviation of run a from run b, [steps][K] (the worst column of the env); quaternions up to sign;
    cf in units of the suite's bound 5 N + 5e-3 |cf|"""
    d = np.abs(a["dof"] - b["dof"])
    out = {"q": d[..., 0::2].max(-1), "qd": d[..., 1::2].max(-1)}
    for key, sl in (("pos", slice(0, 3)), ("lin", slice(7, 10)), ("ang", slice(10, 13))):
        out[key] = np.maximum(*(np.abs(a[t][..., sl] - b[t][..., sl]).max((-1, -2)) for t in ("root", "rb")))
    quat = lambda t: np.minimum(np.abs(a[t][..., 3:7] - b[t][..., 3:7]).max(-1), np.abs(a[t][..., 3:7] + b[t][..., 3:7]).max(-1)).max(-1)
    out["quat"] = np.maximum(quat("root"), quat("rb"))
    out["cf"] = (np.abs(a["cf"] - b["cf"]) / (5.0 + 5e-3 * np.abs(b["cf"]))).max((-1, -2))
    return {k: np.where(np.isfinite(v), v, np.inf) for k, v in out.items()}


def tolerances(klass):
    """the tolerances of a quantity class of this module, or the table (quantity -> tolerance) a caller measured for its own cases"""
    return klass if isinstance(klass, dict) else TOL[klass]


def compare(tag, got, want, klass):
    """prints the measured maxima next to the tolerances, then -> (list of failures, maxima)"""
    dev = deviations(got, want)
    fails, cells, worst = [], [], {}
    for key in KEYS:
        worst[key], tol = float(dev[key].max()), tolerances(klass)[key]
        cells.append(f"{key} {worst[key]:.1e} ({tol:.0e})")
        if not worst[key] <= tol:
            s, k = np.unravel_index(np.argmax(dev[key]), dev[key].shape)
            fails.append(f"{tag}: {key} off by {worst[key]:.3e} > {tol:.0e} at compared step {s}, env {k}")
    print(f"{tag}: " + " | ".join(cells))
    return fails, worst


# ---- the conditions on the inputs, on the oracle alone -----------------------------------------------------------------------------
def told_apart(ref, klass, k, j):
    """some compared quantity of env k differs from env j's by more than 100 x its tolerance"""
    pick = lambda r, e: {key: v[:, e:e + 1] for key, v in r.items()}
    dev = deviations(pick(ref, k), pick(ref, j))
    return any(dev[key].max() > 100.0 * tolerances(klass)[key] for key in KEYS if tolerances(klass)[key] > 0)


def differs_in(ref, other, klass):
    """fraction of the envs in which some quantity of the two runs differs by more than 100 x its tolerance"""
    dev = deviations(ref, other)
    return np.mean(np.any([dev[key].max(0) > 100.0 * tolerances(klass)[key] for key in KEYS if tolerances(klass)[key] > 0], axis=0))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_cases_are_well_posed(case, oracle64, oracle32):
    assert IDS.count(case.name) == 1 and case.K <= KMAX and case.N <= 70
    b = build(case)
    u = None
    if case.route == "horizon":
        eps = oracle64.sample(b.cfg)
        if case.variant.startswith("shard"):      # the shard's noise is its slice of the K_total set
            full = type(b.cfg).from_buffer_copy(b.cfg)
            full.num_samples, full.k_offset = 33, 0
            np.testing.assert_array_equal(eps, oracle64.sample(full)[:, :, case.k_offset:case.k_offset + case.K])
        du, u, clamped = horizon_controls(b, eps * noise_scale(case))
        cc, scale = control_cost(b, du)
        print(f"{case.name}: {100 * clamped:.1f} % of the controls at the clamp, control cost in [{cc.min():.3g}, {cc.max():.3g}]")
        assert 0.01 <= clamped <= 0.80 and np.abs(b.U0).min() > 0 and scale.min() > 0
        g = b.cfg.k_offset + np.arange(case.K)
        if case.variant in ("prior", "shard-hi"):    # the prior conditions of the rollout matrix; here both samples are in the shard
            assert b.cfg.use_priors and b.cfg.sample_null_action and (g == b.cfg.k_total - 2).sum() == 1 and (g == b.cfg.k_total - 1).sum() == 1
            umax = max(abs(b.cfg.u_max[0]), abs(b.cfg.u_min[0]))
            far = lambda d: np.abs(d).max(axis=1).min() > 0.05 * umax
            assert far(b.prior) and far(b.prior - b.U0) and far(np.diff(b.prior, axis=0))
        if case.variant == "shard-lo":
            assert b.prior is not None and g.max() < b.cfg.k_total - 2
    r64, r32 = reference(oracle64, case, b, u), reference(oracle32, case, b, u)
    assert all(np.isfinite(v).all() for v in r64.values()) and all(np.isfinite(v).all() for v in r32.values())
    dev, kl = deviations(r32, r64), case.klass
    print(f"{case.name}: fp32 oracle vs fp64 oracle: " + " | ".join(f"{k} {dev[k].max():.1e} (tol/10 {TOL[kl][k] / 10:.0e})" for k in KEYS))
    for k in KEYS:
        assert dev[k].max() <= TOL[kl][k] / 10.0, f"{k}: the fp32 oracle leaves the fp64 one by more than a tenth of the tolerance"
    if case.route not in ("mode1", "host"):      # (one command for every env there: the envs are copies of each other by definition)
        for k in range(1, case.K):
            assert told_apart(r64, kl, k, k - 1) and told_apart(r64, kl, k, 0), f"env {k} is not told apart from env {k - 1} / env 0"
    if case.tweak:                               # the limits / the drive mode matter: the stock velocity-driven arm does something else
        stock = build(dataclasses.replace(case, tweak=""))
        other = oracle_steps(oracle64, stock, commands(case, b.m.nu), 0)
        frac = differs_in(r64, {k: v[[s - 1 for s in case.steps]] for k, v in other.items()}, kl)
        print(f"{case.name}: differs from the stock arm under the same commands in {100 * frac:.0f} % of the envs")
        assert frac > 0.5
    if case.seed >= 0:                           # the randomised actors matter: the block's weight on the ground
        nominal = build(dataclasses.replace(case, seed=-1))
        other = oracle_steps(oracle64, nominal, commands(case, b.m.nu), case.k_offset)
        frac = np.mean(np.abs(r64["cf"] - other["cf"]).max((0, 2, 3)) > 1.0)
        print(f"{case.name}: cf rows differ from the nominal model's by more than 1 N in {100 * frac:.0f} % of the envs")
        assert frac > 0.5


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return capi.load_library()


class Tensors:
    """the four reference-layout device tensors of `rows` envs, filled with NaN before every call"""

    def __init__(self, m, rows):
        import torch
        shapes = {"dof": (rows, 2 * m.n_bodies), "root": (rows, m.n_actors, 13), "rb": (rows, m.n_rb, 13), "cf": (rows, m.n_rb, 3)}
        self.t = {k: torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for k, s in shapes.items()}

    def fill(self, g, name, only=None):
        import torch
        for v in self.t.values():
            v.fill_(float("nan"))
        torch.cuda.synchronize()             # (the context launches on a stream of its own)
        g.call(name, *(C.c_void_p(self.t[k].data_ptr()) if only in (None, k) else None for k in ("dof", "root", "rb", "cf")))
        g.call("mppi_synchronize")
        return {k: v.cpu().numpy().copy() for k, v in self.t.items()}


def stacked(rows):
    return {k: np.stack([r[k] for r in rows]).astype(np.float64) for k in rows[0]}


def open_context(lib, case, b):
    env = dict(case.env)
    with environment(MPPI_WORLD_STEP=env.get("MPPI_WORLD_STEP")):
        g = Gpu(lib, b, env.get("MPPI_ROLLOUT", AUTO))
    assert f" step={case.step} " in g.info, (case.name, g.info)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_kernels_match_the_oracle_per_env(case, lib, oracle64):
    """D-effort-limits-K65 is the row that found something: with the articulated-body solve of a saturated drive taken about the
    WORLD origin (as the solve under the implicit drive still is, where kd h = 15 hides it) the `quad` kernel left the oracle by
    qd 5.8e-5 / angular 5.4e-5 at env 35 against 5e-5, the `lane` kernel by 1.9e-5 on envs 0 .. 16 - the fp32 oracle by 4.6e-6.
    The re-solve of step / quad_step is now taken about the last body's origin (mppi_quad.hpp quad_step)."""
    import torch
    b = build(case)
    K, nu, m = case.K, b.cfg.nu, b.m
    try:
        g = open_context(lib, case, b)
    except capi.MppiHipError as e:
        # the one-lane kernels keep 64 envs' rows in LDS per wavefront: a scene that needs more than 160 KiB for them is refused
        assert case.may_refuse and "libmppi_hip error -3" in str(e) and "160 KiB" in str(e), (case.name, e)
        print(f"{case.name}: mppi_create refuses the one-lane kernels of this scene ({e})")
        return
    T = Tensors(m, K)
    tag = f"{case.name} K={K} step={case.step}"
    u = None
    if case.route == "horizon":
        np.testing.assert_allclose(g.eps, oracle64.sample(b.cfg), atol=2e-6 if case.klass == "contact" else 1e-6)
        eps = g.eps * noise_scale(case)
        if case.variant == "scaled":
            ext = torch.from_numpy(eps).cuda().contiguous()
            g.call("mppi_set_noise_dev", C.c_void_p(ext.data_ptr()))
        du, u, _ = horizon_controls(b, eps)
    else:
        cmds = commands(case, nu)
        dev_u = torch.from_numpy(cmds).cuda().contiguous()
    g.call("mppi_sim_reset")
    rows = []
    for t in range(case.N):
        if case.route == "mode0":
            g.call("mppi_sim_step", C.c_void_p(dev_u[t].data_ptr()), 0)
        elif case.route == "mode1":
            g.call("mppi_sim_step", C.c_void_p(dev_u[t, 0].data_ptr()), 1)
        elif case.route == "host":
            g.call("mppi_sim_step_host", capi.fptr(np.ascontiguousarray(cmds[t, 0])))
        else:
            g.call("mppi_sim_step_horizon", t)
        if t + 1 in case.steps:
            rows.append(T.fill(g, "mppi_sim_materialise"))
    got, want = stacked(rows), reference(oracle64, case, b, u)
    fails, _ = compare(tag, got, want, case.klass)
    if case.klass != "contact":
        assert not got["cf"].any(), "contact forces of a contact-free scene"
    if case.route == "horizon":
        g.call("mppi_sim_finish")
        S, du_dev = g.get("mppi_get_costs", (K,)), g.get("mppi_get_perturbations", (case.N, nu, K))
        cc, scale = control_cost(b, du)
        print(f"{tag}: du {np.abs(du_dev - du).max():.1e} ({DU_TOL:.0e}) | control cost {np.max(np.abs(S - cc) / scale):.1e} of sum |terms| ({CTRL_REL:.0e})")
        fails += [f"{tag}: du"] * (not np.abs(du_dev - du).max() <= DU_TOL) + [f"{tag}: control cost"] * (not (np.abs(S - cc) <= CTRL_REL * scale).all())
        fails += trajectory_dump(lib, case, b, tag, want, du, cc, scale)
    if case.extras:
        partial_outputs_and_reset(g, case, b, T, rows[-1], oracle64)
    g.close()
    assert not fails, "\n".join(fails)


def trajectory_dump(lib, case, b, tag, want, du, cc, scale):
    """the same horizon through mppi_rollout_trajectory + mppi_materialise_trajectory on a second context: all H * K rows"""
    import torch
    H, K, m = case.N, case.K, b.m
    g = Gpu(lib, b, AUTO)
    assert "rollout=lane " not in g.info and "rollout=scene " not in g.info        # (a kernel that has the dump)
    if case.variant == "scaled":
        ext = torch.from_numpy(g.eps * noise_scale(case)).cuda().contiguous()
        g.call("mppi_set_noise_dev", C.c_void_p(ext.data_ptr()))
    g.call("mppi_rollout_trajectory")
    T = Tensors(m, H * K)
    got = {k: v.reshape((H, K) + v.shape[1:]).astype(np.float64) for k, v in T.fill(g, "mppi_materialise_trajectory").items()}
    fails, _ = compare(tag + " trajectory dump", got, want, case.klass)
    S, du_dev = g.get("mppi_get_costs", (K,)), g.get("mppi_get_perturbations", (H, b.cfg.nu, K))
    fails += [f"{tag}: dump du"] * (not np.abs(du_dev - du).max() <= DU_TOL) + [f"{tag}: dump control cost"] * (not (np.abs(S - cc) <= CTRL_REL * scale).all())
    if case.klass != "contact":      # the rows of the cost link alone are the rb rows of that link, bit for bit
        link = b.scene.rigid_body_index("panda", "panda_ee_tip")
        out = torch.full((H * K, 13), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g.call("mppi_materialise_trajectory_link", link, C.c_void_p(out.data_ptr()))
        g.call("mppi_synchronize")
        np.testing.assert_array_equal(out.cpu().numpy(), T.t["rb"].cpu().numpy()[:, link, :], err_msg=f"{tag}: link rows")
    g.close()
    return fails


def partial_outputs_and_reset(g, case, b, T, full, oracle64):
    """F: each output pointer alone = its counterpart of the four-pointer call, bit for bit; then a reset to another x0"""
    for only in ("dof", "root", "rb", "cf"):
        alone = T.fill(g, "mppi_sim_materialise", only=only)
        np.testing.assert_array_equal(alone[only], full[only], err_msg=f"{case.name}: {only} requested alone")
        for other in alone:
            assert other == only or np.isnan(alone[other]).all(), f"{case.name}: {other} written though not requested"
    if case.klass != "contact":
        assert not T.fill(g, "mppi_sim_materialise", only="cf")["cf"].any()
    m, K = b.m, case.K
    dof1 = (b.dof + 0.05 * np.cos(np.arange(b.dof.size))).astype(np.float32)
    root1 = b.root.copy()
    root1[:, 0:2] += np.float32(0.125) * (1 + np.arange(m.n_actors, dtype=np.float32))[:, None]     # every actor somewhere else
    g.call("mppi_set_state", capi.fptr(dof1), capi.fptr(root1))
    g.call("mppi_sim_reset")
    got = T.fill(g, "mppi_sim_materialise")
    np.testing.assert_array_equal(got["dof"], np.tile(dof1[None], (K, 1)), err_msg=f"{case.name}: dof rows after the reset")
    np.testing.assert_array_equal(got["root"], np.tile(root1[None], (K, 1, 1)), err_msg=f"{case.name}: root rows after the reset (free-actor slots)")
    assert not got["cf"].any(), "cf after the reset"
    assert (got["rb"] == got["rb"][:1]).all()
    rbo, _ = oracle64.rigid_body_state(m, root1, dof1[0::2], dof1[1::2])
    x0 = {"dof": dof1[None, None], "root": root1[None, None], "rb": rbo[None, None], "cf": np.zeros((1, 1, m.n_rb, 3))}
    fails, _ = compare(f"{case.name} after the reset", {k: v[None, :1].astype(np.float64) for k, v in got.items()}, {k: np.asarray(v, np.float64) for k, v in x0.items()}, case.klass)
    assert not fails, "\n".join(fails)
