"""The table of single-term cost programs (MPPI_COST_PROGRAM, include/mppi_hip.h) that pins the interpreter of the rollout
kernels (csrc/mppi_device.hpp program_cost_with; StaticEnv / GivenEnv / SceneEnv; link_pose; the quad-layout gather of
mppi_scene_quad.hpp; pack_cost) to the fp64 oracle TERM BY TERM: every row is a program of one term with weight 1 (a few with
-2.5, one with MPPI_MAX_TERMS terms), so nothing hides behind a heavier term.  tests/test_cost_term_cases.py checks on the oracle
and on the host build that a pass means something; tests/test_gpu_cost_terms.py runs the rows on the device.

Route A  mppi_eval_cost (k_eval_cost + GivenEnv) on N_ENVS designed envs per row, at the edges of each measurement; reference:
         oracle64.cost on the fp32-rounded inputs, env by env; tolerance per row class rtol = atol = max(2e-6, 10 x the worst
         deviation of the fp32 oracle from the fp64 one over the class, rounded up 1-2-5) - ORACLE32_A holds those deviations.
Route B  S[k] of mppi_rollout against oracle64.rollout under the same program, every sample; tolerance per row: 10 x the worst
         per-sample deviation of oracle32.rollout from oracle64.rollout, rounded up 1-2-5, relative to max |S| of the row - and
         never below route A's 2e-6: where the two oracle builds happen to agree to 1e-7 (joint velocities that follow their
         targets, a block nothing reaches) ten fp32 roundings of the same sum exceed 10 x that, and route C - the same costs
         without the dynamics - is floored there too.
Route C  the octet kernels against sum_t gamma^t oracle64.cost on their OWN dumped trajectory (+ the fp64 control cost): the
         dynamics drop out of the comparison; tolerance 10 x the worst deviation of the two oracle builds on those states, never
         below route A's 2e-6 (rollout_costs_on below is that reference; the GPU test feeds it the device's states).

Excluded inputs: a TILT row exactly on the gimbal (the reference evaluates atan2(+-0, +-0) there and jumps by pi with the sign of a
zero - well_posed_a rejects every input on which the two oracle builds differ by more than 1e-3); the zero-length ALIGN ray is
compared for non-finiteness only (the reference gives NaN)."""
import dataclasses
import functools
import os
import types

import numpy as np

from mppiisaac.backend import capi
from scenes import boxer_push, build_scene, panda_pick, panda_reach

GOLDEN_STATES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "closed_loop_states.npz")
N_ENVS = 130            # route A: two full wavefronts and a tail of 2 (the k >= n guard of k_eval_cost)
FLOOR = 2e-6            # what the suite already asserts on mppi_eval_cost (test_golden_objective_inputs_through_the_hip_cost_program)
GAMMA = 0.9             # rollout_var_discount of every route B / C context
H = 3
f32 = lambda a: np.ascontiguousarray(a, np.float32)

# worst deviation |oracle32.cost - oracle64.cost| / (1 + |oracle64.cost|) over the envs of each route A class (measured by
# tests/test_cost_term_cases.py::test_route_a_constants_are_current, which fails when one is out of date by a factor 2)
ORACLE32_A = {"DIST": 8.5e-8, "TILT": 1.4e-5, "YAW_ABS": 1.1e-7, "ALIGN": 1.8e-7, "FORCE_L1": 1.2e-7, "SPEED": 3.9e-8, "DOF_SQ": 1.8e-7,
              "ABS_DZ": 3.8e-8, "BELOW": 3.8e-8, "MAXTERMS": 2.2e-7}
# -> rtol = atol: TILT 2e-4 (asin next to +-1: 1.4e-5 at delta = 1e-3), DOF_SQ and MAXTERMS 2e-6 (1.8e-6 / 2.2e-6 -> 2e-6 / 5e-6), the rest the floor


def round_up_125(x):
    if x <= 0.0:
        return 0.0
    e = int(np.floor(np.log10(x)))
    return next(float(f"{m}e{e}") for m in (1, 2, 5, 10) if x <= float(f"{m}e{e}") * (1 + 1e-12))


def tol_a(klass):
    return max(FLOOR, round_up_125(10.0 * ORACLE32_A[klass]))


# ---- programs ----------------------------------------------------------------------------------------------------------------------
def term(op, n=0, src=(), idx=(), w=1.0, p=()):
    return dict(op=op, n=n, src=tuple(src), idx=tuple(idx), w=w, p=tuple(p))


def program(*terms):
    c = capi.Cost()
    c.kind, c.n_terms = capi.COST_PROGRAM, len(terms)
    for i, t in enumerate(terms):
        c.terms[i].op, c.terms[i].n, c.terms[i].w = t["op"], t["n"], t["w"]
        for j, v in enumerate(t["src"]):
            c.terms[i].src[j] = v
        for j, v in enumerate(t["idx"]):
            c.terms[i].idx[j] = v
        for j, v in enumerate(t["p"]):
            c.terms[i].p[j] = v
    return c


def changed(t, **kw):
    t = dict(t)
    t.update(kw)
    return t


def with_idx(t, a, v):
    idx = list(t["idx"]) + [0] * (3 - len(t["idx"]))
    idx[a] = v
    return changed(t, idx=tuple(idx))


RB, ACTOR, DOF_XY, CONST = capi.SRC_RB, capi.SRC_ACTOR, capi.SRC_DOF_XY, capi.SRC_CONST


# ---- route A -----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class RowA:
    name: str
    klass: str
    ctx: str                     # push | anymal
    terms: tuple
    dof: np.ndarray              # [n][2 nd]
    root: np.ndarray             # [n][A][13]
    rb: np.ndarray               # [n][B][13]
    cf: np.ndarray               # [n][B][3]
    edges: dict                  # edge name -> env indices that reach it
    nonfinite: np.ndarray = None  # envs in which the reference is not finite (the zero-length ALIGN rays): exactly these
    bit_equal_to: str = ""       # another row whose device values this row's must equal bit for bit

    @property
    def cost(self):
        return program(*self.terms)


@functools.lru_cache(maxsize=None)
def context_a(which):
    """-> (scene, model, config) of the two route A contexts"""
    from mppiisaac.planner.mppi import MPPIConfig, make_config
    if which == "push":
        scene = boxer_push(K=64, H=4)[0]
    else:
        scene = build_scene(["anymal", "goal"], [[0.0, 0.0, 0.62]])
        assert scene.n_dof >= 9
    m = scene.to_c()
    cfg = make_config(MPPIConfig(num_samples=64, horizon=4, noise_sigma=np.eye(m.nu).tolist()))
    return scene, m, cfg


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def base_inputs(scene, seed):
    """rows the term never asks for are filled too, each row at its own scale: a wrong row shows"""
    rng = np.random.default_rng(seed)
    n, nd, A, B = N_ENVS, scene.n_dof, len(scene.env_cfg), scene.n_rb
    dof = rng.uniform(-1.5, 1.5, (n, 2 * nd))
    root, rb = rng.uniform(-2.0, 2.0, (n, A, 13)), rng.uniform(-2.0, 2.0, (n, B, 13))
    root[:, :, 3:7], rb[:, :, 3:7] = unit(rng.normal(size=(n, A, 4))), unit(rng.normal(size=(n, B, 4)))
    cf = rng.normal(size=(n, B, 3)) * (10.0 ** (np.arange(B) % 5 - 1))[None, :, None]
    return types.SimpleNamespace(rng=rng, dof=dof, root=root, rb=rb, cf=cf)


def finish(scene, x):
    """fp32 rounding; a box / sphere actor's rigid-body row IS its root row (the gym tensors hold the same numbers twice)"""
    x.dof, x.root, x.rb, x.cf = f32(x.dof), f32(x.root), f32(x.rb), f32(x.cf)
    for a, cfg in enumerate(scene.env_cfg):
        if cfg.type != "robot":
            x.rb[:, scene.first_rb[a]] = x.root[:, a]
    return x


def next32(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))


def groups(sizes):
    """consecutive env ranges of the given sizes -> {name: indices}; what is left of N_ENVS stays generic"""
    out, at = {}, 0
    for name, k in sizes:
        out[name] = np.arange(at, at + k)
        at += k
    assert at <= N_ENVS
    return out


def rows_a():
    rows = []
    scene, m, _ = context_a("push")
    ee, chassis, wheel = (scene.rigid_body_index("boxer", l) for l in ("ee_link", "chassis_link", "wheel_left_link"))
    robot, block, goal, obst = (scene.actor_index(a) for a in ("boxer", "block", "goal", "paper_obst1"))
    block_rb, last_rb = scene.first_rb[block], scene.n_rb - 1

    def setter(x, src, idx):
        """-> f(envs, points [len(envs)][3]) that places the operand; None for a CONST (fixed by the program)"""
        if src == RB and idx in scene.first_rb[1:]:             # a box / sphere body: its actor's root row (finish() copies it)
            return setter(x, ACTOR, scene.first_rb.index(idx))
        if src == RB:
            return lambda e, p: x.rb.__setitem__((e, idx, slice(0, 3)), p)
        if src == ACTOR:
            return lambda e, p: x.root.__setitem__((e, idx, slice(0, 3)), p)
        if src == DOF_XY:    # (q0, q1, 0)
            return lambda e, p: (x.dof.__setitem__((e, 0), p[:, 0]), x.dof.__setitem__((e, 2), p[:, 1]))
        return None

    # -- DIST: operand kinds in both positions, n = 2 and 3, a box actor's body spelled RB and ACTOR, the fp32 weight
    cpt = (1.5, -0.75, 0.25)                                       # fp32-exact: the oracle keeps constants in its own precision
    dist = [("link-actor-n2", 2, (RB, ACTOR), (ee, goal), 1.0), ("link-actor-n3", 3, (RB, ACTOR), (ee, goal), 1.0),
            ("actor-link-n3", 3, (ACTOR, RB), (block, chassis), 1.0), ("dofxy-const-n2", 2, (DOF_XY, CONST), (0, 0), 1.0),
            ("const-dofxy-n3", 3, (CONST, DOF_XY), (0, 0), 1.0), ("actor-const-n3-w", 3, (ACTOR, CONST), (robot, 0), -2.5),
            ("boxbody-rb-n3", 3, (RB, ACTOR), (block_rb, goal), 1.0), ("boxbody-actor-n3", 3, (ACTOR, ACTOR), (block, goal), 1.0)]
    for i, (name, n, src, idx, w) in enumerate(dist):
        x = base_inputs(scene, 100 if name.startswith("boxbody") else 101 + i)
        g = groups([("z-difference", 16), ("coincident", 16), ("one-ulp-apart", 16), ("400-m-out", 16)])
        sa, sb = setter(x, src[0], idx[0]), setter(x, src[1], idx[1])
        flat = DOF_XY in src                                    # (q0, q1, 0) against a constant in the plane z = 0
        const = (cpt[0], cpt[1], 0.0) if flat else cpt
        anchor = x.rng.uniform(-2.0, 2.0, (N_ENVS, 3))
        if CONST in src:
            anchor[:] = const
        anchor = f32(anchor).astype(np.float64)
        other = anchor + x.rng.uniform(-1.0, 1.0, (N_ENVS, 3))
        e = g["z-difference"]
        other[e, 2] = anchor[e, 2] + x.rng.choice([-1.0, 1.0], len(e)) * x.rng.uniform(100.0, 1000.0, len(e))
        other[g["coincident"]] = anchor[g["coincident"]]
        e = g["one-ulp-apart"]
        other[e] = anchor[e]
        other[e, 0] = next32(anchor[e, 0], True)
        e = g["400-m-out"]
        if CONST not in src:
            anchor[e, 0:2] = f32(400.0 * unit(x.rng.normal(size=(len(e), 2))))
            other[e] = anchor[e] + 0.01 * unit(x.rng.normal(size=(len(e), 3)))
        else:
            g.pop("400-m-out")                                  # (the constant is the anchor of every env of these rows)
        if flat:
            g.pop("z-difference")
        # the anchor is the constant, or operand 1; the other operand approaches it
        every = np.arange(N_ENVS)
        if src[0] == CONST:
            sb(every, other)
        elif src[1] == CONST:
            sa(every, other)
        else:
            sb(every, anchor)
            sa(every, other)
        rows.append(RowA("dist-" + name, "DIST", "push", (term(capi.OP_DIST, n, src, idx, w, const),), x.dof, x.root, x.rb, x.cf, g))
    rows[-2].bit_equal_to = rows[-1].name
    for r in rows:
        finish(scene, r)

    # -- TILT: the measurement reads the xyzw row as (r, i, j, k); both readings of "a rotation about an axis" are placed
    x = base_inputs(scene, 120)
    g = groups([("gimbal", 32), ("atan2-cut", 32), ("norm-0.5", 8), ("norm-2", 8), ("negated", 16)])

    def rot(axis, angle, reading):
        h, q = 0.5 * angle, np.zeros(4)
        if reading == "rijk":                                  # stored (x, y, z, w) = (cos, axis sin): what the measurement takes for w first
            q[0], q[1 + axis] = np.cos(h), np.sin(h)
        else:                                                  # the physical xyzw quaternion of that rotation
            q[axis], q[3] = np.sin(h), np.cos(h)
        return q
    deltas = np.logspace(-1, -3, 8)
    x.rb[g["gimbal"], ee, 3:7] = [rot(1, s * (np.pi / 2 - d), rd) for rd in ("rijk", "xyzw") for s in (1, -1) for d in deltas]
    x.rb[g["atan2-cut"], ee, 3:7] = [rot(ax, s * (np.pi - d), rd) for rd in ("rijk", "xyzw") for ax in (0, 2) for s in (1, -1) for d in np.logspace(-1, -3, 4)]
    x.rb[g["norm-0.5"], ee, 3:7] *= 0.5
    x.rb[g["norm-2"], ee, 3:7] *= 2.0
    x.rb[g["negated"][8:], ee, 3:7] = -x.rb[g["negated"][:8], ee, 3:7]
    rows.append(finish(scene, RowA("tilt-ee", "TILT", "push", (term(capi.OP_TILT, 0, (RB,), (ee,)),), x.dof, x.root, x.rb, x.cf, g)))

    # -- YAW_ABS of a free actor: unwrapped (a yaw next to pi against p[3] = -3 gives 6.14), yaw = p[3] = 0 and 1e-5 off, tilted actors
    def yaw_quat(yaw):
        return np.stack([0 * yaw, 0 * yaw, np.sin(0.5 * yaw), np.cos(0.5 * yaw)], axis=-1)
    for name, p3, w in (("wrap", -3.0, 1.0), ("zero", 0.0, -2.5)):
        x = base_inputs(scene, 130)
        g = groups([("near-pi", 16), ("at-p3", 8), ("1e-5-off-p3", 8), ("tilted", 32)])
        x.root[g["near-pi"], block, 3:7] = yaw_quat(np.concatenate([np.pi - np.logspace(-3, -5, 8), -np.pi + np.logspace(-3, -5, 8)]))
        x.root[g["at-p3"], block, 3:7] = yaw_quat(np.full(8, p3)) if p3 else np.array([0.0, 0.0, 0.0, 1.0]) * np.linspace(0.5, 2.0, 8)[:, None]
        x.root[g["1e-5-off-p3"], block, 3:7] = yaw_quat(p3 + 1e-5 * np.array([1, -1, 2, -2, 3, -3, 4, -4.0]))
        if p3:
            g.pop("at-p3")                                     # (exactly p[3] is reachable for yaw 0 only)
        g["tilted"] = np.arange(g["tilted"][0], N_ENVS)        # (every generic env: random unit quaternions)
        rows.append(finish(scene, RowA("yaw-" + name, "YAW_ABS", "push", (term(capi.OP_YAW_ABS, 0, (ACTOR,), (block,), w, (0, 0, 0, p3)),), x.dof, x.root, x.rb, x.cf, g)))

    # -- ALIGN at b = block between the rays to a = ee link and c = goal
    x = base_inputs(scene, 140)
    g = groups([("parallel", 8), ("perpendicular", 8), ("antiparallel", 8), ("1e-3-off-antiparallel", 16), ("1e-6-m-ray", 16), ("z-difference", 16),
                ("zero-ray", 16)])
    b = f32(x.rng.uniform(-2.0, 2.0, (N_ENVS, 3))).astype(np.float64)
    phi, dphi = x.rng.uniform(-np.pi, np.pi, N_ENVS), x.rng.uniform(-np.pi, np.pi, N_ENVS)
    ra, rc = x.rng.uniform(0.2, 2.0, N_ENVS), x.rng.uniform(0.2, 2.0, N_ENVS)
    dphi[g["parallel"]], dphi[g["perpendicular"]], dphi[g["antiparallel"]] = 0.0, np.pi / 2 * np.array([1, -1] * 4), np.pi
    dphi[g["1e-3-off-antiparallel"]] = np.pi + 1e-3 * np.array([1, -1] * 8)
    ra[g["1e-6-m-ray"]] = 1e-6
    ra[g["zero-ray"][:8]], rc[g["zero-ray"][8:]] = 0.0, 0.0
    z = x.rng.uniform(-1.0, 1.0, (N_ENVS, 2))
    z[g["z-difference"]] = x.rng.uniform(100.0, 1000.0, (16, 2)) * x.rng.choice([-1.0, 1.0], (16, 2))
    x.root[:, block, 0:3] = b
    x.rb[:, ee, 0:3] = b + np.stack([ra * np.cos(phi), ra * np.sin(phi), z[:, 0]], axis=-1)
    x.root[:, goal, 0:3] = b + np.stack([rc * np.cos(phi + dphi), rc * np.sin(phi + dphi), z[:, 1]], axis=-1)
    rows.append(finish(scene, RowA("align-ee-block-goal", "ALIGN", "push", (term(capi.OP_ALIGN, 0, (RB, ACTOR, ACTOR), (ee, block, goal)),),
                                   x.dof, x.root, x.rb, x.cf, g, nonfinite=g["zero-ray"])))

    # -- FORCE_L1: first / last rigid-body row, a box actor's body, a link in the middle; neighbouring rows a decade apart (base_inputs)
    for name, n, idx, w in (("first-n1", 1, 0, 1.0), ("last-n2", 2, last_rb, 1.0), ("boxbody-n3", 3, block_rb, 1.0), ("wheel-n3-w", 3, wheel, -2.5)):
        x = base_inputs(scene, 150)
        g = groups([("negative-components", 16), ("zero-force", 8)])
        x.cf[g["negative-components"], idx] = -np.abs(x.cf[g["negative-components"], idx])
        x.cf[g["zero-force"], idx] = 0.0
        g["neighbours-a-decade-apart"] = np.arange(24, N_ENVS)
        rows.append(finish(scene, RowA("force-" + name, "FORCE_L1", "push", (term(capi.OP_FORCE_L1, n, (), (idx,), w),), x.dof, x.root, x.rb, x.cf, g)))

    # -- SPEED of the robot's actor and of a free actor
    for name, n, idx in (("robot-n1", 1, robot), ("robot-n3", 3, robot), ("block-n2", 2, block), ("block-n3", 3, block)):
        x = base_inputs(scene, 160)
        g = groups([("zero-velocity", 16), ("one-component", 16)])
        x.root[g["zero-velocity"], idx, 7:10] = 0.0
        x.root[g["one-component"], idx, 7:9] = 0.0              # only z moves: n < 3 must give exactly 0
        g["generic"] = np.arange(32, N_ENVS)
        rows.append(finish(scene, RowA("speed-" + name, "SPEED", "push", (term(capi.OP_SPEED, n, (ACTOR,), (idx,)),), x.dof, x.root, x.rb, x.cf, g)))

    # -- ABS_DZ in both operand orders, BELOW of a link and of an actor: p[3] above / below / equal / 1 ulp either side
    thr = 0.3125                                                # fp32-exact
    for name, op, src, idx, klass in (("absdz-link-actor", capi.OP_ABS_DZ, (RB, ACTOR), (ee, block), "ABS_DZ"), ("absdz-actor-link", capi.OP_ABS_DZ, (ACTOR, RB), (goal, chassis), "ABS_DZ"),
                                      ("below-link", capi.OP_BELOW, (RB,), (ee,), "BELOW"), ("below-actor", capi.OP_BELOW, (ACTOR,), (block,), "BELOW")):
        x = base_inputs(scene, 170)
        g = groups([("above", 16), ("below", 16), ("equal", 8), ("one-ulp-above", 8), ("one-ulp-below", 8)])
        sa = setter(x, src[0], idx[0])
        every = np.arange(N_ENVS)
        pa = x.rng.uniform(-2.0, 2.0, (N_ENVS, 3))
        ref = np.full(N_ENVS, thr)
        if op == capi.OP_ABS_DZ:
            pb = f32(x.rng.uniform(-2.0, 2.0, (N_ENVS, 3))).astype(np.float64)
            setter(x, src[1], idx[1])(every, pb)
            ref = pb[:, 2]
        pa[g["above"], 2] = ref[g["above"]] + x.rng.uniform(0.01, 2.0, 16)
        pa[g["below"], 2] = ref[g["below"]] - x.rng.uniform(0.01, 2.0, 16)
        pa[g["equal"], 2] = ref[g["equal"]]
        pa[g["one-ulp-above"], 2] = next32(ref[g["one-ulp-above"]], True)
        pa[g["one-ulp-below"], 2] = next32(ref[g["one-ulp-below"]], False)
        sa(every, pa)
        rows.append(finish(scene, RowA(name, klass, "push", (term(op, 0, src, idx, 1.0, (0, 0, 0, thr)),), x.dof, x.root, x.rb, x.cf, g)))

    # -- MPPI_MAX_TERMS is a loop bound: sixteen terms, every op among them
    x = base_inputs(scene, 180)
    sixteen = [term(capi.OP_DIST, 2 + i % 2, (RB, CONST), (i % 8, 0), 1.0, (0.5 * i, -0.25 * i, 0.125)) for i in range(8)]
    sixteen += [term(capi.OP_TILT, 0, (RB,), (ee,)), term(capi.OP_YAW_ABS, 0, (ACTOR,), (block,), 1.0, (0, 0, 0, 0.5)),
                term(capi.OP_ALIGN, 0, (RB, ACTOR, ACTOR), (ee, block, goal)), term(capi.OP_FORCE_L1, 3, (), (scene.first_rb[obst],)), term(capi.OP_SPEED, 2, (ACTOR,), (block,)),
                term(capi.OP_DOF_SQ, 1, (), (0, 2, 2), 1.0, (0.5, -0.25)), term(capi.OP_ABS_DZ, 0, (RB, ACTOR), (ee, goal)),
                term(capi.OP_BELOW, 0, (RB,), (chassis,), 1.0, (0, 0, 0, 0.5))]
    assert len(sixteen) == capi.MAX_TERMS
    rows.append(finish(scene, RowA("sixteen-terms", "MAXTERMS", "push", tuple(sixteen), x.dof, x.root, x.rb, x.cf, {"generic": np.arange(N_ENVS)})))

    # -- DOF_SQ on the 12-DOF tree: ranges, positions / velocities, 0 / 1 / 8 references (not fp32-exact) over more than 8 joints
    scene, m, _ = context_a("anymal")
    nb = scene.n_dof
    refs = (0.1, -0.3, 0.7, 1.1, -0.9, 0.05, 1.3, -1.7)
    for name, n, lo, hi, nref in (("pos-all-ref8", 0, 0, nb, 8), ("vel-all-ref8", 1, 0, nb, 8), ("pos-3-4-ref1", 0, 3, 4, 1), ("pos-empty", 0, 5, 5, 0),
                                  ("vel-all-ref0", 1, 0, nb, 0), ("pos-all-ref1", 0, 0, nb, 1), ("vel-2-end-ref8", 1, 2, nb, 8)):
        x = base_inputs(scene, 190)
        g = {"generic": np.arange(16, N_ENVS), "on-the-references": np.arange(16)}
        for j in range(min(nref, hi - lo)):
            x.dof[:16, 2 * (lo + j) + n] = refs[j]
        rows.append(finish(scene, RowA("dofsq-" + name, "DOF_SQ", "anymal", (term(capi.OP_DOF_SQ, n, (), (lo, hi, nref), -2.5 if name == "pos-all-ref1" else 1.0, refs),),
                                       x.dof, x.root, x.rb, x.cf, g)))
    assert len({r.name for r in rows}) == len(rows)
    return rows


def reference_a(oracle, row):
    """oracle.cost on the (fp32-rounded) inputs of the row, env by env"""
    _, m, _ = context_a(row.ctx)
    cost = row.cost
    with np.errstate(all="ignore"):
        return np.array([oracle.cost(m, cost, row.root[k], row.dof[k, 0::2], row.dof[k, 1::2], row.rb[k], row.cf[k]) for k in range(N_ENVS)])


def deviation_a(ref32, ref64):
    ok = np.isfinite(ref64)
    return np.abs(ref32[ok] - ref64[ok]) / (1.0 + np.abs(ref64[ok]))


# ---- route B / C -------------------------------------------------------------------------------------------------------------------
LANE, QUAD, OCT, AUTO = "lane", "quad", "oct", ""
# MPPI_ROLLOUT -> the kernel mppi_kernel_info must name, per scene; and the settings whose kernel offers mppi_rollout_trajectory (route C)
KERNELS_B = {"arm": {LANE: "lane", QUAD: "lane", AUTO: "lane"},          # programs of contact-free scenes run on the one-lane kernel
             "push": {LANE: "scene", QUAD: "scene-quad", OCT: "scene-oct", AUTO: "scene-oct-pair"},
             "contact": {LANE: "scene", QUAD: "scene-quad", OCT: "scene-oct", AUTO: "scene-oct-pair"},
             "gripper": {AUTO: "scene-oct", LANE: "scene"},               # (light pairs take no helper wavefront)
             "jackals": {AUTO: "scene", LANE: "scene"}}                   # (only the one-lane scene kernel carries a forest)
TRAJECTORY_B = {"arm": (), "push": (OCT, AUTO), "contact": (OCT, AUTO), "gripper": (AUTO,), "jackals": ()}


@dataclasses.dataclass
class RowB:
    name: str
    t: dict                       # the term
    nominal: bool = False         # the row of its scene that runs with U != 0 (the signed control cost is present)
    exact_zero: bool = False      # a designed constant row: the measurement is exactly 0 in every sample
    constant: bool = False        # a designed constant row: nothing in it moves
    bit_equal_to: str = ""
    not_covered: tuple = ()       # mix-ups this row cannot tell apart (at most one, never an index mix-up)

    @property
    def cost(self):
        return program(self.t)


@dataclasses.dataclass
class SceneB:
    name: str
    scene: object
    m: object
    cfg: object
    dof: np.ndarray
    root: np.ndarray
    eps: np.ndarray              # [H][nu][K], fp32
    U0: np.ndarray               # the nominal of the rows marked `nominal`
    Ubase: np.ndarray            # the nominal of every other row
    rows: list
    second: dict = None          # two moving bases: {index of the second robot's row / link -> the first robot's}
    may_refuse: tuple = ()       # kernels mppi_create may refuse for this scene (LDS of the one-lane kernel)
    separate: str = "B"          # the tolerance the spread and the mix-ups of the rows are measured against (see CONTACT_NOTE)

    @property
    def K(self):
        return self.cfg.num_samples

    @property
    def kernels(self):
        return KERNELS_B[self.name]

    @property
    def trajectory(self):
        return TRAJECTORY_B[self.name]

    @property
    def origin(self):
        return self.root[self.m.robot_actor, 0:2].astype(np.float64)

    def nominal_of(self, row):
        return self.U0 if row.nominal else self.Ubase


def _prepare(cfg, oracle, scale):
    cfg.rollout_var_discount, cfg.noise_abs_cost = GAMMA, 0
    return f32(oracle.sample(cfg) * scale)


def _u0(cfg, amp, seed=0):
    return f32(amp * np.random.default_rng(seed).normal(size=(H, cfg.nu)))


@functools.lru_cache(maxsize=None)
def scene_b(name):
    from oracle.oracle import Oracle
    o = Oracle("f64")
    if name == "arm":           # contact-free: programs run on the one-lane kernel whatever MPPI_ROLLOUT says (StaticEnv)
        scene, m, cfg, _, dof, root = panda_reach(K=77, H=H)
        eps = _prepare(cfg, o, 1.0)
        tip, l4, l6 = (scene.rigid_body_index("panda", l) for l in ("panda_ee_tip", "panda_link4", "panda_link6"))
        goal = scene.actor_index("goal")
        q0 = dof[0::2]
        rows = [RowB("dist-link-actor", term(capi.OP_DIST, 3, (RB, ACTOR), (tip, goal))),
                RowB("dist-link-const", term(capi.OP_DIST, 3, (RB, CONST), (tip, 0), 1.0, (0.5, 0.25, 0.5)), nominal=True),
                RowB("tilt", term(capi.OP_TILT, 0, (RB,), (l6,))),
                RowB("dofsq-pos-ref7", term(capi.OP_DOF_SQ, 0, (), (0, 7, 7), 1.0, tuple(float(v) + 0.1 * (-1) ** j for j, v in enumerate(q0)))),
                RowB("dofsq-vel", term(capi.OP_DOF_SQ, 1, (), (1, 6, 0))),
                RowB("absdz-link-actor", term(capi.OP_ABS_DZ, 0, (RB, ACTOR), (l4, goal))),
                RowB("below-link", term(capi.OP_BELOW, 0, (RB,), (tip,), 1.0, (0, 0, 0, 0.0))),   # threshold set below, inside the spread
                RowB("force-link", term(capi.OP_FORCE_L1, 3, (), (tip,)), exact_zero=True)]
        s = SceneB(name, scene, m, cfg, f32(dof), f32(root), eps, _u0(cfg, 0.05), np.zeros((H, cfg.nu), np.float32), rows)
        z = trajectory_of(o, s, s.Ubase)["rb"][:, :, tip, 2]
        thr = float(np.float32(np.median(z)))
        assert z.min() < thr < z.max()
        rows[6].t = changed(rows[6].t, p=(0, 0, 0, thr))
        return s
    if name in ("push", "contact"):
        K = 100
        scene, m, cfg, _, dof, root = boxer_push(K=K, H=H)
        dof, root = f32(dof), f32(root)
        root[0, 2] = 0.019
        block, goal, robot = scene.actor_index("block"), scene.actor_index("goal"), scene.actor_index("boxer")
        ee, chassis, wheel, castor = (scene.rigid_body_index("boxer", l) for l in ("ee_link", "chassis_link", "wheel_left_link", "rotacastor_left_link"))
        block_rb = scene.first_rb[block]
        eps = _prepare(cfg, o, 0.3)
        if name == "push":      # the open floor of test_ragged_sizes_contact_scene: the base floats, the rollout origin is (0, 2.5)
            root[block, 0:3] = [2.5, 1.8, 0.0923]
            rows = [RowB("dist-link-const", term(capi.OP_DIST, 2, (RB, CONST), (ee, 0), 1.0, (0.5, 2.0, 0.25))),
                    # (the chassis and the block are 2.6 m apart and 7 cm apart in height: the third component moves S by 20 x the tolerance only)
                    RowB("dist-robot-block-n2", term(capi.OP_DIST, 2, (ACTOR, ACTOR), (robot, block)), not_covered=("n+1",)),
                    RowB("yaw-robot", term(capi.OP_YAW_ABS, 0, (ACTOR,), (robot,), 1.0, (0, 0, 0, 0.25))),
                    RowB("speed-robot-n2", term(capi.OP_SPEED, 2, (ACTOR,), (robot,))),
                    RowB("speed-robot-n3", term(capi.OP_SPEED, 3, (ACTOR,), (robot,))),
                    RowB("align-link-block-goal", term(capi.OP_ALIGN, 0, (RB, ACTOR, ACTOR), (ee, block, goal)), nominal=True),
                    RowB("dofsq-wheel-vel", term(capi.OP_DOF_SQ, 1, (), (0, 2, 2), 1.0, (0.3, -0.7))),
                    RowB("absdz-link-actor", term(capi.OP_ABS_DZ, 0, (RB, ACTOR), (ee, goal))),
                    RowB("below-link", term(capi.OP_BELOW, 0, (RB,), (ee,), 1.0, (0, 0, 0, 0.5))),
                    RowB("dist-blockbody-goal-rb", term(capi.OP_DIST, 3, (RB, ACTOR), (block_rb, goal)), bit_equal_to="dist-blockbody-goal-actor", constant=True),
                    RowB("dist-blockbody-goal-actor", term(capi.OP_DIST, 3, (ACTOR, ACTOR), (block, goal)), constant=True)]   # (nothing reaches the block on the open floor)
            return SceneB(name, scene, m, cfg, dof, root, eps, _u0(cfg, 0.2), np.zeros((H, 2), np.float32), rows)
        root[block, 0:3] = [0.0, 2.05, 0.0923]                  # 0.45 m in front of the chassis: every sample loads the block from the first step
        U = np.zeros((H, 2), np.float32)
        U[:, 0] = 0.5
        rows = [RowB("force-block-n1", term(capi.OP_FORCE_L1, 1, (), (block_rb,))),
                RowB("force-block-n3", term(capi.OP_FORCE_L1, 3, (), (block_rb,))),
                RowB("force-chassis-n3", term(capi.OP_FORCE_L1, 3, (), (chassis,))),
                # (the ee link carries no shape; its neighbours in the force rows - the left wheel, the block - are loaded.  U != 0 here, so S is
                #  the control cost: an empty DOF_SQ range gives the same S bit for bit iff the force term adds exactly 0)
                RowB("force-untouched-n3", term(capi.OP_FORCE_L1, 3, (), (ee,)), exact_zero=True, bit_equal_to="empty-dofsq"),
                RowB("empty-dofsq", term(capi.OP_DOF_SQ, 0, (), (1, 1, 0)), exact_zero=True)]
        return SceneB(name, scene, m, cfg, dof, root, eps, U, U, rows, separate="C")
    if name == "gripper":
        K = 40
        scene, m, cfg, _, _, _ = panda_pick(K=K, H=H)
        Z = np.load(GOLDEN_STATES)
        dof, root = f32(Z["panda_pick_held_dof"]), f32(Z["panda_pick_held_root"])
        eps = _prepare(cfg, o, 1.0)
        ee, lf, rf = (scene.rigid_body_index("panda", l) for l in ("panda_ee", "panda_leftfinger", "panda_rightfinger"))
        block = scene.actor_index("panda_pick_block")
        block_rb = scene.first_rb[block]
        q0 = dof[0::2]
        rows = [RowB("force-leftfinger", term(capi.OP_FORCE_L1, 3, (), (lf,))),
                RowB("force-rightfinger", term(capi.OP_FORCE_L1, 3, (), (rf,))),
                RowB("force-block", term(capi.OP_FORCE_L1, 3, (), (block_rb,))),
                # (panda_link7 and panda_ee are welded to one body with the same orientation: TILT cannot tell them apart, the DIST row below can)
                RowB("tilt-ee", term(capi.OP_TILT, 0, (RB,), (ee,)), not_covered=("operand0-1",)),
                RowB("dist-ee-block", term(capi.OP_DIST, 3, (RB, ACTOR), (ee, block)), nominal=True),
                RowB("dofsq-pos-all-ref8", term(capi.OP_DOF_SQ, 0, (), (0, 9, 8), 1.0, tuple(float(v) + 0.1 * (-1) ** j for j, v in enumerate(q0[:8]))))]
        return SceneB(name, scene, m, cfg, dof, root, eps, _u0(cfg, 0.05), np.zeros((H, cfg.nu), np.float32), rows,
                      may_refuse=(LANE,), separate="C")
    if name == "jackals":
        from mppiisaac.planner.mppi import MPPIConfig, make_config
        K = 24
        scene = build_scene(["jackal_a", "jackal_b", "goal"], [[0.0, 0.0, 0.1], [0.5, -2.0, 0.1]])
        m = scene.to_c()
        cfg = make_config(MPPIConfig(num_samples=K, horizon=H, noise_sigma=np.eye(4).tolist(), lambda_=0.01, u_min=[-1.5], u_max=[1.5],
                                     sample_null_action=True), viz_link=scene.viz_link_index())
        dof, root = scene.initial_state()
        dof, root = f32(dof), f32(root)
        root[0:2, 2] = 0.0616                                   # on their wheels, as the step matrix starts them
        eps = _prepare(cfg, o, 1.0)
        a, b, goal = (scene.actor_index(n) for n in ("jackal_a", "jackal_b", "goal"))
        wa, wb = scene.rigid_body_index("jackal_a", "front_left_wheel_link"), scene.rigid_body_index("jackal_b", "front_left_wheel_link")
        ca, cb = scene.rigid_body_index("jackal_a", "rear_right_wheel_link"), scene.rigid_body_index("jackal_b", "rear_right_wheel_link")
        rows = [RowB("dist-second-actor-const", term(capi.OP_DIST, 2, (ACTOR, CONST), (b, 0), 1.0, (1.0, -1.5, 0.0)), nominal=True),
                RowB("yaw-second", term(capi.OP_YAW_ABS, 0, (ACTOR,), (b,), 1.0, (0, 0, 0, 0.25))),
                RowB("speed-second-n2", term(capi.OP_SPEED, 2, (ACTOR,), (b,))),
                RowB("dist-second-wheel-goal", term(capi.OP_DIST, 3, (RB, ACTOR), (wb, goal))),
                RowB("dist-second-rearwheel-goal", term(capi.OP_DIST, 2, (RB, ACTOR), (cb, goal)))]
        return SceneB(name, scene, m, cfg, dof, root, eps, _u0(cfg, 0.2), np.zeros((H, 4), np.float32), rows,
                      second={("actor", b): a, ("rb", wb): wa, ("rb", cb): ca})
    raise KeyError(name)


SCENES_B = ("arm", "push", "contact", "gripper", "jackals")


def controls(s, U, eps=None):
    """-> (u [H][K][nu] the clamped controls, du = u - U, the fp64 control cost lambda sum U du / sigma) of every sample (oracle's rollout_one)"""
    cfg, K, nu = s.cfg, s.K, s.cfg.nu
    eps = s.eps if eps is None else eps
    lo, hi = np.array([cfg.u_min[j] for j in range(nu)]), np.array([cfg.u_max[j] for j in range(nu)])
    v = U.astype(np.float64)[:, :, None] + eps.astype(np.float64)
    if cfg.sample_null_action:
        v[:, :, K - 1] = 0.0
    assert not cfg.use_priors and cfg.k_offset == 0 and not cfg.noise_abs_cost
    u = np.clip(v, lo[None, :, None], hi[None, :, None])
    du = u - U.astype(np.float64)[:, :, None]
    return u.transpose(0, 2, 1), du, control_cost(s, U, du)


def control_cost(s, U, du):
    sig = np.array([s.cfg.noise_sigma_diag[j] for j in range(s.cfg.nu)])
    return s.cfg.lambda_ * (U.astype(np.float64)[:, :, None] * np.asarray(du, np.float64) / sig[None, :, None]).sum(axis=(0, 1))


_TRAJ = {}


def trajectory_of(o, s, U):
    """the oracle's own rollout, states kept: dof [H][K][2n], root [H][K][A][13], rb [H][K][B][13], cf [H][K][B][3], ctrl [K]"""
    key = (s.name, o.dtype, U.tobytes())
    if key in _TRAJ:
        return _TRAJ[key]
    m, K, n = s.m, s.K, s.m.n_bodies
    u, du, ctrl = controls(s, U)
    T = {"dof": np.zeros((H, K, 2 * n)), "root": np.zeros((H, K, m.n_actors, 13)), "rb": np.zeros((H, K, m.n_rb, 13)), "cf": np.zeros((H, K, m.n_rb, 3)),
         "ctrl": ctrl}
    is_scene = o.is_scene(m)
    for k in range(K):
        root, q, qd = s.root.astype(np.float64), s.dof[0::2].astype(np.float64), s.dof[1::2].astype(np.float64)
        for t in range(H):
            target = o.cmd_map(m, u[t, k])
            if is_scene:
                root, q, qd, cf = o.scene_step(m, root, q, qd, target)
                T["cf"][t, k] = cf
            else:
                q, qd = o.step(m, root, q, qd, target)
            rb, _ = o.rigid_body_state(m, root, q, qd)
            T["dof"][t, k, 0::2], T["dof"][t, k, 1::2], T["root"][t, k], T["rb"][t, k] = q, qd, root, rb
    _TRAJ[key] = T
    return T


def rollout_costs_on(o, m, cost, T, gamma=GAMMA, transpose_links=False):
    """S[k] = sum_t gamma^t o.cost(program, state_tk) + ctrl[k] on GIVEN states (route C's reference; the mix-ups of the separation test)"""
    Hh, K = T["dof"].shape[:2]
    rb = T["rb"]
    if transpose_links:          # the link rotations transposed (cos and sin of a planar rotation swapped): conjugate quaternions
        rb = rb.copy()
        rb[..., 3:6] *= -1.0
    S = np.array(T["ctrl"], np.float64).copy()
    with np.errstate(all="ignore"):
        for k in range(K):
            for t in range(Hh):
                S[k] += gamma ** t * o.cost(m, cost, T["root"][t, k], T["dof"][t, k, 0::2], T["dof"][t, k, 1::2], rb[t, k], T["cf"][t, k])
    return S


def tolerance_b(S32, S64):
    """-> (relative to max |S|, absolute) tolerance of a route B row from the two oracle builds' rollouts"""
    top = np.abs(S64).max()
    if top == 0.0:
        return 0.0, 0.0
    rel = max(FLOOR, round_up_125(10.0 * np.abs(S32 - S64).max() / top))
    return rel, rel * top


def mixups(s, row):
    """the plausible plumbing errors of a row, each as (name, kind, changed term, keyword changes of rollout_costs_on)"""
    t, out = row.t, []
    op = t["op"]
    nmax = {capi.OP_DIST: (2, 3), capi.OP_FORCE_L1: (1, 3), capi.OP_SPEED: (1, 3)}.get(op)
    if nmax:
        for d in (-1, 1):
            if nmax[0] <= t["n"] + d <= nmax[1]:
                out.append((f"n{d:+d}", "n", changed(t, n=t["n"] + d), {}))
    A, B, nb = s.m.n_actors, s.m.n_rb, s.m.n_bodies
    if op == capi.OP_DOF_SQ:
        lo, hi, nref = t["idx"]
        for d in (-1, 1):
            if 0 <= lo + d <= hi:
                out.append((f"lo{d:+d}", "index", with_idx(t, 0, lo + d), {}))
            if lo <= hi + d <= nb:
                out.append((f"hi{d:+d}", "index", with_idx(t, 1, hi + d), {}))
        if nref:
            p = list(t["p"]) + [0.0] * (8 - len(t["p"]))
            out.append(("ref-1", "index", changed(t, p=tuple([p[7]] + p[:7])), {}))     # reference j - 1
    elif op == capi.OP_FORCE_L1:
        for d in (-1, 1):
            if 0 <= t["idx"][0] + d < B:
                out.append((f"rb{d:+d}", "index", with_idx(t, 0, t["idx"][0] + d), {}))
    else:
        for a, src in enumerate(t["src"]):
            lim = {RB: B, ACTOR: A}.get(src)
            if lim:
                for d in (-1, 1):
                    if 0 <= t["idx"][a] + d < lim:
                        out.append((f"operand{a}{d:+d}", "index", with_idx(t, a, t["idx"][a] + d), {}))
    if CONST in t["src"] and np.abs(s.origin).max() > 0 and op in (capi.OP_DIST, capi.OP_ALIGN):
        p = list(t["p"])
        p[0], p[1] = p[0] + s.origin[0], p[1] + s.origin[1]
        out.append(("const-unshifted", "origin", changed(t, p=tuple(p)), {}))
    if s.second:
        tt = t
        for a, src in enumerate(t["src"]):
            key = ("actor" if src == ACTOR else "rb", t["idx"][a])
            if src in (RB, ACTOR) and key in s.second:
                tt = with_idx(tt, a, s.second[key])
        if tt is not t:
            out.append(("first-robot", "index", tt, {}))
    if op == capi.OP_TILT:
        out.append(("rotation-transposed", "rotation", t, dict(transpose_links=True)))
    if not row.exact_zero:
        out.append(("discount-1", "discount", t, dict(gamma=1.0)))
    return out


# Scenes that start IN contact (`separate == "C"`): 10 x the deviation of the two oracle builds' ROLLOUTS is 1e-2 .. 2 of max |S| there
# (a contact that closes a substep apart), so no mix-up can move a sample by 100 x route B's tolerance.  Route B holds these rows to
# that loose bound on every kernel; what separates their mix-ups is route C's tolerance (costs on given states), and the non-GPU
# test measures the spread and the separation of these rows against THAT tolerance, computed on the oracle's own trajectory.
CONTACT_NOTE = "spread and mix-ups measured against route C's tolerance"


def tolerance_c(S32, S64):
    """per sample: 10 x the worst deviation of the two oracle builds' costs on the SAME states, never below route A's rtol = atol = 2e-6"""
    return np.maximum(10.0 * np.abs(S32 - S64).max(), FLOOR * (1.0 + np.abs(S64)))


@functools.lru_cache(maxsize=None)
def references_b(name):
    """row name -> (S of oracle64.rollout, relative and absolute tolerance from oracle32.rollout, tolerance of route C on the oracle's states)"""
    from oracle.oracle import Oracle
    o64, o32 = Oracle("f64"), Oracle("f32")
    s, out = scene_b(name), {}
    for row in s.rows:
        U = s.nominal_of(row)
        S64, _, _ = o64.rollout(s.m, s.cfg, row.cost, s.dof, s.root, U, s.eps)
        S32, _, _ = o32.rollout(s.m, s.cfg, row.cost, s.dof, s.root, U, s.eps)
        rel, tol = tolerance_b(S32, S64)
        T = trajectory_of(o64, s, U)
        Sp = rollout_costs_on(o64, s.m, row.cost, T)
        tol_c = tolerance_c(rollout_costs_on(o32, s.m, row.cost, T), Sp)
        out[row.name] = types.SimpleNamespace(S=S64, S32=S32, rel=rel, tol=tol, S_states=Sp, tol_c=tol_c)
    return out
