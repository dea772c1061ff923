"""Inputs of the per-env state tests (test_per_env_states.py, no GPU; test_gpu_per_env_states.py): every env of a batched simulator
starts from its OWN state, written with mppi_sim_set_states* (csrc/mppi_kernels.hpp k_sim_set_states, k_sim_set_states_scene), and
is then stepped with its own commands against the fp64 oracle's orc_envs_step.

Scenes, commands, tolerances and the comparison are those of test_gpu_step_matrix.py (build, commands, TOL, compare): nothing is
asserted more loosely here.  What is new is the START of every env, drawn per (env, column) from default_rng(SEED_STARTS):
  panda    joints +-0.2 rad, joint rates +-0.2 rad/s
  boxer    (start of E-boxer) base xy +-0.03 m, yaw +-0.1 rad, joint rates +-0.1 rad/s, block xy +-0.02 m
  jackals  (on their wheels) both bases as the boxer's, joint rates +-0.1 rad/s
  pick     (recorded closed-loop state) arm joints +-0.005 rad, block +-1 mm, block velocity +-0.01 m/s
A yaw is COMPOSED with the row's quaternion (unit to rounding), never added to components.  An env's start does not depend on how
many envs there are (the draws are made for KMAX envs and cut), so one oracle run at KMAX serves every K.

The seeds are inputs chosen on the oracle (test_per_env_states.py: the fp32 oracle has to stay within a TENTH of every tolerance on
every env at every step): SEED_STARTS for the starts, SEED_OTHER for the second set of starts that the indexed calls write over
the first (only its rows of the envs of touched() are used).  Of the seeds 109 .. 123, with the draw order of starts() and all 80
envs, two meet the condition in all four scenes (113: worst share of a tolerance 0.084 panda, 0.081 boxer, 0.059 jackals, 0.042
pick; 117: 0.085 / 0.096 / 0.045 / 0.052); the pushing scene is the one that decides (0.10 .. 0.16 under the thirteen others, in
the wheel angles), the arm exceeds a tenth under six of them (up to 0.41)."""
import ctypes as C

import numpy as np

from mppiisaac.backend import capi
from test_gpu_step_matrix import KMAX, Case, build, commands

SEED_STARTS, SEED_OTHER = 113, 119

# the step cases: (scene, K, step kernel mppi_kernel_info must name); contact-free scenes N = 6 steps, contact scenes N = 4
STEP_CASES = [Case(f"panda-K{K}", "panda", K, "quad" if K == 1 or K >= 64 else "lane") for K in (1, 17, 63, 64, 65, 80)]
STEP_CASES += [Case(f"boxer-K{K}", "boxer", K, "scene-quad", N=4) for K in (7, 65)]
STEP_CASES += [Case(f"boxer-K{K}-rollout-lane", "boxer", K, "scene", N=4, env=(("MPPI_ROLLOUT", "lane"),)) for K in (7, 65)]
STEP_CASES += [Case(f"pick-K{K}", "pick", K, "scene-quad", N=4) for K in (7, 65)]
STEP_CASES += [Case("pick-K7-rollout-lane", "pick", 7, "scene", N=4, env=(("MPPI_ROLLOUT", "lane"),), may_refuse=True)]
STEP_CASES += [Case(f"jackals-K{K}", "jackals", K, "scene", N=4) for K in (5, 65)]
STEP_IDS = [c.name for c in STEP_CASES]
# set -> materialise, no step
ROUND_TRIP = [("panda", K) for K in (1, 2, 17, 63, 64, 65, 80)] + [("boxer", K) for K in (1, 7, 17, 65)] + [("pick", K) for K in (7, 65)] \
    + [("jackals", K) for K in (5, 65)]
# indexed calls: these envs of K = 65 and 80 (as a set: K - 1 is 64 at K = 65), given in a shuffled order
INDEXED = [("panda", 65), ("panda", 80), ("boxer", 65), ("boxer", 80)]
SCENES = ("panda", "boxer", "jackals", "pick")
_STEPS = {"panda": 6, "boxer": 4, "jackals": 4, "pick": 4}


def touched(K):
    ids = sorted({0, 15, 16, 63, 64, K - 1})
    return [ids[i] for i in np.random.default_rng(K).permutation(len(ids))]


def scene_case(scene, K=KMAX):
    """the step-matrix case whose scene, start and commands the per-env tests of `scene` use"""
    return Case(f"{scene}-K{K}", scene, K, "", N=_STEPS[scene])


def per_env_actors(m):
    """actors whose root row is per env: the moving bases of the forest and the free (non-fixed, non-robot) actors - mppi_hip.h"""
    moving = [] if m.actors[m.robot_actor].fixed else [m.robot_actor] + [m.extra_base_actor[r] for r in range(m.n_extra_bases)]
    return moving + [a for a in range(m.n_actors) if a != m.robot_actor and not m.actors[a].fixed and m.actors[a].type != capi.ACTOR_ROBOT]


def yawed(row, angle):
    """root row with a rotation by `angle` about the world's z composed onto its quaternion (xyzw), fp64"""
    x, y, z, w = row[3:7]
    s, c = np.sin(angle / 2), np.cos(angle / 2)
    out = row.copy()
    out[3:7] = [c * x - s * y, c * y + s * x, c * z + s * w, c * w - s * z]
    return out


_STARTS = {}


def starts(scene, seed=SEED_STARTS):
    """-> (b of build(), dof [KMAX][2n] fp32, root [KMAX][A][13] fp32): the per-env start states, kept unchanged.  The rows of the
    actors that are not per env are the shared rows of b.root in every env."""
    if (scene, seed) not in _STARTS:
        b = build(scene_case(scene))
        m, rng = b.m, np.random.default_rng(seed)
        n, A = m.n_bodies, m.n_actors
        dof = np.tile(b.dof.astype(np.float64).reshape(1, 2 * n), (KMAX, 1))
        root = np.tile(b.root.astype(np.float64).reshape(1, A, 13), (KMAX, 1, 1))
        U = lambda amp, *shape: rng.uniform(-amp, amp, size=(KMAX,) + shape)
        if scene == "panda":
            dof[:, 0::2] += U(0.2, n)
            dof[:, 1::2] += U(0.2, n)
        elif scene == "pick":
            arm = 7
            dof[:, 0:2 * arm:2] += U(0.005, arm)
            blk = b.scene.actor_index("panda_pick_block")
            root[:, blk, 0:3] += U(0.001, 3)
            root[:, blk, 7:10] += U(0.01, 3)
        else:
            bases = per_env_actors(m)[:1 + m.n_extra_bases]
            for a in bases:
                root[:, a, 0:2] += U(0.03, 2)
                yaw = U(0.1)
                for k in range(KMAX):
                    root[k, a] = yawed(root[k, a], yaw[k])
            dof[:, 1::2] += U(0.1, n)
            if scene == "boxer":
                root[:, b.scene.actor_index("block"), 0:2] += U(0.02, 2)
        dof, root = np.ascontiguousarray(dof, np.float32), np.ascontiguousarray(root, np.float32)
        dof.setflags(write=False)
        root.setflags(write=False)
        _STARTS[(scene, seed)] = (b, dof, root)
    return _STARTS[(scene, seed)]


def oracle_steps_from(o, m, dof0, root0, u, g0=0):
    """orc_envs_step from the per-env states dof0 [K][2n], root0 [K][A][13] with u [N][K][nu] -> the four tensors after every
    step, [N][K]... in fp64"""
    f = o.dtype
    N, K = u.shape[0], u.shape[1]
    dof, root = np.ascontiguousarray(dof0[:K], f), np.ascontiguousarray(root0[:K], f)
    rb, cf = np.zeros((K, m.n_rb, 13), f), np.zeros((K, m.n_rb, 3), f)
    out = {"dof": [], "root": [], "rb": [], "cf": []}
    for t in range(N):
        ut = np.ascontiguousarray(u[t], f)
        o.lib.orc_envs_step(C.byref(m), C.c_int(K), C.c_int(g0), o.p(ut), o.p(dof), o.p(root), o.p(rb), o.p(cf))
        for key, v in (("dof", dof), ("root", root), ("rb", rb), ("cf", cf)):
            out[key].append(v.copy())
    return {k: np.stack(v).astype(np.float64) for k, v in out.items()}


_REFS = {}


def reference(o, scene, K=KMAX):
    """the oracle's states of envs 0 .. K-1 of `scene` after every step, from the per-env starts under the per-env commands of
    the step matrix: one run at KMAX per scene and precision (the envs are independent), kept unchanged"""
    key = (o.dtype, scene)
    if key not in _REFS:
        b, dof, root = starts(scene)
        _REFS[key] = oracle_steps_from(o, b.m, dof, root, commands(scene_case(scene), b.m.nu, KMAX))
        for v in _REFS[key].values():
            v.setflags(write=False)
    return {k: v[:, :K] for k, v in _REFS[key].items()}


def mixed_starts(scene, K):
    """the starts after an indexed call: the envs of touched(K) from the SECOND set of starts, every other env from the first"""
    _, dof, root = starts(scene)
    _, dof2, root2 = starts(scene, SEED_OTHER)
    ids = touched(K)
    dof, root = dof[:K].copy(), root[:K].copy()
    dof[ids], root[ids] = dof2[ids], root2[ids]
    return ids, dof, root


def reference_mixed(o, scene, K):
    """... and the oracle's states from them: the touched envs are stepped anew (with their own commands), the others are
    those of reference()"""
    key = (o.dtype, scene, "mixed", K)
    if key not in _REFS:
        b = starts(scene)[0]
        ids, dof, root = mixed_starts(scene, K)
        ref = {k: v.copy() for k, v in reference(o, scene, K).items()}
        u = commands(scene_case(scene), b.m.nu, KMAX)
        new = oracle_steps_from(o, b.m, dof[ids], root[ids], np.ascontiguousarray(u[:, ids]))
        for k in ref:
            ref[k][:, ids] = new[k]
        _REFS[key] = ref
    return _REFS[key]
