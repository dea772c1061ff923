"""The no-GPU half of the link-acceleration / wrench-force tests (inputs, references, metrics and tolerances:
link_acceleration_cases.py; the kernels on the GPU: test_gpu_link_acceleration.py).

 * the two entries are exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states their conventions,
   the wrapper has the accessors; ABI stays 9;
 1 the references check themselves: the two Richardson levels of (Jdot qd)_ref agree within 1e-8; with qd = 0 the reference is J_ref qdd;
   each part moves some entry by at least 100 tolerances; the fp32 restatement the tolerances come from sits within a tenth of them;
 2 an analytic answer that needs no oracle: the Panda with only its first (vertical) joint turning at w - every link accelerates by
   -w^2 r_perp, its angular acceleration is zero;
 3 the device routines (csrc/mppi_device.hpp), compiled for the host, meet the tolerances for every robot at every base pose, all four
   acceleration calls and the wrench call, and on the forest of two point robots; the promised exact zeros; a part left out by its bit
   is the part left out by a zeroed input, bit for bit, and the separate calls sum to the full one; body ranges are slices of the
   whole range, bit for bit;
 4 the `far` row of the mobile manipulator (prismatic base joints 420 m out) meets the tolerance of its `origin` row ALONE;
 5 wrenches: a NaN in an ignored row leaves tau unchanged; tau . qd = sum w . (J_ref qd); a unit wrench e_j on link b gives row j of
   J_ref,b;
 6 the host build refuses what the library refuses - a model that does not pack, a moving base, a tree that is not instantiated, bits
   other than MPPI_ID_VELOCITY in terms, null pointers, a range outside [0, n_rb) - without writing.
The four planted defects of the device routines (w x (w x r) of the link offset dropped, the prismatic 2 w x (qd a) dropped, d x F
dropped in the inward pass, the link's own lever r x f dropped) were each shown to fail row 3 on a scratch copy of the host build:
profiles/r17a_planted_defects.txt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import inverse_dynamics_cases as ic
import jacobian_cases as jc
import link_acceleration_cases as lc
from mppiisaac.backend import capi
from scenes import build_scene

ROBOT_IDS = list(lc.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
V = lc.ID_VELOCITY
_vp, _i = C.c_void_p, C.c_int


def test_the_entries_are_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_link_acceleration"] == (_i, [_vp, _i, _i, _vp, _i, _vp])
    assert capi._SIGNATURES["mppi_sim_wrench_forces"] == (_i, [_vp, _i, _i, _vp, _vp])
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    for name in ("mppi_sim_link_acceleration", "mppi_sim_wrench_forces"):
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)
        assert f"int {name}(" in header
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    said = header[header.index("How a link ACCELERATES"):header.index("int mppi_sim_link_acceleration(")]
    for words in ("world axes", "rows 0-2 linear", "rigid-body index", "zero Jacobians", "qdd_dev is NULL", "MPPI_ID_VELOCITY", "MPPI_ID_GRAVITY",
                  "exact zeros", "exact zero rows", "must not overlap", "moment about the link frame origin", "ADD", "SUBTRACT", "IGNORED",
                  "NOT in either", "no drives, no limits, no contact forces", "not a wrench", "captured graph", "MOVING base", "Refused before"):
        assert words in said, words
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("link_accelerations", "get_actor_link_acceleration_by_name", "acquire_link_bias_acceleration_tensor",
                 "refresh_link_bias_acceleration_tensors", "joint_forces_from_wrenches", "joint_forces_from_link_wrench"):
        assert callable(getattr(IsaacGymWrapper, name))


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_link_acceleration")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "liblink_acceleration_hostemu.so"))


def host_acc(lib, model, root, dof, qdd, terms, with_qdd, rb_first=0, rb_count=None):
    K = len(dof)
    rb_count = int(model.n_rb) - rb_first if rb_count is None else rb_count
    root32 = np.ascontiguousarray(root, np.float32)
    q, qd, a = (np.ascontiguousarray(x, np.float32) for x in (dof[:, 0::2], dof[:, 1::2], qdd))
    acc = np.full((K, rb_count, 6), np.nan, np.float32)
    assert lib.emu_link_acceleration(C.byref(model), K, fp(root32), fp(q), fp(qd), rb_first, rb_count, fp(a) if with_qdd else None, terms, fp(acc)) == 0
    assert np.isfinite(acc).all()
    return acc


def host_tau(lib, model, root, dof, w, rb_first=0, finite=True):
    K, n = len(dof), dof.shape[1] // 2
    root32 = np.ascontiguousarray(root, np.float32)
    q, w = np.ascontiguousarray(dof[:, 0::2], np.float32), np.ascontiguousarray(w, np.float32)
    tau = np.full((K, n), np.nan, np.float32)
    assert lib.emu_wrench_forces(C.byref(model), K, fp(root32), fp(q), rb_first, w.shape[1], fp(w), fp(tau)) == 0
    assert np.isfinite(tau).all()
    return tau


@pytest.fixture(scope="module")
def host_results(hostemu):
    """{(robot, pose): ({call: acc [K][n_rb][6]}, tau [K][n])} of the host build: computed once, shared, read-only"""
    out = {}
    for robot in ROBOT_IDS:
        for pose in lc.POSES[robot]:
            r = lc.references(robot, pose)
            dof, qdd, w = lc.inputs(robot, pose)
            acc = {call: host_acc(hostemu, r.model, r.root, dof, qdd, *call) for call in lc.ACC_CALLS}
            tau = host_tau(hostemu, r.model, r.root, dof, w)
            for a in list(acc.values()) + [tau]:
                a.setflags(write=False)
            out[robot, pose] = (acc, tau)
    return out


def measure(acc, tau, r):
    """-> ({call: (e_lin, e_ang)}, e_tau)"""
    return {c: lc.e_acc(acc[c], lc.combine(r.parts, *c), r.D) for c in acc}, lc.e_tau(tau, r.tau_ref, r.Dj)


def report(tag, e, et, tols):
    print(f"\n[{tag}] e_lin / e_ang per (terms, qdd given) (tol {tols[0]:.0e} / {tols[1]:.0e}): " + ", ".join(f"{c}: {a:.1e} / {b:.1e}" for c, (a, b) in e.items())
          + f"; e_tau {et:.1e} (tol {tols[2]:.0e})")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. the references check themselves ---------------------------------------------------------------------------------------------
# the angular Jdot qd of the two planar bases (x, y, one yaw joint) is identically zero: asserted on the linear rows only there
PLANAR = ("point_robot", "heijn")


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_references_are_well_posed(robot, oracle64):
    tols = lc.tolerances(robot)
    worst = lc.restatement_worst(robot)
    assert all(0.0 < t <= lc.CAP for t in tols)
    assert all(w <= 0.1 * t for w, t in zip(worst, tols))         # the rule: ten times the restatement's own deviation, rounded up
    moved = {"J qdd lin": 0.0, "J qdd ang": 0.0, "Jdot qd lin": 0.0, "Jdot qd ang": 0.0}
    for pose in lc.POSES[robot]:
        r = lc.references(robot, pose)
        dof, qdd, w = lc.inputs(robot, pose)
        assert len(dof) == lc.ROBOTS[robot][3] and w.shape == (len(dof), r.model.n_rb, 6)
        assert np.abs(w[:, :, :3]).max() <= lc.FORCE_AMP and np.abs(w[:, :, 3:]).max() <= lc.MOMENT_AMP and np.abs(w[:, :, 3:]).max() > 0.9 * lc.MOMENT_AMP
        assert r.parts["gap"] <= lc.RICHARDSON_AGREE              # the two Richardson levels
        assert all(np.isfinite(a).all() for a in (r.J, r.parts["A"], r.parts["V"], r.tau_ref)) and min(r.D) > 0.0 and (r.Dj > 0.0).all()
        # with qd = 0 the reference is J_ref qdd
        still = np.array(dof[:8])
        still[:, 1::2] = 0.0
        _, p0 = lc.reference_parts(oracle64, r.model, r.root, still[:, 0::2], still[:, 1::2], qdd[:8])
        assert not p0["V"].any() and np.array_equal(lc.combine(p0, *lc.FULL), r.parts["A"][:8])
        # the exactly-zero rows: the links welded to the base, and nothing else of a robot-only scene
        welded = np.array([L["body"] < 0 for L in r.scene.robot_model["links"]])
        assert np.array_equal(r.zero[r.first:r.first + r.L], welded) and r.zero.sum() == welded.sum()
        for part, name in (("A", "J qdd"), ("V", "Jdot qd")):
            moved[name + " lin"] = max(moved[name + " lin"], float(np.abs(r.parts[part][:, :, 0:3]).max() / r.D[0] / tols[0]))
            moved[name + " ang"] = max(moved[name + " ang"], float(np.abs(r.parts[part][:, :, 3:6]).max() / r.D[1] / tols[1]))
        print(f"\n[{robot} {pose}] K {len(dof)}: Richardson levels differ by {r.parts['gap']:.1e}; D_lin {r.D[0]:.2f} D_ang {r.D[1]:.2f}; D_j "
              f"{np.array2string(r.Dj, precision=2)}; restatement e_lin {r.w32[0]:.1e} e_ang {r.w32[1]:.1e} e_tau {r.w32[2]:.1e} (tol "
              + " / ".join(f"{t:.0e}" for t in tols) + ")")
    print(f"[{robot}] parts move some entry by, in tolerances: " + ", ".join(f"{k} {v:.0f}" for k, v in moved.items()))
    for k, v in moved.items():
        if k == "Jdot qd ang" and robot in PLANAR:
            continue
        assert v >= 100.0, f"{robot}: {k} moves no entry by 100 tolerances ({v:.0f})"


# ---- 2. an analytic answer ----------------------------------------------------------------------------------------------------------
def test_first_joint_turning_is_centripetal(hostemu):
    """the Panda's first joint is vertical through the base at the origin: with it alone turning at w, every link origin moves on a
    horizontal circle - a = -w^2 r_perp, r_perp the horizontal part of the link position (an fp64 forward-kinematics pass over the JSON
    model, no oracle) - and nothing accelerates in angle"""
    r = lc.references("franka_panda")
    mj = r.scene.robot_model
    assert mj["bodies"][0]["axis"] == [0.0, 0.0, 1.0] and mj["bodies"][0]["parent"] == -1 and not np.asarray(r.root)[0, 0:2].any()
    dof0 = lc.inputs("franka_panda")[0]
    K, n = 16, dof0.shape[1] // 2
    omega = 2.0
    dof = np.array(dof0[:K])
    dof[:, 1::2] = 0.0
    dof[:, 1] = omega
    got = host_acc(hostemu, r.model, r.root, dof, np.zeros((K, n), np.float32), V, False)
    want = np.zeros((K, len(mj["links"]), 3))
    for k in range(K):
        R, p, Rw = lc._body_frames(mj, np.eye(3), dof[k, 0::2].astype(np.float64), np.float64)
        pw = [None] * n
        for i, b in enumerate(mj["bodies"]):
            pw[i] = (np.asarray(r.root, np.float64)[0, 0:3] if b["parent"] < 0 else pw[b["parent"]]) + (np.eye(3) if b["parent"] < 0 else Rw[b["parent"]]) @ p[i]
        for l, L in enumerate(mj["links"]):
            if L["body"] >= 0:
                pos = pw[L["body"]] + Rw[L["body"]] @ np.asarray(L["p"], np.float64)
                want[k, l] = -omega ** 2 * np.array([pos[0], pos[1], 0.0])
    tl, ta, _ = lc.tolerances("franka_panda")
    links = got[:, r.first:r.first + r.L]
    e = np.abs(links[:, :, 0:3] - want).max() / np.abs(want).max()
    print(f"\n[first joint at {omega} rad/s] largest |a| {np.abs(want).max():.3f} m/s^2; e_lin on that scale {e:.1e} (tol {tl:.0e}); largest angular {np.abs(links[:, :, 3:]).max():.1e}")
    assert np.abs(want).max() > 1.0 and e <= tl
    assert np.abs(links[:, :, 3:6]).max() <= ta * omega ** 2


# ---- 3. the tolerances, all calls ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_functions_on_the_host_meet_the_tolerances(robot, host_results, hostemu):
    tols = lc.tolerances(robot)
    for pose in lc.POSES[robot]:
        r = lc.references(robot, pose)
        acc, tau = host_results[robot, pose]
        e, et = measure(acc, tau, r)
        report(f"{robot} {pose} host build", e, et, tols)
        assert max(a for a, _ in e.values()) <= tols[0] and max(b for _, b in e.values()) <= tols[1] and et <= tols[2]
        # the promised exact zeros, bit for bit: nothing asked for; the bodies without a Jacobian in every call
        assert not bits(acc[(0, False)]).any()
        assert r.zero.any() and all(not bits(a[:, r.zero]).any() for a in acc.values())
        # the separate calls sum to the full one
        parts_sum = acc[(V, False)].astype(np.float64) + acc[(0, True)]
        el, ea = lc.e_acc(parts_sum, acc[lc.FULL].astype(np.float64), r.D)
        assert el <= 2.0 * tols[0] and ea <= 2.0 * tols[1]
        # the same sums, to the last bit: a part left out by its bit (or by NULL) is the part left out by zeroing its input
        dof, qdd, w = lc.inputs(robot, pose)
        still = np.array(dof)
        still[:, 1::2] = 0.0
        for with_qdd in (True, False):
            assert np.array_equal(bits(host_acc(hostemu, r.model, r.root, still, qdd, V, with_qdd)), bits(acc[(0, with_qdd)]))            # qd = 0
        for terms in (V, 0):
            assert np.array_equal(bits(host_acc(hostemu, r.model, r.root, dof, np.zeros_like(qdd), terms, True)), bits(acc[(terms, False)]))  # qdd = 0
        # a body range is a slice of the whole range; the wrenches of a range are the wrenches of the whole range with the others zero
        B = int(r.model.n_rb)
        for first, count in ((0, 1), (B - 1, 1), (B // 3, B // 2), (0, B)):
            assert np.array_equal(bits(host_acc(hostemu, r.model, r.root, dof, qdd, V, True, first, count)), bits(acc[lc.FULL][:, first:first + count]))
            only = np.zeros_like(w)
            only[:, first:first + count] = w[:, first:first + count]
            assert np.array_equal(bits(host_tau(hostemu, r.model, r.root, dof, w[:, first:first + count], first)), bits(host_tau(hostemu, r.model, r.root, dof, only)))


def forest_case(K=16):
    """the forest of two point robots -> (references namespace, dof, qdd, wrenches) at inputs of its own"""
    actors, init = jc.two_point_robot_actors()
    scene = build_scene(list(actors), init)
    n = scene.n_dof
    rng = np.random.default_rng(lc.SEED)
    dof = np.zeros((K, 2 * n), np.float32)
    dof[:, 0::2], dof[:, 1::2] = rng.uniform(-2.0, 2.0, size=(K, n)), rng.uniform(-ic.QD_AMP, ic.QD_AMP, size=(K, n))
    qdd = rng.uniform(-ic.QDD_AMP, ic.QDD_AMP, size=(K, n)).astype(np.float32)
    w = lc.wrenches(K, int(scene.to_c().n_rb))
    return lc.references_of(scene, dof, qdd, w), dof, qdd, w


def test_two_point_robots_are_one_forest(hostemu):
    r, dof, qdd, w = forest_case()
    n = r.scene.n_dof
    assert n == 6
    tols = lc.tolerances("point_robot")
    assert all(x <= 0.1 * t for x, t in zip(r.w32, tols))         # the point robot's tolerances fit the forest's inputs
    acc = {call: host_acc(hostemu, r.model, r.root, dof, qdd, *call) for call in lc.ACC_CALLS}
    tau = host_tau(hostemu, r.model, r.root, dof, w)
    e, et = measure(acc, tau, r)
    report("two point robots, host build", e, et, tols)
    assert max(a for a, _ in e.values()) <= tols[0] and max(b for _, b in e.values()) <= tols[1] and et <= tols[2]
    # the rigid bodies of the first robot are those whose Jacobian has no entry in the second robot's columns
    of_first = ~np.abs(r.J[:, :, :, 3:]).max((0, 2, 3)).astype(bool) & ~r.zero
    of_second = ~np.abs(r.J[:, :, :, :3]).max((0, 2, 3)).astype(bool) & ~r.zero
    assert of_first.any() and of_second.any() and not (of_first & of_second).any()
    other = np.array(qdd)
    other[:, 3:] = -other[:, 3:]
    again = host_acc(hostemu, r.model, r.root, dof, other, *lc.FULL)
    assert np.array_equal(bits(again[:, of_first]), bits(acc[lc.FULL][:, of_first]))               # a robot's links do not move with the other robot's qdd
    assert np.abs(again[:, of_second] - acc[lc.FULL][:, of_second]).max((1, 2)).min() > 100.0 * tols[0] * r.D[0]
    only = np.zeros_like(w)
    only[:, of_first] = w[:, of_first]
    t1 = host_tau(hostemu, r.model, r.root, dof, only)
    assert not t1[:, 3:].any() and np.abs(t1[:, :3]).max(1).min() > 0.0                          # a wrench on one robot: zeros in the other's joints


# ---- 4. far against origin ----------------------------------------------------------------------------------------------------------
def test_far_from_the_origin_meets_the_tolerance_of_the_origin_row(host_results):
    o, f = lc.references("omnipanda", "origin"), lc.references("omnipanda", "far")
    tols = lc.tolerances_from(o.w32)                                # from the origin row's restatement alone
    dof = lc.inputs("omnipanda", "far")[0]
    assert (np.abs(dof[:, 0]) == ic.FAR).all() and (np.abs(dof[:, 2]) == ic.FAR).all()
    e, et = measure(*host_results["omnipanda", "far"], f)
    e0, et0 = measure(*host_results["omnipanda", "origin"], o)
    report("omnipanda far, against the tolerance of origin", e, et, tols)
    report("omnipanda origin", e0, et0, tols)
    assert max(a for a, _ in e.values()) <= tols[0] and max(b for _, b in e.values()) <= tols[1] and et <= tols[2]
    # the same figures: the accelerations and joint forces do not depend on where the base joints stand
    for c in lc.ACC_CALLS:
        el, ea = lc.e_acc(host_results["omnipanda", "far"][0][c], host_results["omnipanda", "origin"][0][c].astype(np.float64), o.D)
        assert el <= tols[0] and ea <= tols[1]
    assert lc.e_tau(host_results["omnipanda", "far"][1], host_results["omnipanda", "origin"][1].astype(np.float64), o.Dj) <= tols[2]


# ---- 5. wrenches --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_wrench_forces_do_the_work_of_the_wrenches(robot, host_results, hostemu):
    r = lc.references(robot)
    dof, qdd, w = lc.inputs(robot)
    tau = host_results[robot, "origin"][1]
    tol = lc.tolerances(robot)[2]
    # a NaN or Inf in an ignored row leaves tau unchanged, bit for bit
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = np.array(w)
        poisoned[:, r.zero] = bad
        assert np.array_equal(bits(host_tau(hostemu, r.model, r.root, dof, poisoned)), bits(tau))
    # tau . qd = sum_b w_b . (J_ref,b qd): each joint's share within its tolerance
    qd = dof[:, 1::2].astype(np.float64)
    work = np.einsum("kbr,kbri,ki->k", w.astype(np.float64), r.J, qd)
    gap = np.abs(np.einsum("ki,ki->k", tau.astype(np.float64), qd) - work)
    bound = tol * np.abs(qd) @ r.Dj
    print(f"\n[{robot}] tau . qd against sum w . (J_ref qd): worst gap / bound {(gap / bound).max():.2f}")
    assert (gap <= bound).all()


def test_a_unit_wrench_gives_a_row_of_the_jacobian(hostemu):
    for robot in ("franka_panda", "panda_gripper"):
        r = lc.references(robot)
        dof = lc.inputs(robot)[0][:16]
        tol_J = jc.tolerances(robot)[0]
        worst = 0.0
        for b in range(int(r.model.n_rb)):
            for j in range(6):
                unit = np.zeros((len(dof), 1, 6), np.float32)
                unit[:, 0, j] = 1.0
                worst = max(worst, float(np.abs(host_tau(hostemu, r.model, r.root, dof, unit, b) - r.J[:len(dof), b, j, :]).max()))
        print(f"\n[{robot}] unit wrenches against the rows of J_ref: {worst:.1e} (tol_J {tol_J:.0e})")
        assert worst <= tol_J


# ---- 6. refusals of the host build --------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu, tmp_path):
    from scenes import boxer_push
    out = np.zeros(4096, np.float32)
    r = lc.references("franka_panda")
    dof, qdd, w = lc.inputs("franka_panda")
    K, B = 2, int(r.model.n_rb)
    q, qd, a, ww = (np.ascontiguousarray(x) for x in (dof[:K, 0::2], dof[:K, 1::2], qdd[:K], w[:K]))
    root32 = np.ascontiguousarray(r.root, np.float32)
    acc = lambda model, root, q, qd, first, count, a, terms, o: hostemu.emu_link_acceleration(C.byref(model), K, fp(root), fp(q), fp(qd), first, count, fp(a), terms, fp(o))
    wre = lambda model, root, q, first, count, ww, o: hostemu.emu_wrench_forces(C.byref(model), K, fp(root), fp(q), first, count, fp(ww), fp(o))
    # a moving base
    _, boxer, _, _, bdof, broot = boxer_push(K=8, H=2)
    bq, bqd = np.ascontiguousarray(np.tile(np.asarray(bdof, np.float32)[0::2], (K, 1))), np.ascontiguousarray(np.tile(np.asarray(bdof, np.float32)[1::2], (K, 1)))
    broot32 = np.ascontiguousarray(broot, np.float32)
    bw = np.ones((K, int(boxer.n_rb), 6), np.float32)
    for a_in in (bq, None):
        assert acc(boxer, broot32, bq, bqd, 0, int(boxer.n_rb), a_in, V, out) == -2
    assert wre(boxer, broot32, bq, 0, int(boxer.n_rb), bw, out) == -2
    # a model that does not pack (a position drive needs a stiffness)
    bad = lc.scene_of("franka_panda").to_c()
    bad.drive_mode, bad.drive_kp = capi.DRIVE_POSITION, -1.0
    assert acc(bad, root32, q, qd, 0, B, a, V, out) == -1 and wre(bad, root32, q, 0, B, ww, out) == -1
    # a tree this build does not instantiate: the synthetic five-body URDF of test_gpu_runtime_tree.py
    from test_gpu_runtime_tree import actor_yaml, write_branched_urdf
    urdf, actor = str(tmp_path / "branched5.urdf"), str(tmp_path / "arm5.yaml")
    write_branched_urdf(urdf)
    actor_yaml(actor, urdf)
    tree = build_scene([actor], [[0.0, 0.0, 0.0]])
    tm = tree.to_c()
    _, troot = tree.initial_state()
    tq = np.zeros((K, tree.n_dof), np.float32)
    assert acc(tm, np.ascontiguousarray(troot, np.float32), tq, tq, 0, int(tm.n_rb), tq, V, out) == -3
    assert wre(tm, np.ascontiguousarray(troot, np.float32), tq, 0, int(tm.n_rb), np.ones((K, int(tm.n_rb), 6), np.float32), out) == -3
    # bits other than MPPI_ID_VELOCITY: gravity has no part in a kinematic quantity
    for terms in (lc.ID_GRAVITY, lc.ID_GRAVITY | V, 4, 16, 18, -1, 1 << 30):
        assert acc(r.model, root32, q, qd, 0, B, a, terms, out) == -4, terms
    # null pointers
    assert acc(r.model, root32, q, qd, 0, B, a, V, None) == -5
    assert wre(r.model, root32, q, 0, B, None, out) == -5 and wre(r.model, root32, q, 0, B, ww, None) == -5
    # a range outside [0, n_rb)
    for first, count in ((-1, 1), (0, 0), (0, B + 1), (B, 1), (B - 1, 2), (1, 1 << 31 - 1)):
        assert acc(r.model, root32, q, qd, first, count, a, V, out) == -6, (first, count)
        assert wre(r.model, root32, q, first, count, ww, out) == -6, (first, count)
    assert not out.any()                                            # nothing was written
    assert acc(r.model, root32, q, qd, 0, B, a, V, out) == 0 and out[:K * B * 6].any() and not out[K * B * 6:].any()
    out[:] = 0.0
    assert wre(r.model, root32, q, 0, B, ww, out) == 0 and out[:K * 7].all() and not out[K * 7:].any()
