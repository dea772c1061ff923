"""The no-GPU half of the forward-dynamics tests (inputs, references, metrics and tolerances: forward_dynamics_cases.py; the kernel
on the GPU: test_gpu_forward_dynamics.py).

 * the entry is exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states its contract, the
   wrapper has the accessors;
 1 the device function forward_dynamics (csrc/mppi_device.hpp) itself, compiled for the host, meets BOTH tolerances of the GPU half
   for every robot at every base pose, for all eight combinations of terms with tau given and left out; nothing asked for and no
   tau: exactly 0; the separate calls sum to the full one; where the routine promises the very same sums - a part left out by its
   bit against the same part left out by a zeroed input - the results agree to the last bit;
 2 the `far` row of the mobile manipulator (prismatic base joints 420 m out) meets the tolerance of its `origin` row ALONE;
 3 a pass means something, on the reference alone: the references are finite; leaving out any term, the tau rows of a neighbouring
   env, the joint order of tau reversed, the sign of gravity - each moves some entry by >= 100 tolerances in both metrics (or by what
   is stated below, with the reason); the fp32 oracle the tolerances come from is re-measured and sits within a tenth of them;
 4 the host build refuses what the library refuses - a moving base, unknown bits in terms, a null output - without writing.
The four planted defects of the device routine (shift of the articulated inertia left out, bias moment not moved by d x f, velocity
product dropped for prismatic joints, the parent's 1/d used for the child) were each shown to fail row 1 on a scratch copy of the
host build: profiles/r15a_planted_defects.txt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forward_dynamics_cases as fc
import inverse_dynamics_cases as ic
from mppiisaac.backend import capi

ROBOT_IDS = list(fc.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
G, V = fc.ID_GRAVITY, fc.ID_VELOCITY


def test_the_entry_is_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_forward_dynamics"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    assert "mppi_sim_forward_dynamics" in capi.EXPORTED_SYMBOLS
    getattr(lib, "mppi_sim_forward_dynamics")
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    assert "int mppi_sim_forward_dynamics(" in header
    said = header[header.index("What acceleration a joint force GIVES"):header.index("int mppi_sim_forward_dynamics(")]
    for words in ("free of contact", "must not overlap", "MOVING base", "exact zeros", "NOT in it", "tau_dev is NULL", "Refused before"):
        assert words in said, words
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("forward_dynamics", "acquire_free_acceleration_tensor", "refresh_free_acceleration_tensors", "inverse_mass_matrix"):
        assert callable(getattr(IsaacGymWrapper, name))


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu_fd():
    d = os.path.join(HERE, "hostemu_forward_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libforward_dynamics_hostemu.so"))


def host_call(lib, model, root, dof, tau, terms, with_tau):
    K, n = tau.shape
    root32 = np.ascontiguousarray(root, np.float32)
    q, qd, t = (np.ascontiguousarray(x, np.float32) for x in (dof[:, 0::2], dof[:, 1::2], tau))
    qdd = np.full((K, n), np.nan, np.float32)
    assert lib.emu_forward_dynamics(C.byref(model), K, fp(root32), fp(q), fp(qd), fp(t) if with_tau else None, terms, fp(qdd)) == 0
    assert np.isfinite(qdd).all()
    return qdd


@pytest.fixture(scope="module")
def host_results(hostemu_fd):
    """{(robot, pose): {call: qdd [K][n]}} of the host build over ALL_CALLS: computed once, shared, read-only"""
    out = {}
    for robot in ROBOT_IDS:
        for pose in fc.POSES[robot]:
            model, root = fc.references(robot, pose)[1], fc.references(robot, pose)[3]
            dof, tau = fc.inputs(robot, pose)
            out[robot, pose] = {call: host_call(hostemu_fd, model, root, dof, tau, *call) for call in fc.ALL_CALLS}
            for a in out[robot, pose].values():
                a.setflags(write=False)
    return out


def report(tag, e, tq, tr):
    print(f"\n[{tag}] e_qdd / e_res per (terms, tau given) (tol {tq:.0e} / {tr:.0e}): " + ", ".join(f"{c}: {a:.1e} / {b:.1e}" for c, (a, b) in e.items()))


# ---- 1. both tolerances, all eight calls --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_function_on_the_host_meets_both_tolerances(robot, host_results, hostemu_fd):
    tq, tr = fc.tolerances(robot)
    for pose in fc.POSES[robot]:
        scene, model, model_off, root, ref, D, M_ref, Dtau, _, _, _ = fc.references(robot, pose)
        got = host_results[robot, pose]
        e = fc.measure(got, ref, D, M_ref, Dtau)
        report(f"{robot} {pose} host build", e, tq, tr)
        assert max(a for a, _ in e.values()) <= tq and max(b for _, b in e.values()) <= tr
        assert not got[(0, False)].any()                               # nothing asked for, no tau: exact zeros
        # the separate calls sum to the full one (the solve is linear in tau, the gravity and the velocity products)
        parts_sum = got[(G, False)].astype(np.float64) + got[(V, False)] + got[(0, True)]
        full = got[fc.FULL].astype(np.float64)
        assert fc.e_qdd(parts_sum, full, D) <= 2.0 * tq and fc.e_res(parts_sum, full, M_ref, Dtau) <= 2.0 * tr
        # the same sums, to the last bit: a part left out by its bit is the part left out by zeroing its input
        dof, tau = fc.inputs(robot, pose)
        still = np.array(dof)
        still[:, 1::2] = 0.0
        for terms in (G | V, V):
            for with_tau in (True, False):
                assert np.array_equal(host_call(hostemu_fd, model, root, still, tau, terms, with_tau), got[(terms & G, with_tau)])       # qd = 0
                assert np.array_equal(host_call(hostemu_fd, model_off, root, dof, tau, terms, with_tau), got[(terms & V, with_tau)])     # gravity off
        for call in ((G | V, True), (0, True)):                                                                                     # tau = 0
            assert np.array_equal(host_call(hostemu_fd, model, root, dof, np.zeros_like(tau), *call), got[(call[0], False)])


# ---- 2. far against origin ----------------------------------------------------------------------------------------------------------
def test_far_from_the_origin_meets_the_tolerance_of_the_origin_row(host_results):
    o, f = fc.references("omnipanda", "origin"), fc.references("omnipanda", "far")
    tq, tr = fc.tolerances_from(o[8], o[9])                           # from the origin row's fp32 oracle alone
    dof = fc.inputs("omnipanda", "far")[0]
    assert (np.abs(dof[:, 0]) == ic.FAR).all() and (np.abs(dof[:, 2]) == ic.FAR).all()
    e = fc.measure(host_results["omnipanda", "far"], f[4], f[5], f[6], f[7])
    e0 = fc.measure(host_results["omnipanda", "origin"], o[4], o[5], o[6], o[7])
    report("omnipanda far, against the tolerance of origin", e, tq, tr)
    report("omnipanda origin", e0, tq, tr)
    assert max(a for a, _ in e.values()) <= tq and max(b for _, b in e.values()) <= tr


# ---- 3. a pass means something ------------------------------------------------------------------------------------------------------
# What each change must move SOME entry by, in tolerances of (a) e_qdd and (b) e_res: 100 unless stated here.
#  - heijn (a planar base: x, y, yaw): its velocity term is what a centre of mass 0.4 mm off the yaw axis makes of rates of 1 rad/s
#    - 74 tolerances of the torque scale at the most, whatever the draw, as test_inverse_dynamics.py found (50 is asserted there and
#    here), and 30 tolerances of the acceleration scale, whose tolerance (5e-6) is 2.5 times the torque one: 25 asserted.
FLOOR = {("heijn", "without the velocity term"): (25.0, 50.0)}


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_are_well_posed(robot, oracle64):
    tq, tr = fc.tolerances(robot)
    wq, wr = fc.oracle32_worst(robot)
    assert 0.0 < tq <= fc.CAP_QDD and 0.0 < tr <= fc.CAP_RES
    assert wq <= 0.1 * tq and wr <= 0.1 * tr                         # the rule: ten times the fp32 oracle's own deviation, rounded up
    some = {}
    for pose in fc.POSES[robot]:
        scene, model, model_off, root, ref, D, M_ref, Dtau, pq, pr, pfull = fc.references(robot, pose)
        dof, tau = fc.inputs(robot, pose)
        K, n = tau.shape
        assert K == fc.ROBOTS[robot][3]
        assert all(np.isfinite(r).all() for r in ref.values()) and np.isfinite(M_ref).all() and (D > 0.0).all() and (Dtau > 0.0).all()
        assert 2.0 < D.min() and D.max() <= 3.0 + 1e-3               # qdd_ref is the +-3 of the accelerations tau was made from
        full = ref[fc.FULL]
        q, qd = dof[:, 0::2].astype(np.float64), dof[:, 1::2].astype(np.float64)
        other = {
            "without tau": ref[(G | V, False)], "without the gravity term": ref[(V, True)], "without the velocity term": ref[(G, True)],
            "gravity's sign": full - 2.0 * ref[(G, False)],           # (the solve is linear in g)
            "joint order of tau reversed": fc.oracle_qdd(oracle64, model, model_off, root, q, qd, tau[:, ::-1].astype(np.float64), *fc.FULL),
        }
        for shift in (1, -1):
            other[f"env k{shift:+d}'s tau"] = fc.oracle_qdd(oracle64, model, model_off, root, q, qd, np.roll(tau, shift, axis=0).astype(np.float64), *fc.FULL)
        moved = {}
        for name, o in other.items():
            a = (np.abs(o - full) / D[None, :]).max(1) / tq                                              # [K]: every env's worst entry, in tolerances
            b = (np.abs(np.einsum("kij,kj->ki", M_ref, o - full)) / Dtau[None, :]).max(1) / tr
            moved[name] = (a, b)
        print(f"\n[{robot} {pose}] K {K}: fp32 oracle e_qdd {pq:.1e} (full call {pfull:.1e}), e_res {pr:.1e} over all calls (tol {tq:.0e} / {tr:.0e}); D_j "
              f"{np.array2string(D, precision=2)}; moved by, in tolerances of e_qdd | e_res (some entry / the least-moved env): "
              + ", ".join(f"{k} {a.max():.0f} / {a.min():.0f} | {b.max():.0f} / {b.min():.0f}" for k, (a, b) in moved.items()))
        for k, (a, b) in moved.items():
            some[k] = (max(some.get(k, (0.0, 0.0))[0], float(a.max())), max(some.get(k, (0.0, 0.0))[1], float(b.max())))
    for k, (a, b) in some.items():
        fa, fb = FLOOR.get((robot, k), (100.0, 100.0))
        assert a >= fa and b >= fb, f"{robot}: {k} moves no entry by {fa:.0f} / {fb:.0f} tolerances ({a:.0f} / {b:.0f})"


# ---- 4. refusals of the host build --------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu_fd):
    from scenes import boxer_push
    _, model, _, _, dof, root = boxer_push(K=8, H=2)
    out = np.zeros(64, np.float32)
    q, qd = np.ascontiguousarray(np.asarray(dof, np.float32)[0::2]), np.ascontiguousarray(np.asarray(dof, np.float32)[1::2])
    root32 = np.ascontiguousarray(root, np.float32)
    for tau in (q, None):
        assert hostemu_fd.emu_forward_dynamics(C.byref(model), 1, fp(root32), fp(q), fp(qd), fp(tau), 3, fp(out)) == -2      # a moving base
    assert not out.any()
    model, root = fc.references("franka_panda")[1], fc.references("franka_panda")[3]
    dof, tau = fc.inputs("franka_panda")
    q, qd, t = (np.ascontiguousarray(x) for x in (dof[:2, 0::2], dof[:2, 1::2], tau[:2]))
    root32 = np.ascontiguousarray(root, np.float32)
    for terms in (4, 7, 8, -1, 1 << 30):
        assert hostemu_fd.emu_forward_dynamics(C.byref(model), 2, fp(root32), fp(q), fp(qd), fp(t), terms, fp(out)) == -4, terms  # unknown bits
    assert hostemu_fd.emu_forward_dynamics(C.byref(model), 2, fp(root32), fp(q), fp(qd), fp(t), 3, None) == -5                  # a null output
    assert not out.any()
    assert hostemu_fd.emu_forward_dynamics(C.byref(model), 2, fp(root32), fp(q), fp(qd), fp(t), 3, fp(out)) == 0
    assert out[:14].all() and not out[14:].any()
