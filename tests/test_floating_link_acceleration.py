"""The no-GPU half of the moving-base link-acceleration / wrench-force tests (inputs, references, metrics and tolerances:
floating_link_acceleration_cases.py; the kernels on the GPU: test_gpu_floating_link_acceleration.py).

 * the two entries are exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states their conventions,
   the wrapper has the accessors; ABI stays 9; both pointers are filled exactly once, under the NBASE == 1 guard of the function that
   fills the table (the on-demand plugin units go through it);
 1 the reference is believed first: on the fixed-base mobile manipulator and heijn (origin and tilted) the same flow-difference route
   with the base rows left out reproduces link_acceleration_cases.reference_parts within FIXED_ROUTE_AGREE; on the moving-base robots
   the Richardson levels agree, J_ref v meets the oracle's velocity columns, every scale is O(1);
 2 a pass means something: neighbouring envs and each part of the call move an entry by at least 100 tolerances;
 3 the device routines (csrc/mppi_device.hpp), compiled for the host, meet the tolerances for boxer, jackal_a, albert and anymal at
   every env, body and entry in the four acceleration calls and the wrench call;
 4 the zero-input rules bit for bit: NULL == a zero vd row; v = 0 in the state == no velocity bit; terms = 0 without vd == exact zeros;
 5 terms = 0 on vd = e_c is column c of the host build's own floating_link_jacobian, unit wrenches give its rows - within one tolerance
   (the recursion sums the lever arm in another order than the Jacobian's walk), exactly zero where the Jacobian is zero;
 6 duality: tau . v = sum_b w_b . (J_b v) against the oracle's velocity rows;
 7 a base translated by FAR_SHIFT, with another linear velocity, leaves every bit as it was;
 8 in the PUSH_SCENE the block and the obstacle get exact zero rows, and NaN / Inf in their wrench rows reaches nothing;
 9 links welded to the base move with it (a_b + wd_b x r + w_b x (w_b x r) in fp64 from the inputs), a wrench on one shows in rows 0:6
   only: (f, n + r x f), the joint rows exact zeros;
 10 the host build refuses what the library refuses, without writing;
 11 the wrapper raises PerStepOnly inside a horizon view, NotImplementedError with the library's text for a fixed base, ValueError
   naming the expected shapes (a stub).
Four planted defects of the device routines (the bodies next to the base started from zero motion; the base links left at zero as in
the fixed front; the children's d x F left out on the way to the base origin; rows 0:3 and 3:6 exchanged) were each shown to fail row
3 on a scratch copy of the host build: profiles/r21a_planted_defects.txt.

MEASURED (host build, worst e_lin / e_ang over the four calls, e_tau | the fp32 restatement | tolerances): boxer 1.0e-7 / 1.3e-7,
1.8e-7 | 7.0e-7 / 5.1e-7, 4.5e-7 | 1e-5 / 1e-5, 5e-6; jackal_a 8.6e-8 / 1.1e-7, 1.6e-7 | 3.6e-7 / 3.6e-7, 2.6e-7 | 5e-6 / 5e-6, 5e-6;
albert 1.5e-7 / 1.9e-7, 3.1e-7 | 3.7e-7 / 2.9e-7, 5.8e-7 | 5e-6 / 5e-6, 1e-5; anymal 1.9e-7 / 1.5e-7, 3.3e-7 | 3.7e-7 / 4.9e-7, 4.1e-7 |
5e-6 / 5e-6, 5e-6.  No cap binds."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
import floating_link_acceleration_cases as fl
import jacobian_cases as jc
import link_acceleration_cases as lc
from mppiisaac.backend import capi
from scenes import build_scene

ROBOT_IDS = list(fl.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
_vp, _i = C.c_void_p, C.c_int
call_name = lambda c: f"{c[0]}{'+vd' if c[1] else ''}"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entries_are_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_floating_link_acceleration"] == (_i, [_vp, _i, _i, _vp, _i, _vp])
    assert capi._SIGNATURES["mppi_sim_floating_wrench_forces"] == (_i, [_vp, _i, _i, _vp, _vp])
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    for name in ("mppi_sim_floating_link_acceleration", "mppi_sim_floating_wrench_forces"):
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    assert ("int mppi_sim_floating_link_acceleration(mppi_ctx_t *ctx, int rb_first, int rb_count, const float *vd_dev /* [K][6 + n_dof] or NULL */, "
            "int terms,") in header
    assert "int mppi_sim_floating_wrench_forces(mppi_ctx_t *ctx, int rb_first, int rb_count, const float *wrench_dev /* [K][rb_count][6] */," in header
    said = header[header.index("How a link of a robot with a MOVING base ACCELERATES"):header.index("int mppi_sim_floating_link_acceleration(")]
    for words in ("(root linvel, root\n * angvel, qd)", "mppi_sim_floating_jacobian", "EACH ENV'S OWN base rows", "7:13", "time derivative",
                  "rows 0-2 the classical acceleration", "gravity has no part", "exact zeros", "column c of J_b", "welded to the moving base",
                  "a_b + wd_b x r + w_b x (w_b x r)", "exact zero rows", "difference\n * of world positions", "does not depend on where the base stands",
                  "total force on the base", "total moment about the base origin", "then the joints in DOF order", "to no joint row", "by select",
                  "mppi_sim_floating_forward_dynamics", "captured graph", "MPPI_EINVAL", "unknown bits",
                  "use mppi_sim_link_acceleration / mppi_sim_wrench_forces", "n_extra_bases > 0", "Refused before"):
        assert words in said, words
    # the three sentences that said a moving base has no such entry point to the new entries
    assert "have no entry yet" not in header and "of a moving base stay refused" not in header
    still = header[header.index("STILL refused for a moving base"):header.index("int mppi_sim_floating_jacobian(")]
    assert "mppi_sim_floating_link_acceleration and mppi_sim_floating_wrench_forces" in still
    for start, end in (("What forces a motion TAKES of a robot with a MOVING base", "int mppi_sim_floating_inverse_dynamics("),
                       ("What acceleration a base wrench and joint forces GIVE", "int mppi_sim_floating_forward_dynamics(")):
        para = header[header.index(start):header.index(end)]
        assert "stay refused for a moving base: use mppi_sim_floating_link_acceleration / mppi_sim_floating_wrench_forces" in para
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("floating_link_accelerations", "get_actor_link_floating_acceleration_by_name", "acquire_floating_link_bias_acceleration_tensor",
                 "refresh_floating_link_bias_acceleration_tensors", "floating_forces_from_wrenches", "floating_forces_from_link_wrench"):
        assert callable(getattr(IsaacGymWrapper, name))


def test_both_pointers_are_filled_once_under_the_guard_and_plugins_carry_them():
    csrc = os.path.join(HERE, "..", "mppi-isaac_amd", "csrc")
    kernels = open(os.path.join(csrc, "mppi_kernels.hpp")).read()
    fill = kernels[kernels.index("void fill_topo_entry_scene(TopoEntry &e) {"):]
    fill = fill[:fill.index("\n}\n")]
    guarded = fill[fill.index("if constexpr (T::NBASE == 1)"):]
    entry = kernels[kernels.index("struct TopoEntry {"):]
    entry = entry[:entry.index("};")]
    host = open(os.path.join(csrc, "mppi_hip.hip")).read()
    for name, fixed in (("link_acceleration", "mppi_sim_link_acceleration"), ("wrench_forces", "mppi_sim_wrench_forces")):
        assert f"e.sim_floating_{name} = &launch_sim_floating_{name}_t<T>;" in guarded
        assert kernels.count(f"e.sim_floating_{name} =") == 1
        assert entry.index("static_lds") < entry.index(f"(*sim_floating_{name})")        # at the end of the row
        assert f"if (!e->sim_floating_{name}) return fail(MPPI_EUNSUPPORTED" in host
        assert f'floating_entry(c, "mppi_sim_floating_{name}", "{fixed}", e)' in host
        assert f'rb_range_check(c, "mppi_sim_floating_{name}", rb_first, rb_count)' in host
        assert f"__launch_bounds__(kWave) void k_sim_floating_{name}(" in kernels
    assert "out[2] = sizeof(mppi::TopoEntry)" in host               # a stale plugin is rebuilt
    assert 'mppi_plugin_fill_scene(mppi::TopoEntry *e) { fill_topo_entry_scene<mppi::Topo<' in host
    # one routine, two fronts
    device = open(os.path.join(csrc, "mppi_device.hpp")).read()
    for front in ("link_accelerations_pass<false, T>(", "link_accelerations_pass<true, T>(", "link_acceleration_of<false, T>(", "link_acceleration_of<true, T>(",
                  "gather_link_wrench_on<false, T>(", "gather_link_wrench_on<true, T>(", "wrench_joint_forces_pass<false, T>(", "wrench_joint_forces_pass<true, T>("):
        assert device.count(front) == 1, front


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,pose", [("omnipanda", "origin"), ("omnipanda", "tilted"), ("heijn", "origin"), ("heijn", "tilted")])
def test_the_route_reproduces_the_fixed_base_references(robot, pose, oracle64):
    r = lc.references(robot, pose)
    dof, qdd, _ = lc.inputs(robot, pose)
    K = 8
    q, qd = dof[:K, 0::2].astype(np.float64), dof[:K, 1::2].astype(np.float64)
    J, parts = fl.route_parts(oracle64, r.model, r.root, q, qd, qdd[:K].astype(np.float64), moving=False)
    gaps = {"J": float(np.abs(J - r.J[:K]).max()), "A": float(np.abs(parts["A"] - r.parts["A"][:K]).max()), "V": float(np.abs(parts["V"] - r.parts["V"][:K]).max())}
    print(f"\n[{robot} {pose}] the flow-difference route without base rows against link_acceleration_cases.reference_parts: "
          + ", ".join(f"{k} {v:.1e}" for k, v in gaps.items()) + f"; Richardson gap {parts['gap']:.1e}")
    assert max(gaps.values()) <= fl.FIXED_ROUTE_AGREE and parts["gap"] <= fl.RICHARDSON_AGREE
    assert np.abs(parts["V"]).max() > 0.1 and np.abs(parts["A"]).max() > 1.0


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_reference_is_well_posed(robot, oracle64):
    r = fl.references(robot)
    dof, roots, vd, w = fl.inputs(robot)
    K, n = len(dof), dof.shape[1] // 2
    B = int(r.model.n_rb)
    assert K == fl.ROBOTS[robot][2] and r.J.shape == (K, B, 6, 6 + n) and r.tau_ref.shape == (K, 6 + n) and w.shape == (K, B, 6)
    assert all(fl.combine(r.parts, *c).shape == (K, B, 6) for c in fl.ACC_CALLS) and not fl.combine(r.parts, 0, False).any()
    # J_ref v is what the oracle reports as the bodies' velocity columns at the env's own twist and rates
    a = int(r.model.robot_actor)
    vel = np.stack([oracle64.rigid_body_state(r.model, roots[k].astype(np.float64), dof[k, 0::2].astype(np.float64), dof[k, 1::2].astype(np.float64))[0][:, 7:13]
                    for k in range(6)])
    Jv = float(np.abs(np.einsum("kbri,ki->kbr", r.J[:6], r.v[:6]) - vel).max())
    print(f"\n[{robot}] Richardson levels agree to {r.parts['gap']:.1e}; D_lin {r.D[0]:.2f}, D_ang {r.D[1]:.2f}; D_j of tau_ref from {r.Dj.min():.2f} to "
          f"{r.Dj.max():.1f}; J_ref v against the oracle's velocity columns {Jv:.1e}")
    assert r.parts["gap"] <= fl.RICHARDSON_AGREE and Jv <= 1e-14
    assert 1.0 <= r.D[0] <= 20.0 and 1.0 <= r.D[1] <= 20.0 and r.Dj.min() >= 0.5       # every scale O(1): no floor binds
    assert np.array_equal(r.Dj, np.abs(r.tau_ref).max(0))
    assert not r.zero.any() and r.L == B                                                # a robot-only scene: every body is a link


# ---- 2. a pass means something ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_tell_the_envs_and_the_parts_apart(robot):
    r = fl.references(robot)
    tol = fl.tolerances(robot)
    assert all(0.0 < t <= fl.CAP for t in tol) and tol == fl.tolerances_from(r.w32)
    full = fl.combine(r.parts, *fl.FULL)
    step = np.abs(np.diff(full, axis=0))
    apart = min((step[:, :, 0:3].max((1, 2)) / r.D[0]).min() / tol[0], (step[:, :, 3:6].max((1, 2)) / r.D[1]).min() / tol[1])
    apart_tau = (np.abs(np.diff(r.tau_ref, axis=0)) / r.Dj).max(1).min() / tol[2]
    moved = {p: min(e / t for e, t in zip(fl.e_acc(r.parts[p], 0.0, r.D), tol)) for p in ("A", "V")}
    print(f"\n[{robot}] tol {tol[0]:.0e} / {tol[1]:.0e} / {tol[2]:.0e} (fp32 restatement {r.w32[0]:.1e} / {r.w32[1]:.1e} / {r.w32[2]:.1e}); neighbouring envs differ by "
          f"at least {apart:.0f} tol (acc), {apart_tau:.0f} tol (tau); the parts move an entry by J vd {moved['A']:.0f}, Jdot v {moved['V']:.0f} tol")
    assert apart >= 100.0 and apart_tau >= 100.0 and min(moved.values()) >= 100.0


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_link_acceleration")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_link_acceleration_hostemu.so"))


def _state(roots, dof):
    return np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(dof[:, 0::2], np.float32), np.ascontiguousarray(dof[:, 1::2], np.float32)


def host_acc(lib, model, roots, dof, vd, terms, with_vd, rb_first=0, rb_count=None):
    K = len(dof)
    rb_count = int(model.n_rb) - rb_first if rb_count is None else rb_count
    roots32, q, qd = _state(roots, dof)
    vd32 = np.ascontiguousarray(vd, np.float32) if with_vd else None
    acc = np.full((K, rb_count, 6), np.nan, np.float32)
    assert lib.emu_floating_link_acceleration(C.byref(model), K, fp(roots32), fp(q), fp(qd), rb_first, rb_count, fp(vd32), terms, fp(acc)) == 0
    assert np.isfinite(acc).all()
    return acc


def host_tau(lib, model, roots, dof, w, rb_first=0, rb_count=None):
    K, n = len(dof), dof.shape[1] // 2
    rb_count = int(model.n_rb) - rb_first if rb_count is None else rb_count
    roots32, q, _ = _state(roots, dof)
    w32 = np.ascontiguousarray(w, np.float32)
    assert w32.shape == (K, rb_count, 6)
    tau = np.full((K, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_wrench_forces(C.byref(model), K, fp(roots32), fp(q), rb_first, rb_count, fp(w32), fp(tau)) == 0
    return tau


def host_J(lib, model, roots, dof):
    K, n = len(dof), dof.shape[1] // 2
    roots32, q, _ = _state(roots, dof)
    J = np.full((K, int(model.n_rb), 6, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_link_jacobian(C.byref(model), K, fp(roots32), fp(q), 0, int(model.n_rb), fp(J)) == 0
    return J


# ---- 3. the tolerances --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_functions_on_the_host_meet_the_tolerances(robot, hostemu):
    r = fl.references(robot)
    dof, roots, vd, w = fl.inputs(robot)
    tol = fl.tolerances(robot)
    acc = {c: host_acc(hostemu, r.model, roots, dof, vd, *c) for c in fl.ACC_CALLS}
    tau = host_tau(hostemu, r.model, roots, dof, w)
    worst, et = fl.measure(acc, tau, r)
    print(f"\n[{robot}] host build, e_lin / e_ang per call (terms, vd given): " + ", ".join(f"{call_name(c)} {e[0]:.1e} / {e[1]:.1e}" for c, e in worst.items())
          + f"; e_tau {et:.1e}; tol {tol[0]:.0e} / {tol[1]:.0e} / {tol[2]:.0e}, fp32 restatement {r.w32[0]:.1e} / {r.w32[1]:.1e} / {r.w32[2]:.1e}")
    assert max(e[0] for e in worst.values()) <= tol[0] and max(e[1] for e in worst.values()) <= tol[1] and et <= tol[2]
    assert np.isfinite(tau).all()
    # a sub-range of bodies is the slice of the full call, bit for bit
    B = int(r.model.n_rb)
    assert np.array_equal(bits(host_acc(hostemu, r.model, roots, dof, vd, *fl.FULL, 1, B - 2)), bits(acc[fl.FULL][:, 1:B - 1]))
    assert np.array_equal(bits(host_acc(hostemu, r.model, roots, dof, vd, *fl.FULL, B - 1, 1)), bits(acc[fl.FULL][:, B - 1:]))


# ---- 4. the zero-input rules --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_zeroed_inputs_are_the_calls_without_them(robot, hostemu):
    r = fl.references(robot)
    dof, roots, vd, _ = (a[:16] for a in fl.inputs(robot))
    a = int(r.model.robot_actor)
    zero_vd = np.zeros_like(vd)
    for terms in (fl.ID_VELOCITY, 0):
        assert np.array_equal(bits(host_acc(hostemu, r.model, roots, dof, zero_vd, terms, True)), bits(host_acc(hostemu, r.model, roots, dof, vd, terms, False)))
    still_dof, still_roots = np.array(dof), np.array(roots)
    still_dof[:, 1::2] = 0.0
    still_roots[:, a, 7:13] = 0.0
    for with_vd in (True, False):
        assert np.array_equal(bits(host_acc(hostemu, r.model, still_roots, still_dof, vd, fl.ID_VELOCITY, with_vd)),
                              bits(host_acc(hostemu, r.model, roots, dof, vd, 0, with_vd)))
    assert not host_acc(hostemu, r.model, roots, dof, vd, 0, False).any()           # nothing asked for: every product has a zero factor
    assert not np.array_equal(host_acc(hostemu, r.model, roots, dof, vd, *fl.FULL), host_acc(hostemu, r.model, roots, dof, vd, 0, True))


# ---- 5. against the host build's own Jacobian ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_unit_rows_give_the_columns_and_unit_wrenches_the_rows_of_the_jacobian(robot, hostemu):
    r = fl.references(robot)
    dof, roots, _, _ = (a[:8] for a in fl.inputs(robot))
    K, N, B = len(dof), 6 + dof.shape[1] // 2, int(r.model.n_rb)
    tol = fl.tolerances(robot)
    J = host_J(hostemu, r.model, roots, dof).astype(np.float64)
    cols = np.stack([host_acc(hostemu, r.model, roots, dof, np.tile(np.eye(N, dtype=np.float32)[c], (K, 1)), 0, True) for c in range(N)], axis=3)
    rows = np.zeros((K, B, 6, N))
    for b in range(B):
        for j in range(6):
            w = np.zeros((K, B, 6), np.float32)
            w[:, b, j] = 1.0
            rows[:, b, j] = host_tau(hostemu, r.model, roots, dof, w)
    scale = np.array([max(1.0, np.abs(J[:, :, 0:3]).max())] * 3 + [1.0] * 3)[None, None, :, None]
    e_cols, e_rows = float((np.abs(cols - J) / scale).max()), float((np.abs(rows - J) / scale).max())
    print(f"\n[{robot}] terms = 0 on vd = e_c against the host build's floating_link_jacobian: {e_cols:.1e}; unit wrenches against its rows: {e_rows:.1e} "
          f"(of max(1, largest lever arm) = {scale[0, 0, 0, 0]:.2f}); tol {min(tol):.0e}")
    assert e_cols <= min(tol) and e_rows <= min(tol)
    assert not cols[J == 0.0].any() and not rows[J == 0.0].any()                    # what the Jacobian has exactly zero stays exactly zero
    assert np.array_equal(cols[:, :, :, 0:3][J[:, :, :, 0:3] == 1.0], np.ones(int((J[:, :, :, 0:3] == 1.0).sum())))


# ---- 6. duality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_the_forces_do_the_work_of_the_wrenches(robot, hostemu, oracle64):
    r = fl.references(robot)
    dof, roots, _, w = (a[:16] for a in fl.inputs(robot))
    tol_tau = fl.tolerances(robot)[2]
    tau = host_tau(hostemu, r.model, roots, dof, w).astype(np.float64)
    v = r.v[:16]
    vel = np.stack([oracle64.rigid_body_state(r.model, roots[k].astype(np.float64), dof[k, 0::2].astype(np.float64), dof[k, 1::2].astype(np.float64))[0][:, 7:13]
                    for k in range(16)])
    power, work = np.einsum("kj,kj->k", tau, v), np.einsum("kbr,kbr->k", w.astype(np.float64), vel)
    bound = tol_tau * (r.Dj[None, :] * np.abs(v)).sum(1)            # every row of tau within tol_tau D_j
    print(f"\n[{robot}] tau . v against sum_b w_b . (J_b v): {np.abs(power - work).max():.1e} W at worst (bound {bound.min():.1e} .. {bound.max():.1e}, powers up to {np.abs(work).max():.0f} W)")
    assert (np.abs(power - work) <= bound).all() and np.abs(work).min() > 100.0 * bound.max()


# ---- 7. what the results must not notice --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_results_do_not_depend_on_where_the_base_stands_or_how_fast_it_travels(robot, hostemu):
    r = fl.references(robot)
    dof, roots, vd, w = (a[:16] for a in fl.inputs(robot))
    a = int(r.model.robot_actor)
    far = np.array(roots)
    far[:, a, 0:3] += np.asarray(fl.FAR_SHIFT, np.float32)
    far[:, a, 7:10] += np.float32(5.0)
    assert np.array_equal(bits(host_acc(hostemu, r.model, far, dof, vd, *fl.FULL)), bits(host_acc(hostemu, r.model, roots, dof, vd, *fl.FULL)))
    assert np.array_equal(bits(host_tau(hostemu, r.model, far, dof, w)), bits(host_tau(hostemu, r.model, roots, dof, w)))


# ---- 8. the bodies of other actors --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def push():
    scene = build_scene(fl.PUSH_SCENE, [[0.0, 2.5, 0.05]])
    model = scene.to_c()
    dof0, roots0 = fc.draw_inputs(scene, 16)
    dof, roots, vd = fi.draw_rates(dof0, roots0, scene.robot_idx)
    w = lc.wrenches(16, int(model.n_rb))
    return SimpleNamespace(scene=scene, model=model, dof=dof, roots=roots, vd=vd, w=w, r=fl.references_at(scene, model, roots, dof, vd, w))


def test_bodies_of_box_actors_get_exact_zero_rows_and_their_wrenches_reach_nothing(hostemu, push):
    r, tol = push.r, fl.tolerances("boxer")
    other = r.zero
    assert other.sum() == 2 and not other[r.first:r.first + r.L].any()
    assert all(x <= 0.2 * t for x, t in zip(r.w32, tol))            # boxer's tolerances fit the scene's inputs
    acc = {c: host_acc(hostemu, push.model, push.roots, push.dof, push.vd, *c) for c in fl.ACC_CALLS}
    tau = host_tau(hostemu, push.model, push.roots, push.dof, push.w)
    worst, et = fl.measure(acc, tau, r)
    assert max(e[0] for e in worst.values()) <= tol[0] and max(e[1] for e in worst.values()) <= tol[1] and et <= tol[2]
    for c in fl.ACC_CALLS:
        assert not fl.combine(r.parts, *c)[:, other].any() and not bits(acc[c][:, other]).any()     # +0.0 everywhere
    for b in np.flatnonzero(other):
        assert not bits(host_acc(hostemu, push.model, push.roots, push.dof, push.vd, *fl.FULL, int(b), 1)).any()
    for poison in (np.nan, np.inf, -np.inf):
        w = np.array(push.w)
        w[:, other] = poison
        assert np.array_equal(bits(host_tau(hostemu, push.model, push.roots, push.dof, w)), bits(tau))
    for b in np.flatnonzero(other):                                 # a range of such bodies alone: exact zeros
        lone = np.full((16, 1, 6), np.nan, np.float32)
        assert not host_tau(hostemu, push.model, push.roots, push.dof, lone, int(b), 1).any()


# ---- 9. links welded to the base ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,count", [("boxer", 6), ("jackal_a", 10), ("albert", 13), ("anymal", 5)])
def test_links_welded_to_the_base_move_with_it_and_load_the_base_rows_only(robot, count, hostemu, oracle64):
    r = fl.references(robot)
    dof, roots, vd, w = (a[:16] for a in fl.inputs(robot))
    K, n = len(dof), dof.shape[1] // 2
    a = int(r.model.robot_actor)
    tol = fl.tolerances(robot)
    welded = [r.first + l for l, L in enumerate(r.scene.robot_model["links"]) if L["body"] < 0]
    assert len(welded) == count == int((~np.abs(r.J[:, :, :, 6:]).max((0, 2, 3)).astype(bool)).sum())
    acc = host_acc(hostemu, r.model, roots, dof, vd, *fl.FULL)
    rows = np.stack([oracle64.rigid_body_state(r.model, roots[k].astype(np.float64), dof[k, 0::2].astype(np.float64), dof[k, 1::2].astype(np.float64))[0] for k in range(K)])
    arm = rows[:, welded, 0:3] - roots[:, None, a, 0:3].astype(np.float64)             # r = p_link - p_base
    wb, ab, wdb = (np.broadcast_to(x.astype(np.float64)[:, None, :], arm.shape) for x in (roots[:, a, 10:13], vd[:, 0:3], vd[:, 3:6]))
    rigid = np.concatenate([ab + np.cross(wdb, arm) + np.cross(wb, np.cross(wb, arm)), wdb], axis=2)
    e = fl.e_acc(acc[:, welded], rigid, r.D)
    print(f"\n[{robot}] {count} links welded to the base against a_b + wd_b x r + w_b x (w_b x r), wd_b in fp64: e_lin {e[0]:.1e}, e_ang {e[1]:.1e}")
    assert e[0] <= tol[0] and e[1] <= tol[1] and np.abs(rigid[:, :, 0:3]).max() > 1.0
    assert np.array_equal(bits(acc[:, welded, 3:6]), bits(np.broadcast_to(vd[:, None, 3:6], (K, count, 3))))   # the base's own angular acceleration, as numbers
    # a wrench on a welded link: (f, n + r x f) in rows 0:6, no joint row
    only = np.zeros_like(w)
    only[:, welded] = w[:, welded]
    tau = host_tau(hostemu, r.model, roots, dof, only)
    f, m = only[:, welded, 0:3].astype(np.float64), only[:, welded, 3:6].astype(np.float64)
    want = np.concatenate([f.sum(1), (m + np.cross(arm, f)).sum(1)], axis=1)
    assert not tau[:, 6:].any()                                     # exact zeros in every joint row
    assert np.abs(tau[:, 0:6] - want).max() <= tol[2] * np.abs(want).max() and np.abs(want).min(0).max() > 0.1
    for b in welded[:2]:                                            # one welded link alone, a one-body range
        t1 = host_tau(hostemu, r.model, roots, dof, w[:, b:b + 1], b, 1)
        assert not t1[:, 6:].any() and np.array_equal(bits(t1[:, 0:3]), bits(w[:, b, 0:3]))


# ---- 10. refusals of the host build -------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu):
    out = np.zeros(4096, np.float32)
    r = fl.references("boxer")
    dof, roots, vd, w = fl.inputs("boxer")
    K, B = 2, int(r.model.n_rb)

    def acc(model, roots, q, qd, first, count, vd, terms, o):
        return hostemu.emu_floating_link_acceleration(C.byref(model), K, fp(roots), fp(q), fp(qd), first, count, fp(vd), terms, fp(o))

    def tau(model, roots, q, first, count, w, o):
        return hostemu.emu_floating_wrench_forces(C.byref(model), K, fp(roots), fp(q), first, count, fp(w), fp(o))
    q, qd, roots32, vd32, w32 = (np.ascontiguousarray(x) for x in (dof[:K, 0::2], dof[:K, 1::2], roots[:K], vd[:K], w[:K]))
    # a fixed base; a fixed-base forest
    p = jc.references("franka_panda")
    pq = np.ascontiguousarray(jc.inputs("franka_panda")[0][:K, 0::2])
    proots = np.ascontiguousarray(np.tile(np.asarray(p[2], np.float32), (K, 1, 1)))
    assert acc(p[1], proots, pq, pq, 0, 1, None, 2, out) == -2 and tau(p[1], proots, pq, 0, 1, out, out) == -2
    actors, init = jc.two_point_robot_actors()
    forest = build_scene(list(actors), init)
    froots = np.ascontiguousarray(np.tile(np.asarray(forest.initial_state()[1], np.float32), (K, 1, 1)))
    fq = np.zeros((K, forest.n_dof), np.float32)
    assert acc(forest.to_c(), froots, fq, fq, 0, 1, None, 2, out) == -2 and tau(forest.to_c(), froots, fq, 0, 1, w32, out[1000:]) == -2
    # a forest of two moving bases
    two = build_scene(["jackal_a", "jackal_b"], [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    tm = two.to_c()
    assert int(tm.n_extra_bases) == 1
    troots = np.ascontiguousarray(np.tile(np.asarray(two.initial_state()[1], np.float32), (K, 1, 1)))
    tq = np.zeros((K, two.n_dof), np.float32)
    assert acc(tm, troots, tq, tq, 0, 1, None, 2, out) == -7 and tau(tm, troots, tq, 0, 1, w32, out[1000:]) == -7
    # null pointers, ranges outside [0, n_rb), bits other than MPPI_ID_VELOCITY
    assert acc(r.model, roots32, q, qd, 0, B, vd32, 2, None) == -5
    assert tau(r.model, roots32, q, 0, B, None, out) == -5 and tau(r.model, roots32, q, 0, B, w32, None) == -5
    for first, count in ((-1, 1), (0, 0), (B, 1), (0, B + 1), (B - 1, 2), (1, 2 ** 31 - 1)):
        assert acc(r.model, roots32, q, qd, first, count, vd32, 2, out) == -6, (first, count)
        assert tau(r.model, roots32, q, first, count, w32, out) == -6, (first, count)
    for terms in (1, 3, 4, -1, 1 << 16):
        assert acc(r.model, roots32, q, qd, 0, B, vd32, terms, out) == -4, terms
    assert not out.any()                                            # nothing was written
    assert acc(r.model, roots32, q, qd, 0, B, vd32, 2, out) == 0 and out[:K * B * 6].all() and not out[K * B * 6:].any()


# ---- 11. the wrapper's refusals, through a stub -------------------------------------------------------------------------------------
def test_wrapper_refuses_a_horizon_view_a_fixed_base_and_wrong_shapes():
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
    texts = {"acc": b"mppi_sim_floating_link_acceleration: this robot has a fixed base (there are no base columns); use mppi_sim_link_acceleration",
             "tau": b"mppi_sim_floating_wrench_forces: this robot has a fixed base (there are no base columns); use mppi_sim_wrench_forces"}
    calls, last = [], []

    def acc_entry(ctx, first, count, vd, terms, out):
        calls.append(("acc", first, count, vd, terms))
        last[:] = ["acc"]
        return capi.MPPI_EUNSUPPORTED

    def tau_entry(ctx, first, count, w, out):
        calls.append(("tau", first, count, w))
        last[:] = ["tau"]
        return capi.MPPI_EUNSUPPORTED
    own = {}
    sim = object.__new__(IsaacGymWrapper)
    sim._state_t = sim._state_t_own = own
    sim.num_envs, sim.device, sim._ctx, sim._floating_link_bias_acceleration = 4, "cpu", None, {}
    sim.scene = SimpleNamespace(n_dof=7, actor_index=lambda name: 0, rigid_body_index=lambda actor, link: 5)
    sim._c_model = SimpleNamespace(actors=[SimpleNamespace(first_rb=0, n_rb=11)])
    sim._lib = SimpleNamespace(mppi_sim_floating_link_acceleration=acc_entry, mppi_sim_floating_wrench_forces=tau_entry,
                               mppi_last_error=lambda: texts[last[0]])
    sim._reset_envs_if_needed = lambda: None
    t = sim.acquire_floating_link_bias_acceleration_tensor("panda")
    assert tuple(t.shape) == (4, 11, 6) and not t.any() and sim.acquire_floating_link_bias_acceleration_tensor("panda") is t
    for call in (sim.refresh_floating_link_bias_acceleration_tensors, lambda: sim.floating_link_accelerations("panda"),
                 lambda: sim.floating_link_accelerations("panda", vd=np.zeros(13, np.float32), velocity=False),
                 lambda: sim.get_actor_link_floating_acceleration_by_name("panda", "panda_hand", vd=np.zeros((4, 13), np.float32))):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_link_acceleration"):
            call()
    for call in (lambda: sim.floating_forces_from_wrenches("panda", np.zeros((11, 6), np.float32)),
                 lambda: sim.floating_forces_from_wrenches("panda", np.zeros((4, 11, 6), np.float32)),
                 lambda: sim.floating_forces_from_link_wrench("panda", "panda_hand", np.zeros(6, np.float32)),
                 lambda: sim.floating_forces_from_link_wrench("panda", "panda_hand", np.zeros((4, 6), np.float32))):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_wrench_forces"):
            call()
    assert [c[:3] for c in calls] == [("acc", 0, 11)] * 3 + [("acc", 5, 1)] + [("tau", 0, 11)] * 2 + [("tau", 5, 1)] * 2
    assert [c[4] for c in calls[:4]] == [2, 2, 0, 2] and calls[0][3] is None and calls[1][3] is None and calls[2][3] is not None
    with pytest.raises(ValueError, match=r"vd has shape \(7,\): expected \[13\] or \[4, 13\]"):
        sim.floating_link_accelerations("panda", vd=np.zeros(7, np.float32))
    with pytest.raises(ValueError, match=r"wrenches have shape \(4, 6\): expected \[11, 6\] or \[4, 11, 6\]"):
        sim.floating_forces_from_wrenches("panda", np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match=r"wrenches have shape \(3,\): expected \[6\] or \[4, 6\]"):
        sim.floating_forces_from_link_wrench("panda", "panda_hand", np.zeros(3, np.float32))
    assert not t.any() and len(calls) == 8
    sim._state_t = {}                                               # a horizon view: other tensors than the simulator's own
    for call in (lambda: sim.acquire_floating_link_bias_acceleration_tensor("panda"), sim.refresh_floating_link_bias_acceleration_tensors,
                 lambda: sim.floating_link_accelerations("panda"), lambda: sim.get_actor_link_floating_acceleration_by_name("panda", "panda_hand"),
                 lambda: sim.floating_forces_from_wrenches("panda", np.zeros((11, 6), np.float32)),
                 lambda: sim.floating_forces_from_link_wrench("panda", "panda_hand", np.zeros(6, np.float32))):
        with pytest.raises(RuntimeError, match="per-step only") as e:
            call()
        assert isinstance(e.value, PerStepOnly) and "moving-base link accelerations and wrench forces" in str(e.value)
    assert len(calls) == 8
