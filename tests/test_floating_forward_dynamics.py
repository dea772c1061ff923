"""The no-GPU half of the moving-base forward-dynamics tests (inputs, reference, metrics and tolerances:
floating_forward_dynamics_cases.py; the kernel on the GPU: test_gpu_floating_forward_dynamics.py).

 * the entry is exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states its conventions, the
   wrapper has the accessors; ABI stays 9; the pointer is the tenth of the physics entries and the on-demand plugin units fill it
   through the function that fills the table;
 1 the reference is believed first: on the fixed-base mobile manipulator and heijn (origin and tilted) the same route
   (floating_inverse_dynamics_cases.fixed_parts, jacobian_cases.oracle_M, a dense fp64 solve) reproduces
   Oracle("f64").forward_dynamics in all eight calls within FIXED_ROUTE_AGREE of D_j; on the moving-base robots M_ref vd_ref + bias
   returns the fp32 tau within SOLVE_RESIDUAL of Dtau_j, D_j >= 1 in every row, the condition numbers are printed;
 2 a pass means something: neighbouring envs differ by at least 100 tolerances in (a), every part moves the result by far more;
 3 the device routine (csrc/mppi_device.hpp floating_forward_dynamics), compiled for the host, meets both tolerances for boxer,
   jackal_a, albert and anymal at every env and row in the eight calls; terms = 0 without tau gives exact zeros; gravity alone
   without tau is free fall, (g, 0, ..., 0) as numbers;
 4 v = 0 in the state is bit-equal to the call without the velocity bit, gravity off in the model to the call without the gravity
   bit; a base translated by FAR_SHIFT, with another linear velocity, leaves every bit as it was;
 5 floating_inverse_dynamics(floating_forward_dynamics(tau)) returns tau within the sum of the two routines' (b)-tolerances;
   terms = 0 on tau = e_c gives the columns of M^-1 within the column tolerance;
 6 the host build refuses what the library refuses, without writing;
 7 the wrapper raises PerStepOnly inside a horizon view and NotImplementedError with the library's text for a fixed base (a stub).
Four planted defects of the device routine (a child handed to the base without shift_to_parent, the base's own inertia left out,
rows 0:3 returned as a' without - a0, pass 3 started from a zero angular acceleration of the base) were each shown to fail row 3 on
a scratch copy of the host build: profiles/r20a_planted_defects.txt.

MEASURED (host build, worst e_vd / e_res over the eight calls | the fp32 restatement | tolerances): boxer 4.1e-6 / 5.1e-7 | 7.3e-6 /
1.7e-6 | 1e-4 / 2e-5; jackal_a 1.5e-6 / 5.2e-7 | 2.6e-6 / 1.3e-6 | 5e-5 / 2e-5; albert 4.0e-6 / 6.9e-7 | 6.3e-6 / 1.8e-6 | 1e-4 / 2e-5;
anymal 2.3e-5 / 5.3e-7 | 3.4e-5 / 2.0e-6 | 5e-4 / 5e-5.  Neither cap binds.  The restatement's weight round trip, which costs the
inverse dynamics 4e-4 of the x / y force rows of its gravity-only call (rows at their floor there), is measured here against the
force rows of the FULL tau in every call - hundreds of N - and comes to 2e-6.  Columns of M^-1: e_X 1.0e-6, 8.3e-7, 1.3e-6, 1.3e-6
against 1.4e-6, 1.2e-6, 1.5e-6, 3.5e-6 of the fp32 dense inverse (tolerances 2e-5, 2e-5, 2e-5, 5e-5); the round trip through the host
build of floating_inverse_dynamics returns tau to 2.7e-7 of Dtau at worst."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import floating_forward_dynamics_cases as ff
import floating_inverse_dynamics_cases as fi
import forward_dynamics_cases as fd
import jacobian_cases as jc
from mppiisaac.backend import capi
from scenes import build_scene

ROBOT_IDS = list(ff.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
_vp, _i = C.c_void_p, C.c_int
call_name = lambda c: f"{c[0]}{'+tau' if c[1] else ''}"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entry_is_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_floating_forward_dynamics"] == (_i, [_vp, _vp, _i, _vp])
    assert "mppi_sim_floating_forward_dynamics" in capi.EXPORTED_SYMBOLS
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    lib.mppi_sim_floating_forward_dynamics
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    assert "int mppi_sim_floating_forward_dynamics(mppi_ctx_t *ctx, const float *tau_dev /* [K][6 + n_dof] or NULL */, int terms," in header
    said = header[header.index("What acceleration a base wrench and joint forces GIVE"):header.index("int mppi_sim_floating_forward_dynamics(")]
    for words in ("(root linvel, root angvel, qd)", "mppi_sim_floating_mass_matrix", "EACH ENV'S OWN base pose", "7:13", "time derivative of v",
                  "rows 0-2", "moment about the base origin", "then the joints in DOF","does not depend on where the base stands", "exact zeros",
                  "column c of M^-1", "free fall", "CONTACT forces", "mppi_sim_floating_jacobian", "captured graph", "MPPI_EINVAL", "unknown bits",
                  "use mppi_sim_forward_dynamics", "n_extra_bases > 0", "Refused before", "stay refused"):
        assert words in said, words
    still = header[header.index("STILL refused for a moving base"):header.index("int mppi_sim_floating_jacobian(")]
    listed = still[:still.index("and the fixed-base entries")]
    assert "mppi_sim_link_acceleration" in listed and "mppi_sim_wrench_forces" in listed and "forward_dynamics" not in listed
    assert "mppi_sim_floating_forward_dynamics below" in still
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("floating_forward_dynamics", "acquire_floating_free_acceleration_tensor", "refresh_floating_free_acceleration_tensors",
                 "floating_inverse_mass_matrix"):
        assert callable(getattr(IsaacGymWrapper, name))


def test_the_pointer_is_the_tenth_of_the_physics_entries_and_plugins_carry_it():
    csrc = os.path.join(HERE, "..", "mppi-isaac_amd", "csrc")
    kernels = open(os.path.join(csrc, "mppi_kernels.hpp")).read()
    fill = kernels[kernels.index("void fill_topo_entry_scene(TopoEntry &e) {"):]
    fill = fill[:fill.index("\n}\n")]
    guarded = fill[fill.index("if constexpr (T::NBASE == 1)"):]
    assert "e.sim_floating_forward_dynamics = &launch_sim_floating_forward_dynamics_t<T>;" in guarded
    assert kernels.count("e.sim_floating_forward_dynamics =") == 1
    entry = kernels[kernels.index("struct TopoEntry {"):]
    entry = entry[:entry.index("};")]
    physics = [line.split("(*")[1].split(")")[0] for line in entry.splitlines() if "(*sim_" in line and "// mppi_sim_" in line]
    assert physics[-2:] == ["sim_floating_inverse_dynamics", "sim_floating_forward_dynamics"] and len(physics) == 10, physics
    assert entry.index("sim_floating_inverse_dynamics") < entry.index("sim_floating_forward_dynamics") < entry.index("raise_lds")
    host = open(os.path.join(csrc, "mppi_hip.hip")).read()
    assert "if (!e->sim_floating_forward_dynamics) return fail(MPPI_EUNSUPPORTED" in host
    assert 'floating_entry(c, "mppi_sim_floating_forward_dynamics", "mppi_sim_forward_dynamics", e)' in host
    assert "out[2] = sizeof(mppi::TopoEntry)" in host               # a stale plugin is rebuilt
    # the scene unit of a tree built on demand fills its row through the same function
    assert 'mppi_plugin_fill_scene(mppi::TopoEntry *e) { fill_topo_entry_scene<mppi::Topo<' in host
    # the moving-base kernel and the one routine behind both fronts
    device = open(os.path.join(csrc, "mppi_device.hpp")).read()
    assert "forward_dynamics_pass<false, T>(m0, P, d, qd, tau, terms, qdd);" in device and "forward_dynamics_pass<true, T>(m0, P, d, v, tau, terms, vd);" in device
    assert "__launch_bounds__(kWave) void k_sim_floating_forward_dynamics(" in kernels


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,pose", [("omnipanda", "origin"), ("omnipanda", "tilted"), ("heijn", "origin"), ("heijn", "tilted")])
def test_the_route_reproduces_the_oracle_forward_dynamics_on_fixed_bases(robot, pose, oracle64):
    scene, model, model_off, root, ref, D, M_ref, Dtau = fd.references(robot, pose)[:8]
    dof, tau = fd.inputs(robot, pose)
    K = 8
    q, qd = dof[:K, 0::2].astype(np.float64), dof[:K, 1::2].astype(np.float64)
    parts, gap = fi.fixed_parts(oracle64, model, root, q, qd, np.zeros_like(q))
    M = jc.oracle_M(oracle64, model, root, q)
    mine = ff.solve_calls(M, parts["C"], parts["g"], tau[:K].astype(np.float64))
    worst = {c: fd.e_qdd(mine[c], ref[c][:K], D) for c in ff.ALL_CALLS}
    print(f"\n[{robot} {pose}] the dense route against Oracle('f64').forward_dynamics, e_qdd per call: "
          + ", ".join(f"{call_name(c)} {e:.1e}" for c, e in worst.items()) + f"; Richardson gap {gap:.1e}")
    assert max(worst.values()) <= ff.FIXED_ROUTE_AGREE and gap <= fi.RICHARDSON_AGREE
    assert all(np.abs(ref[c][:K]).max() > 0.0 for c in ff.ALL_CALLS if c != (0, False) and not (c == (ff.ID_GRAVITY, False) and robot == "heijn" and pose == "origin"))


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_reference_is_well_posed(robot):
    r = ff.references(robot)
    dof, roots, tau = ff.inputs(robot)
    K, n = len(dof), dof.shape[1] // 2
    assert K == ff.ROBOTS[robot][2] and all(r.ref[c].shape == (K, 6 + n) for c in ff.ALL_CALLS) and tau.dtype == np.float32
    conds = [np.linalg.cond(M) for M in r.M]
    scaled = [np.linalg.cond(M / np.sqrt(np.outer(np.diag(M), np.diag(M)))) for M in r.M]
    print(f"\n[{robot}] cond(M_ref) {max(conds):.1e} at worst ({r.cond[0]:.1e} in env 0), {max(scaled):.1f} after diagonal scaling ({r.cond[1]:.1f} in env 0)")
    print(f"[{robot}] D_j from {r.D.min():.2f} to {r.D.max():.2f}; M_ref vd_ref + bias - tau: {r.residual:.1e} of Dtau; Richardson levels agree to {r.gap:.1e}")
    assert r.D.min() >= 1.0
    assert r.residual <= ff.SOLVE_RESIDUAL and r.gap <= fi.RICHARDSON_AGREE
    # vd_ref is the vd* the tau was computed for, up to the rounding of tau to fp32 (amplified by the conditioning)
    vd_star = fi.inputs(robot)[2].astype(np.float64)
    back = ff.e_vd(r.ref[ff.FULL], vd_star, r.D)
    print(f"[{robot}] vd_ref against vd*: {back:.1e}")
    assert back <= 1e-4
    # free fall: the dense fp64 solve of the weight gives (g, 0, ..., 0) to cond(M) eps |g| (6 + n) <= 2.1e4 * 2.2e-16 * 9.8 * 18 = 8e-10
    g = np.array([r.model.gravity[j] for j in range(3)], np.float64)
    assert np.abs(r.ref[ff.ID_GRAVITY, False] - np.concatenate([g, np.zeros(3 + n)])).max() <= 1e-9 and g[2] < -9.0
    assert not r.ref[0, False].any()


# ---- 2. a pass means something ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_tell_the_envs_and_the_parts_apart(robot):
    r = ff.references(robot)
    tol_vd, tol_res = ff.tolerances(robot)
    assert 0.0 < tol_vd <= ff.CAP_QDD and 0.0 < tol_res <= ff.CAP_RES and (tol_vd, tol_res) == ff.tolerances_from(r.w32)
    full = r.ref[ff.FULL]
    apart = (np.abs(np.diff(full, axis=0)) / r.D).max(1).min() / tol_vd
    moved = {"tau": ff.e_vd(r.ref[0, True], 0.0, r.D) / tol_vd, "C": ff.e_vd(r.ref[ff.ID_VELOCITY, False], 0.0, r.D) / tol_vd,
             "g": ff.e_vd(r.ref[ff.ID_GRAVITY, False], 0.0, r.D) / tol_vd}
    print(f"\n[{robot}] tol (a) {tol_vd:.0e}, (b) {tol_res:.0e} (fp32 restatement {r.w32[0]:.1e}, {r.w32[1]:.1e}); neighbouring envs differ by at least "
          f"{apart:.0f} tol; the parts move an entry by tau {moved['tau']:.0f}, C {moved['C']:.0f}, g {moved['g']:.0f} tol")
    assert apart >= 100.0 and min(moved.values()) >= 100.0


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_forward_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_forward_dynamics_hostemu.so"))


@pytest.fixture(scope="module")
def hostemu_inverse():
    d = os.path.join(HERE, "hostemu_floating_inverse_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_inverse_dynamics_hostemu.so"))


def host_vd(lib, model, roots, dof, tau, terms, with_tau):
    K, n = len(dof), dof.shape[1] // 2
    roots32, q, qd = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(dof[:, 0::2], np.float32), np.ascontiguousarray(dof[:, 1::2], np.float32)
    tau32 = np.ascontiguousarray(tau, np.float32) if with_tau else None
    vd = np.full((K, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_forward_dynamics(C.byref(model), K, fp(roots32), fp(q), fp(qd), fp(tau32), terms, fp(vd)) == 0
    assert np.isfinite(vd).all()
    return vd


# ---- 3. the tolerances --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_function_on_the_host_meets_the_tolerances(robot, hostemu):
    r = ff.references(robot)
    dof, roots, tau = ff.inputs(robot)
    tol_vd, tol_res = ff.tolerances(robot)
    got = {c: host_vd(hostemu, r.model, roots, dof, tau, *c) for c in ff.ALL_CALLS}
    worst = ff.measure(got, r)
    print(f"\n[{robot}] host build, e_vd / e_res per call (terms, tau given): " + ", ".join(f"{call_name(c)} {e[0]:.1e} / {e[1]:.1e}" for c, e in worst.items())
          + f"; tol {tol_vd:.0e} / {tol_res:.0e}, fp32 restatement {r.w32[0]:.1e} / {r.w32[1]:.1e}")
    assert max(e[0] for e in worst.values()) <= tol_vd and max(e[1] for e in worst.values()) <= tol_res
    assert not got[0, False].any()                                                  # nothing asked for: every product has a zero factor
    n = dof.shape[1] // 2
    g = np.array([r.model.gravity[j] for j in range(3)], np.float32)
    fall = np.tile(np.concatenate([g, np.zeros(3 + n, np.float32)]), (len(dof), 1))
    assert np.array_equal(got[ff.ID_GRAVITY, False], fall)                          # free fall, as numbers


# ---- 4. what the result must not notice ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_zeroed_inputs_are_the_calls_without_their_bit(robot, hostemu):
    r = ff.references(robot)
    dof, roots, tau = (a[:16] for a in ff.inputs(robot))
    a = int(r.model.robot_actor)
    still_dof, still_roots = np.array(dof), np.array(roots)
    still_dof[:, 1::2] = 0.0
    still_roots[:, a, 7:13] = 0.0
    for with_tau in (True, False):
        assert np.array_equal(bits(host_vd(hostemu, r.model, still_roots, still_dof, tau, 3, with_tau)), bits(host_vd(hostemu, r.model, roots, dof, tau, ff.ID_GRAVITY, with_tau)))
        assert np.array_equal(bits(host_vd(hostemu, r.model, still_roots, still_dof, tau, 2, with_tau)), bits(host_vd(hostemu, r.model, roots, dof, tau, 0, with_tau)))
    off_scene = ff.scene_of(robot)
    off_scene.robot.gravity = False
    off = off_scene.to_c()
    assert not bool(off.actors[off.robot_actor].gravity)
    for with_tau in (True, False):
        assert np.array_equal(bits(host_vd(hostemu, off, roots, dof, tau, 3, with_tau)), bits(host_vd(hostemu, r.model, roots, dof, tau, ff.ID_VELOCITY, with_tau)))
    assert not np.array_equal(host_vd(hostemu, r.model, roots, dof, tau, 3, True), host_vd(hostemu, r.model, roots, dof, tau, ff.ID_VELOCITY, True))


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_result_does_not_depend_on_where_the_base_stands_or_how_fast_it_travels(robot, hostemu):
    r = ff.references(robot)
    dof, roots, tau = (a[:16] for a in ff.inputs(robot))
    a = int(r.model.robot_actor)
    near = host_vd(hostemu, r.model, roots, dof, tau, *ff.FULL)
    far = np.array(roots)
    far[:, a, 0:3] += np.asarray(ff.FAR_SHIFT, np.float32)
    far[:, a, 7:10] += np.float32(5.0)
    assert np.array_equal(bits(host_vd(hostemu, r.model, far, dof, tau, *ff.FULL)), bits(near))


# ---- 5. the round trip and the columns of M^-1 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inverse_dynamics_of_the_result_returns_tau(robot, hostemu, hostemu_inverse):
    r = ff.references(robot)
    dof, roots, tau = ff.inputs(robot)
    K, n = len(dof), dof.shape[1] // 2
    vd = host_vd(hostemu, r.model, roots, dof, tau, *ff.FULL)
    back = np.full((K, 6 + n), np.nan, np.float32)
    q, qd = np.ascontiguousarray(dof[:, 0::2]), np.ascontiguousarray(dof[:, 1::2])
    assert hostemu_inverse.emu_floating_inverse_dynamics(C.byref(r.model), K, fp(np.ascontiguousarray(roots)), fp(q), fp(qd), fp(vd), 3, fp(back)) == 0
    e = float((np.abs(back.astype(np.float64) - tau) / r.Dtau[None, :]).max())
    bound = ff.tolerances(robot)[1] + fi.tolerance(robot)
    print(f"\n[{robot}] floating_inverse_dynamics(floating_forward_dynamics(tau)) against tau: {e:.1e} of Dtau (bound {bound:.1e})")
    assert e <= bound


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_unit_rows_give_the_columns_of_the_inverse_mass_matrix(robot, hostemu):
    r = ff.references(robot)
    dof, roots, _ = ff.inputs(robot)
    K, N = len(dof), 6 + dof.shape[1] // 2
    X_ref, tol, w32 = ff.Minv_reference(robot)
    X = np.stack([host_vd(hostemu, r.model, roots, dof, np.tile(np.eye(N, dtype=np.float32)[c], (K, 1)), 0, True) for c in range(N)], axis=2)
    e = ff.e_X(X, X_ref)
    asym = float(np.abs(X - X.transpose(0, 2, 1)).max() / np.abs(X).max())
    print(f"\n[{robot}] columns of M^-1: e_X {e:.1e} (tol {tol:.0e}, fp32 dense inverse {w32:.1e}); asymmetry {asym:.1e} of the largest entry")
    assert e <= tol


# ---- 6. refusals of the host build --------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu):
    out = np.zeros(4096, np.float32)
    r = ff.references("boxer")
    dof, roots, tau = ff.inputs("boxer")
    K = 2

    def call(model, roots, q, qd, tau, terms, o):
        return hostemu.emu_floating_forward_dynamics(C.byref(model), K, fp(roots), fp(q), fp(qd), fp(tau), terms, fp(o))
    q, qd, roots32, tau32 = (np.ascontiguousarray(x) for x in (dof[:K, 0::2], dof[:K, 1::2], roots[:K], tau[:K]))
    # a fixed base; a fixed-base forest
    p = jc.references("franka_panda")
    pq = np.ascontiguousarray(jc.inputs("franka_panda")[0][:K, 0::2])
    proots = np.ascontiguousarray(np.tile(np.asarray(p[2], np.float32), (K, 1, 1)))
    assert call(p[1], proots, pq, pq, None, 3, out) == -2
    actors, init = jc.two_point_robot_actors()
    forest = build_scene(list(actors), init)
    froots = np.ascontiguousarray(np.tile(np.asarray(forest.initial_state()[1], np.float32), (K, 1, 1)))
    fq = np.zeros((K, forest.n_dof), np.float32)
    assert call(forest.to_c(), froots, fq, fq, None, 3, out) == -2
    # a forest of two moving bases
    two = build_scene(["jackal_a", "jackal_b"], [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    tm = two.to_c()
    assert int(tm.n_extra_bases) == 1
    troots = np.ascontiguousarray(np.tile(np.asarray(two.initial_state()[1], np.float32), (K, 1, 1)))
    tq = np.zeros((K, two.n_dof), np.float32)
    assert call(tm, troots, tq, tq, None, 3, out) == -7
    # a null output, unknown bits
    assert call(r.model, roots32, q, qd, tau32, 3, None) == -5
    for terms in (4, 7, -1, 1 << 16):
        assert call(r.model, roots32, q, qd, tau32, terms, out) == -4, terms
    assert not out.any()                                            # nothing was written
    n = q.shape[1]
    assert call(r.model, roots32, q, qd, tau32, 3, out) == 0 and out[:K * (6 + n)].all() and not out[K * (6 + n):].any()


# ---- 7. the wrapper's refusals, through a stub --------------------------------------------------------------------------------------
def test_wrapper_refuses_a_horizon_view_and_a_fixed_base():
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
    text = b"mppi_sim_floating_forward_dynamics: this robot has a fixed base (there are no base columns); use mppi_sim_forward_dynamics"
    calls = []

    def entry(ctx, tau, terms, out):
        calls.append((tau, terms))
        return capi.MPPI_EUNSUPPORTED
    own = {}
    sim = object.__new__(IsaacGymWrapper)
    sim._state_t = sim._state_t_own = own
    sim.num_envs, sim.device, sim._ctx, sim._floating_free_acceleration = 4, "cpu", None, None
    sim.scene = SimpleNamespace(n_dof=7, actor_index=lambda name: 0)
    sim._lib = SimpleNamespace(mppi_sim_floating_forward_dynamics=entry, mppi_last_error=lambda: text)
    sim._reset_envs_if_needed = lambda: None
    t = sim.acquire_floating_free_acceleration_tensor("panda")
    assert tuple(t.shape) == (4, 13) and not t.any() and sim.acquire_floating_free_acceleration_tensor("panda") is t
    for call in (sim.refresh_floating_free_acceleration_tensors, sim.floating_forward_dynamics,
                 lambda: sim.floating_forward_dynamics(tau=np.zeros(13, np.float32), gravity=False), sim.floating_inverse_mass_matrix):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_forward_dynamics"):
            call()
    assert [c[1] for c in calls] == [3, 3, 2, 0] and calls[0][0] is None and calls[2][0] is not None and calls[3][0] is not None
    with pytest.raises(ValueError, match="expected"):
        sim.floating_forward_dynamics(tau=np.zeros(7, np.float32))
    assert not t.any()
    sim._state_t = {}                                               # a horizon view: other tensors than the simulator's own
    for call in (lambda: sim.acquire_floating_free_acceleration_tensor("panda"), sim.refresh_floating_free_acceleration_tensors,
                 sim.floating_forward_dynamics, sim.floating_inverse_mass_matrix):
        with pytest.raises(RuntimeError, match="per-step only") as e:
            call()
        assert isinstance(e.value, PerStepOnly) and "moving-base forward dynamics" in str(e.value)
    assert len(calls) == 4
