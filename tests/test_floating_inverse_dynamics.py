"""The no-GPU half of the moving-base inverse-dynamics tests (inputs, reference, metric and tolerances:
floating_inverse_dynamics_cases.py; the kernel on the GPU: test_gpu_floating_inverse_dynamics.py).

 * the entry is exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states its conventions, the
   wrapper has the accessors; ABI stays 9; the on-demand plugin units fill the pointer through the function that fills the table;
 1 the reference is believed first: on the fixed-base mobile manipulator and heijn (origin and tilted) the body-frame route
   reproduces inverse_dynamics_cases.reference_parts in all three parts within 1e-9 of the joint's torque scale; on the moving-base
   robots the power balance v^T (C v) = v^T Mdot v / 2 holds within 1e-8 of max |C v|, the two Richardson levels agree within
   RICHARDSON_AGREE, M vd is congruence_M @ vd, the base force of g is the robot's weight;
 2 a pass means something: neighbouring envs differ by at least 100 tolerances, every part moves the result by far more than the
   tolerance, an env's inputs do not depend on K;
 3 the device routine (csrc/mppi_device.hpp floating_inverse_dynamics), compiled for the host, meets the tolerance for boxer,
   jackal_a, albert and anymal at every env and row, for the five call shapes of inverse_dynamics_cases.CALLS and the remaining
   three; terms = 0 without vd gives exact zeros; the parts of separate calls sum to the full call to rounding;
 4 a Panda given a moving base, at rest base twist: rows 6: are those of the fixed routine bit for bit;
 5 with the base translated by (420, -310, 0), and with another linear velocity of the base, tau comes out bit for bit the same;
 6 the host build refuses what the library refuses, without writing;
 7 the wrapper raises PerStepOnly inside a horizon view and NotImplementedError with the library's text for a fixed base (a stub).
Four planted defects of the device routine (the w_b x (w_b x d) term of a root body's origin acceleration dropped, the base's own
inertia left out of rows 0:6, the moment handed to the base without d x F, gravity applied to the joints only) were each shown to
fail row 3 on a scratch copy of the host build: profiles/r19a_planted_defects.txt.

MEASURED (host build, worst e over the eight calls / the fp32 restatement / tolerance): boxer 2.2e-5 / 4.1e-4 / 1e-4, jackal_a
5.5e-6 / 2.5e-4 / 1e-4, albert 1.6e-6 / 3.9e-4 / 1e-4, anymal 4.9e-7 / 2.6e-4 / 1e-4 (boxer and the jackal in the velocity-only call,
whose wheel rows stand at their floor; 8.4e-7 and 7.1e-7 otherwise).  The cap binds for every robot: the body-frame restatement
turns the weight into the base's axes and back, and what that leaves in the x / y force rows of the gravity-only call (1e-3 N of
2685 N for boxer) is measured against the floor of those rows, 1e-3 of the weight.  The routine under test sums the
weight in world axes and has exact zeros there."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import floating_inverse_dynamics_cases as fi
import floating_jacobian_cases as fc
import inverse_dynamics_cases as ic
import jacobian_cases as jc
from mppiisaac.backend import capi
from scenes import build_scene

ROBOT_IDS = list(fi.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
_vp, _i = C.c_void_p, C.c_int


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entry_is_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_floating_inverse_dynamics"] == (_i, [_vp, _vp, _i, _vp])
    assert "mppi_sim_floating_inverse_dynamics" in capi.EXPORTED_SYMBOLS
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    lib.mppi_sim_floating_inverse_dynamics
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    assert "int mppi_sim_floating_inverse_dynamics(mppi_ctx_t *ctx, const float *vd_dev /* [K][6 + n_dof] or NULL */, int terms," in header
    said = header[header.index("What forces a motion TAKES of a robot with a MOVING base"):header.index("int mppi_sim_floating_inverse_dynamics(")]
    for words in ("(root linvel, root angvel, qd)", "mppi_sim_floating_mass_matrix", "EACH ENV'S OWN base pose", "7:13", "time derivative of v",
                  "power tau^T v", "rows 0-2", "moment about the base origin", "DOF order", "does not depend on where the base stands", "exact zeros",
                  "column c of the mass matrix", "CONTACT forces", "mppi_sim_floating_jacobian", "captured graph", "MPPI_EINVAL", "unknown bits",
                  "use mppi_sim_inverse_dynamics", "n_extra_bases > 0", "Refused before", "stay refused"):
        assert words in said, words
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("floating_inverse_dynamics", "acquire_floating_bias_force_tensor", "refresh_floating_bias_force_tensors"):
        assert callable(getattr(IsaacGymWrapper, name))


def test_the_pointer_is_the_ninth_of_the_physics_entries_and_plugins_carry_it():
    csrc = os.path.join(HERE, "..", "mppi-isaac_amd", "csrc")
    kernels = open(os.path.join(csrc, "mppi_kernels.hpp")).read()
    fill = kernels[kernels.index("void fill_topo_entry_scene(TopoEntry &e) {"):]
    fill = fill[:fill.index("\n}\n")]
    guarded = fill[fill.index("if constexpr (T::NBASE == 1)"):]
    assert "e.sim_floating_inverse_dynamics = &launch_sim_floating_inverse_dynamics_t<T>;" in guarded
    assert kernels.count("e.sim_floating_inverse_dynamics =") == 1
    entry = kernels[kernels.index("struct TopoEntry {"):]
    entry = entry[:entry.index("};")]
    assert entry.index("sim_floating_mass_matrix") < entry.index("sim_floating_inverse_dynamics") < entry.index("raise_lds")
    host = open(os.path.join(csrc, "mppi_hip.hip")).read()
    assert "if (!e->sim_floating_inverse_dynamics) return fail(MPPI_EUNSUPPORTED" in host
    assert 'floating_entry(c, "mppi_sim_floating_inverse_dynamics", "mppi_sim_inverse_dynamics", e)' in host
    assert "out[2] = sizeof(mppi::TopoEntry)" in host               # a stale plugin is rebuilt


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,pose", [("omnipanda", "origin"), ("omnipanda", "tilted"), ("heijn", "origin"), ("heijn", "tilted")])
def test_body_frame_route_reproduces_the_oracle_inverse_route_on_fixed_bases(robot, pose, oracle64):
    scene, model, root, parts, D, _ = ic.references(robot, pose)
    dof, qdd = ic.inputs(robot, pose)
    K = 8
    mine, gap = fi.fixed_parts(oracle64, model, root, dof[:K, 0::2], dof[:K, 1::2], qdd[:K])
    worst = {p: float((np.abs(mine[p] - parts[p][:K]) / D[None, :]).max()) for p in "MCg"}
    print(f"\n[{robot} {pose}] body-frame route against reference_parts, scaled by D_j: M {worst['M']:.1e}, C {worst['C']:.1e}, g {worst['g']:.1e}; Richardson gap {gap:.1e}")
    assert max(worst.values()) <= 1e-9 and gap <= fi.RICHARDSON_AGREE
    assert all(np.abs(parts[p][:K]).max() > 0.0 for p in "MC") and (pose == "origin" and robot == "heijn" or np.abs(parts["g"][:K]).max() > 0.0)


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_reference_is_well_posed(robot, oracle64):
    r = fi.references(robot)
    dof, roots, vd = fi.inputs(robot)
    K, n = len(dof), dof.shape[1] // 2
    assert K == fi.ROBOTS[robot][2] and all(r.parts[p].shape == (K, 6 + n) for p in "MCg")
    assert bool(r.model.actors[r.model.robot_actor].gravity) and float(r.model.gravity[2]) < -9.0 and not r.model.gravity[0] and not r.model.gravity[1]
    print(f"\n[{robot}] Richardson levels agree to {r.gap:.1e}")
    assert r.gap <= fi.RICHARDSON_AGREE
    # the power balance: the velocity part does the work that changes the kinetic energy at constant v
    scale_C = np.abs(r.parts["C"]).max()
    worst = 0.0
    for k in range(0, K, 16):
        gap, power = fi.power_gap(oracle64, r.model, roots[k], dof[k, 0::2].astype(np.float64), r.v[k], r.parts["C"][k])
        assert abs(power) > 1e-3 * scale_C
        worst = max(worst, abs(gap))
    print(f"[{robot}] v^T (C v) - v^T Mdot v / 2: {worst:.1e} (max |C v| {scale_C:.1f})")
    assert worst <= 1e-8 * scale_C
    # M vd against the congruence sum of the mass-matrix tests; the weight
    Mref = fc.congruence_M(oracle64, r.model, np.asarray(roots[:8], np.float64), dof[:8, 0::2].astype(np.float64), True)
    eM = np.abs(np.einsum("kij,kj->ki", Mref, vd[:8].astype(np.float64)) - r.parts["M"][:8]).max() / np.abs(r.parts["M"]).max()
    total = float(r.model.base_mass) + sum(float(r.model.bodies[i].mass) for i in range(n))
    weight = -float(r.model.gravity[2]) * total
    eg = np.abs(r.parts["g"][:, 0:3] - np.array([0.0, 0.0, weight])).max() / weight
    print(f"[{robot}] M vd against congruence_M @ vd {eM:.1e}; the base force of g against the weight {weight:.1f} N: {eg:.1e}")
    assert eM <= 1e-12 and eg <= 1e-10


# ---- 2. a pass means something ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_tell_the_envs_and_the_parts_apart(robot):
    r = fi.references(robot)
    dof, roots, vd = fi.inputs(robot)
    tol = fi.tolerance(robot)
    a = int(r.model.robot_actor)
    assert 0.0 < tol <= fi.CAP and tol == fi.tolerance_from(r.w32)
    dof0, roots0 = fc.inputs(robot)
    assert np.array_equal(dof[:, 0::2], dof0[:, 0::2]) and np.array_equal(roots[:, a, 0:7], roots0[:, a, 0:7])      # the poses of the Jacobian tests
    assert np.abs(dof[:, 1::2]).max() <= fi.QD_AMP and np.abs(roots[:, a, 7:13]).max() <= fi.TWIST_AMP and np.abs(vd).max() <= fi.VD_AMP
    assert np.abs(dof[:, 1::2]).max() > 0.9 * fi.QD_AMP and np.abs(roots[:, a, 7:13]).max() > 0.9 * fi.TWIST_AMP and np.abs(vd).max() > 0.9 * fi.VD_AMP
    few = fi.draw_rates(dof0[:7], roots0[:7], a)
    assert all(np.array_equal(x, y[:7]) for x, y in zip(few, (dof, roots, vd)))        # an env's inputs do not depend on K
    full = fi.combine(r.parts, *fi.FULL)
    D = fi.scale(full, r.force_rows)
    apart = (np.abs(np.diff(full, axis=0)) / D).max(1).min() / tol
    moved = {p: float((np.abs(r.parts[p]) / D).max() / tol) for p in "MCg"}
    print(f"\n[{robot}] tol {tol:.0e} (fp32 restatement {r.w32:.1e}); neighbouring envs differ by at least {apart:.0f} tol; the parts move an entry by "
          f"M {moved['M']:.0f}, C {moved['C']:.0f}, g {moved['g']:.0f} tol")
    assert apart >= 100.0 and min(moved.values()) >= 100.0


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_inverse_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_inverse_dynamics_hostemu.so"))


def host_tau(lib, model, roots, dof, vd, terms, with_vd):
    K, n = len(dof), dof.shape[1] // 2
    roots32, q, qd = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(dof[:, 0::2], np.float32), np.ascontiguousarray(dof[:, 1::2], np.float32)
    vd32 = np.ascontiguousarray(vd, np.float32) if with_vd else None
    tau = np.full((K, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_inverse_dynamics(C.byref(model), K, fp(roots32), fp(q), fp(qd), fp(vd32), terms, fp(tau)) == 0
    assert np.isfinite(tau).all()
    return tau


# ---- 3. the tolerance ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_function_on_the_host_meets_the_tolerance(robot, hostemu):
    r = fi.references(robot)
    dof, roots, vd = fi.inputs(robot)
    tol = fi.tolerance(robot)
    got, worst = {}, {}
    for terms, with_vd in fi.ALL_CALLS:
        got[terms, with_vd] = host_tau(hostemu, r.model, roots, dof, vd, terms, with_vd)
        worst[terms, with_vd] = fi.e_tau(got[terms, with_vd], fi.combine(r.parts, terms, with_vd), r.force_rows)
    print(f"\n[{robot}] host build, e per call (terms, vd given): " + ", ".join(f"{t}{'+vd' if w else ''} {e:.1e}" for (t, w), e in worst.items())
          + f"; tol {tol:.0e}, fp32 restatement {r.w32:.1e}")
    assert max(worst.values()) <= tol
    assert not got[0, False].any()                                                  # nothing asked for: every product has a zero factor
    # the parts of separate calls sum to the full call to rounding: each of the four results carries a few roundings of its row's
    # scale (the sums pass through intermediate moments of that size), so 16 eps of the row's D - a fiftieth of the tolerance
    parts = got[0, True].astype(np.float64) + got[fi.ID_VELOCITY, False] + got[fi.ID_GRAVITY, False]
    D = fi.scale(fi.combine(r.parts, *fi.FULL), r.force_rows)
    split = float((np.abs(parts - got[fi.FULL]) / D).max())
    print(f"[{robot}] separate calls against the full call: {split / np.finfo(np.float32).eps:.1f} eps of D")
    assert split <= 16 * np.finfo(np.float32).eps
    assert np.array_equal(got[fi.ID_GRAVITY, False][:, 0:2], np.zeros((len(dof), 2), np.float32))        # the weight has no x / y force


# ---- 4. a Panda with a moving base --------------------------------------------------------------------------------------------------
def test_floating_panda_at_rest_carries_the_fixed_panda(hostemu):
    fixed_scene = jc.scene_of("franka_panda")
    scene = build_scene(["panda"], [[0.0, 0.0, 0.0]], robot_overrides={"fixed": False})
    fixed_scene.robot.gravity = scene.robot.gravity = True
    model, fixed_model = scene.to_c(), fixed_scene.to_c()
    dof, qdd = ic.inputs("franka_panda")
    K, n = 12, scene.n_dof
    dof, qdd = np.ascontiguousarray(dof[:K]), np.ascontiguousarray(qdd[:K])
    _, root = scene.initial_state()
    roots = np.tile(np.asarray(root, np.float32), (K, 1, 1))
    assert not roots[:, :, 7:13].any()                                              # the base at rest
    vd = np.zeros((K, 6 + n), np.float32)
    vd[:, 6:] = qdd
    d = os.path.join(HERE, "hostemu_inverse_dynamics")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    fixed_lib = C.CDLL(os.path.join(d, "libinverse_dynamics_hostemu.so"))
    root32 = np.ascontiguousarray(root, np.float32)
    for terms, with_vd in fi.CALLS:
        tau = host_tau(hostemu, model, roots, dof, vd, terms, with_vd)
        for k in range(K):
            ref = np.full(n, np.nan, np.float32)
            q, qd = np.ascontiguousarray(dof[k, 0::2]), np.ascontiguousarray(dof[k, 1::2])
            assert fixed_lib.emu_inverse_dynamics(C.byref(fixed_model), fp(root32), fp(q), fp(qd), fp(qdd[k]) if with_vd else None, terms, fp(ref)) == 0
            assert np.array_equal(bits(tau[k, 6:]), bits(ref)), (terms, with_vd, k)
        if terms & fi.ID_GRAVITY:
            assert np.abs(tau[:, 6:]).max() > 10.0                                  # gravity is on: the shoulder holds tens of N m


# ---- 5. what the result must not notice ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_result_does_not_depend_on_where_the_base_stands_or_how_fast_it_travels(robot, hostemu):
    r = fi.references(robot)
    dof, roots, vd = fi.inputs(robot)
    a = int(r.model.robot_actor)
    near = host_tau(hostemu, r.model, roots[:16], dof[:16], vd[:16], *fi.FULL)
    far = np.array(roots[:16])
    far[:, a, 0:3] += np.asarray(fi.FAR_SHIFT, np.float32)
    assert np.array_equal(bits(host_tau(hostemu, r.model, far, dof[:16], vd[:16], *fi.FULL)), bits(near))
    fast = np.array(roots[:16])
    fast[:, a, 7:10] += np.float32(5.0)
    assert np.array_equal(bits(host_tau(hostemu, r.model, fast, dof[:16], vd[:16], *fi.FULL)), bits(near))


# ---- 6. refusals of the host build --------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu):
    out = np.zeros(4096, np.float32)
    r = fi.references("boxer")
    dof, roots, vd = fi.inputs("boxer")
    K = 2

    def call(model, roots, q, qd, vd, terms, o):
        return hostemu.emu_floating_inverse_dynamics(C.byref(model), K, fp(roots), fp(q), fp(qd), fp(vd), terms, fp(o))
    q, qd, roots32, vd32 = (np.ascontiguousarray(x) for x in (dof[:K, 0::2], dof[:K, 1::2], roots[:K], vd[:K]))
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
    assert call(r.model, roots32, q, qd, vd32, 3, None) == -5
    for terms in (4, 7, -1, 1 << 16):
        assert call(r.model, roots32, q, qd, vd32, terms, out) == -4, terms
    assert not out.any()                                            # nothing was written
    n = q.shape[1]
    assert call(r.model, roots32, q, qd, vd32, 3, out) == 0 and out[:K * (6 + n)].all() and not out[K * (6 + n):].any()


# ---- 7. the wrapper's refusals, through a stub --------------------------------------------------------------------------------------
def test_wrapper_refuses_a_horizon_view_and_a_fixed_base():
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
    text = b"mppi_sim_floating_inverse_dynamics: this robot has a fixed base (there are no base columns); use mppi_sim_inverse_dynamics"
    calls = []

    def entry(ctx, vd, terms, out):
        calls.append((vd, terms))
        return capi.MPPI_EUNSUPPORTED
    own = {}
    sim = object.__new__(IsaacGymWrapper)
    sim._state_t = sim._state_t_own = own
    sim.num_envs, sim.device, sim._ctx, sim._floating_bias_force = 4, "cpu", None, None
    sim.scene = SimpleNamespace(n_dof=7, actor_index=lambda name: 0)
    sim._lib = SimpleNamespace(mppi_sim_floating_inverse_dynamics=entry, mppi_last_error=lambda: text)
    sim._reset_envs_if_needed = lambda: None
    t = sim.acquire_floating_bias_force_tensor("panda")
    assert tuple(t.shape) == (4, 13) and not t.any() and sim.acquire_floating_bias_force_tensor("panda") is t
    for call in (sim.refresh_floating_bias_force_tensors, sim.floating_inverse_dynamics, lambda: sim.floating_inverse_dynamics(vd=np.zeros(13, np.float32), gravity=False)):
        with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_inverse_dynamics"):
            call()
    assert [c[1] for c in calls] == [3, 3, 2] and calls[0][0] is None and calls[2][0] is not None
    with pytest.raises(ValueError, match="expected"):
        sim.floating_inverse_dynamics(vd=np.zeros(7, np.float32))
    assert not t.any()
    sim._state_t = {}                                               # a horizon view: other tensors than the simulator's own
    for call in (lambda: sim.acquire_floating_bias_force_tensor("panda"), sim.refresh_floating_bias_force_tensors, sim.floating_inverse_dynamics):
        with pytest.raises(RuntimeError, match="per-step only") as e:
            call()
        assert isinstance(e.value, PerStepOnly) and "moving-base inverse dynamics" in str(e.value)
    assert len(calls) == 3
