"""The no-GPU half of the moving-base Jacobian / mass-matrix tests (inputs, references, metrics and tolerances:
floating_jacobian_cases.py; the kernels on the GPU: test_gpu_floating_jacobian_mass.py).

 * the two entries are exported by the cross-compiled libmppi_hip.so and declared by the binding, the header states their conventions,
   the wrapper has the accessors; ABI stays 9; the on-demand plugin units fill their launch-table row through the very function that
   fills the two pointers;
 1 the reference routes are believed first: the congruence sum over the oracle's body-frame Jacobians reproduces the oracle-inverse
   matrices of jacobian_cases.oracle_M on the fixed-base Panda, mobile manipulator and heijn within 1e-10; the base columns of J_ref
   are [[1, -[r]x], [0, 1]] built in fp64 from the oracle's positions; J_ref v is the oracle's velocity columns under (twist, qd);
   M_ref is symmetric, positive definite, its [0:3, 0:3] block the total mass;
 2 a pass means something: every env has roll, pitch and yaw of its own, neighbouring envs differ by at least 100 tolerances in J and
   in M, the fp32 route sits within a tenth of the tolerances, an env's inputs do not depend on K;
 3 the device routines (csrc/mppi_device.hpp), compiled for the host, meet the tolerances for boxer, jackal_a, albert and anymal at
   every env, body and entry; M == M^T bit for bit, Cholesky succeeds, M[0:3, 0:3] is the total mass; a sub-range of bodies is the
   slice of the full call bit for bit;
 4 a contact scene with a free and a static actor: the blocks of their bodies are exact zeros;
 5 a Panda with a moving base at the joint positions of tests/golden/mass_matrices.json: the [6:, 6:] block is the URDF-route matrix,
   the joint columns of J are those of the fixed routine bit for bit;
 6 with the base translated by (420, -310, 0), same orientation and joints, J and M come out bit for bit the same;
 7 the host build refuses what the library refuses - a fixed base, a forest of moving bases, null pointers, a range outside
   [0, n_rb) - without writing.
Four planted defects of the device routines (the base lever arm with the wrong sign, the base's own inertia left out of the base
block, the coupling moment not moved to the base origin, the base columns read from env 0's pose) were each shown to fail row 3 or 6 on
a scratch copy of the host build: profiles/r18a_planted_defects.txt."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import floating_jacobian_cases as fc
import jacobian_cases as jc
from mppiisaac.backend import capi
from scenes import build_scene

ROBOT_IDS = list(fc.ROBOTS)
HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
_vp, _i = C.c_void_p, C.c_int


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entries_are_exported_and_declared():
    assert capi._SIGNATURES["mppi_sim_floating_jacobian"] == (_i, [_vp, _i, _i, _vp])
    assert capi._SIGNATURES["mppi_sim_floating_mass_matrix"] == (_i, [_vp, _vp])
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    for name in ("mppi_sim_floating_jacobian", "mppi_sim_floating_mass_matrix"):
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)
        assert f"int {name}(" in header
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9
    said = header[header.index("J and M of a robot with a MOVING base"):header.index("int mppi_sim_floating_jacobian(")]
    for words in ("(root linvel, root angvel, qd)", "columns 7:10", "10:13", "DOF order", "rows 0-2 linear", "rigid-body index", "[[1, -[r]x], [0, 1]]",
                  "never as a difference of", "welded to the base", "exact zero", "symmetric bit for bit", "[[m 1, -[h]x], [[h]x, I]]",
                  "base_mass / base_h / base_Io", "ITS OWN base pose", "captured graph", "MPPI_EINVAL", "mppi_sim_jacobian / mppi_sim_mass_matrix",
                  "n_extra_bases > 0", "Refused before", "STILL refused", "mppi_sim_inverse_dynamics", "mppi_sim_wrench_forces"):
        assert words in said, words
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("acquire_floating_jacobian_tensor", "acquire_floating_mass_matrix_tensor", "refresh_floating_jacobian_tensors",
                 "refresh_floating_mass_matrix_tensors", "get_actor_link_floating_jacobian_by_name"):
        assert callable(getattr(IsaacGymWrapper, name))


def test_plugin_units_fill_the_two_pointers_through_the_same_table():
    """no on-demand moving-base tree is built on the GPU (the scene units take tens of seconds): the source of a plugin's scene unit
    (written by mppi_hip.hip) and the generated units of the shipped trees call ONE function, and that function fills the pointers"""
    csrc = os.path.join(HERE, "..", "mppi-isaac_amd", "csrc")
    kernels = open(os.path.join(csrc, "mppi_kernels.hpp")).read()
    fill = kernels[kernels.index("void fill_topo_entry_scene(TopoEntry &e) {"):]
    fill = fill[:fill.index("\n}\n")]
    assert "e.sim_floating_jacobian = &launch_sim_floating_jacobian_t<T>;" in fill and "e.sim_floating_mass_matrix = &launch_sim_floating_mass_matrix_t<T>;" in fill
    assert "if constexpr (T::NBASE == 1)" in fill
    assert kernels.count("e.sim_floating_jacobian =") == 1 and kernels.count("e.sim_floating_mass_matrix =") == 1
    entry = kernels[kernels.index("struct TopoEntry {"):]
    entry = entry[:entry.index("};")]
    assert entry.index("sim_wrench_forces") < entry.index("sim_floating_jacobian") < entry.index("sim_floating_mass_matrix")
    host = open(os.path.join(csrc, "mppi_hip.hip")).read()
    assert 'mppi_plugin_fill_scene(mppi::TopoEntry *e) { fill_topo_entry_scene<mppi::Topo<' in host        # the plugin's scene unit
    assert "out[2] = sizeof(mppi::TopoEntry)" in host                                                       # a stale plugin is rebuilt
    import __graft_entry__ as g
    import inspect
    assert "fill_topo_entry_scene<mppi::Topo<" in inspect.getsource(g.generate_sources)                     # the shipped units
    # each entry checks its own pointer
    for name in ("sim_floating_jacobian", "sim_floating_mass_matrix"):
        assert f"if (!e->{name}) return fail(MPPI_EUNSUPPORTED" in host


# ---- 1. the reference routes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["franka_panda", "omnipanda", "heijn"])
def test_congruence_route_reproduces_the_oracle_inverse_on_fixed_bases(robot, oracle64):
    scene, model, root, _, _, _, _ = jc.references(robot)
    q = jc.inputs(robot)[0][:12, 0::2].astype(np.float64)
    e = jc.e_M(fc.congruence_M(oracle64, model, root, q, False), jc.oracle_M(oracle64, model, root, q))
    print(f"\n[{robot}] congruence sum over body-frame Jacobians against the oracle-inverse M: e_M {e:.1e}")
    assert e <= 1e-10


@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_references_are_well_posed(robot, oracle64):
    r = fc.references(robot)
    dof, roots = fc.inputs(robot)
    K, n = len(dof), dof.shape[1] // 2
    a = int(r.model.robot_actor)
    assert K == fc.ROBOTS[robot][2] and r.J.shape == (K, r.model.n_rb, 6, 6 + n) and r.M.shape == (K, 6 + n, 6 + n)
    worst_cols = worst_v = 0.0
    v = fc.generalised_velocity(dof, roots, a)
    for k in range(0, K, 5):
        rows = oracle64.rigid_body_state(r.model, roots[k], dof[k, 0::2], dof[k, 1::2])[0]
        # the base columns, from positions alone; the root link is the base frame
        assert np.array_equal(rows[r.first, 0:3], roots[k, a, 0:3].astype(np.float64))
        worst_cols = max(worst_cols, float(np.abs(r.J[k, r.first:r.first + r.L, :, 0:6] - fc.base_columns(rows[r.first:r.first + r.L], rows[r.first])).max()))
        # J_ref v = the oracle's velocity columns at the env's own twist and rates
        worst_v = max(worst_v, float(np.abs(r.J[k] @ v[k] - rows[:, 7:13]).max()))
    print(f"\n[{robot}] J_ref base columns against [[1, -[r]x], [0, 1]] of the oracle's positions {worst_cols:.1e}; J_ref v against the velocity columns {worst_v:.1e}")
    # (fp64 with the oracle's velocities carried about the WORLD origin and a quaternion rounded to fp32, unit to 6e-8: a few 1e-13)
    assert worst_cols <= 1e-11 and worst_v <= 1e-12
    # M_ref: symmetric, positive definite, the total mass on the diagonal of its first block
    total = float(r.model.base_mass) + sum(float(r.model.bodies[i].mass) for i in range(n))
    assert np.abs(r.M - r.M.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(r.M).max()
    for k in range(K):
        np.linalg.cholesky(r.M[k])
    assert np.abs(r.M[:, 0:3, 0:3] - total * np.eye(3)).max() <= 1e-10 * total


# ---- 2. a pass means something ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_inputs_tell_the_envs_apart(robot):
    r = fc.references(robot)
    dof, roots = fc.inputs(robot)
    tol_J, tol_M = fc.tolerances(robot)
    a = int(r.model.robot_actor)
    assert 0.0 < tol_J <= fc.CAP and 0.0 < tol_M <= fc.CAP
    assert r.w32[0] <= 0.1 * tol_J and r.w32[1] <= 0.1 * tol_M     # the rule: ten times the fp32 route's own deviation, rounded up
    # every env: a unit quaternion with roll, pitch and yaw all non-zero (no component of the vector part vanishes with all three
    # angles at least 0.2 rad), a position within +-2 m, joints of its own
    quat = roots[:, a, 3:7].astype(np.float64)
    assert np.abs(np.linalg.norm(quat, axis=1) - 1.0).max() < 1e-6
    R = np.stack([fc.quat_R(x, np.float64) for x in quat])
    assert (np.abs(R[:, 2, 0]) > 0.1).all() and (np.abs(R[:, 2, 1]) > 0.05).all() and (np.abs(R[:, 1, 0]) > 0.05).all()   # pitch, roll, yaw
    assert np.abs(roots[:, a, 0:3]).max() <= fc.POS_AMP and np.abs(roots[:, a, 7:13]).max() <= fc.TWIST_AMP and np.abs(dof[:, 1::2]).max() <= fc.QD_AMP
    # an env's inputs do not depend on how many envs there are
    few = fc.draw_inputs(r.scene, 7)
    assert np.array_equal(few[0], dof[:7]) and np.array_equal(few[1], roots[:7])
    if len(dof) > 1:
        dJ = np.abs(np.diff(r.J, axis=0)).max((1, 2, 3)).min() / tol_J
        d = np.sqrt(np.einsum("kii->ki", r.M[:-1]))
        dM = (np.abs(np.diff(r.M, axis=0)) / (d[:, :, None] * d[:, None, :])).max((1, 2)).min() / tol_M
        print(f"\n[{robot}] neighbouring envs differ by at least {dJ:.0f} tol_J in J and {dM:.0f} tol_M in M")
        assert dJ >= 100.0 and dM >= 100.0


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_floating_jacobian")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libfloating_jacobian_hostemu.so"))


def host_J(lib, model, roots, q, rb_first=0, rb_count=None):
    K, n = q.shape
    rb_count = int(model.n_rb) - rb_first if rb_count is None else rb_count
    roots32, q32 = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(q, np.float32)
    J = np.full((K, rb_count, 6, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_jacobian(C.byref(model), K, fp(roots32), fp(q32), rb_first, rb_count, fp(J)) == 0
    assert np.isfinite(J).all()
    return J


def host_M(lib, model, roots, q):
    K, n = q.shape
    roots32, q32 = np.ascontiguousarray(roots, np.float32), np.ascontiguousarray(q, np.float32)
    M = np.full((K, 6 + n, 6 + n), np.nan, np.float32)
    assert lib.emu_floating_mass_matrix(C.byref(model), K, fp(roots32), fp(q32), fp(M)) == 0
    assert np.isfinite(M).all()
    return M


def check_M_properties(M, model, tol_M):
    """M == M^T bit for bit, positive definite, M[0:3, 0:3] = total mass x 1 within the tolerance (scale-free: relative to the mass)"""
    n = M.shape[1] - 6
    total = float(model.base_mass) + sum(float(model.bodies[i].mass) for i in range(n))
    assert np.array_equal(bits(M), bits(M.transpose(0, 2, 1)))
    for k in range(len(M)):
        np.linalg.cholesky(M[k].astype(np.float64))
    assert np.abs(M[:, 0:3, 0:3].astype(np.float64) - total * np.eye(3)).max() <= tol_M * total


# ---- 3. the tolerances --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_device_functions_on_the_host_meet_the_tolerances(robot, hostemu):
    r = fc.references(robot)
    dof, roots = fc.inputs(robot)
    tol_J, tol_M = fc.tolerances(robot)
    q = dof[:, 0::2]
    J, M = host_J(hostemu, r.model, roots, q), host_M(hostemu, r.model, roots, q)
    eJ, eM = fc.e_J(J, r.J), fc.e_M(M, r.M)
    print(f"\n[{robot}] host build: e_J {eJ:.1e} (tol {tol_J:.0e}), e_M {eM:.1e} (tol {tol_M:.0e}); fp32 route {r.w32[0]:.1e} / {r.w32[1]:.1e}")
    assert eJ <= tol_J and eM <= tol_M
    check_M_properties(M, r.model, tol_M)
    # links welded to the base: the base columns and nothing else
    welded = [r.first + l for l, L in enumerate(r.scene.robot_model["links"]) if L["body"] < 0]
    assert welded and not bits(J[:, welded][:, :, :, 6:]).any() and (J[:, welded, 0, 0] == 1.0).all()
    # a sub-range of bodies is the slice of the full call
    B = int(r.model.n_rb)
    for first, count in ((0, 1), (B - 1, 1), (B // 3, B // 2), (0, B)):
        assert np.array_equal(bits(host_J(hostemu, r.model, roots, q, first, count)), bits(J[:, first:first + count]))


# ---- 4. the bodies of other actors --------------------------------------------------------------------------------------------------
def test_bodies_of_box_actors_get_exact_zero_blocks(hostemu):
    scene = build_scene(fc.PUSH_SCENE, [[0.0, 2.5, 0.05]])
    model = scene.to_c()
    dof, roots = fc.draw_inputs(scene, 16)
    r = fc.references_at(scene, model, roots, dof[:, 0::2])
    tol_J, tol_M = fc.tolerances("boxer")
    assert r.w32[0] <= 0.1 * tol_J and r.w32[1] <= 0.1 * tol_M     # boxer's tolerances fit the scene's inputs
    J, M = host_J(hostemu, model, roots, dof[:, 0::2]), host_M(hostemu, model, roots, dof[:, 0::2])
    assert (~r.robot_rb).sum() == 2 and not r.J[:, ~r.robot_rb].any()
    assert not bits(J[:, ~r.robot_rb]).any()                       # +0.0 everywhere, base columns included
    assert fc.e_J(J, r.J) <= tol_J and fc.e_M(M, r.M) <= tol_M
    for b in np.flatnonzero(~r.robot_rb):
        assert not bits(host_J(hostemu, model, roots, dof[:, 0::2], int(b), 1)).any()


# ---- 5. a Panda with a moving base --------------------------------------------------------------------------------------------------
def test_floating_panda_carries_the_fixed_panda(hostemu):
    fixed_scene = jc.scene_of("franka_panda")
    scene = build_scene(["panda"], [[0.0, 0.0, 0.0]], robot_overrides={"fixed": False})
    model, fixed_model = scene.to_c(), fixed_scene.to_c()
    golden = jc.golden_M("franka_panda", fixed_scene)
    dof = jc.inputs("franka_panda")[0][:len(golden)]
    q = np.ascontiguousarray(dof[:, 0::2])
    _, root = scene.initial_state()
    roots = np.tile(np.asarray(root, np.float32), (len(q), 1, 1))
    tol_M = jc.tolerances("franka_panda")[1]
    M = host_M(hostemu, model, roots, q)
    e = jc.e_M(M[:, 6:, 6:], np.stack(golden))
    print(f"\n[floating Panda] the [6:, 6:] block against the URDF-route matrices: e_M {e:.1e} (tol {tol_M:.0e})")
    assert len(golden) == 3 and e <= tol_M
    check_M_properties(M, model, tol_M)
    # the joint columns are those of the fixed routine, bit for bit (same base pose, same joints)
    d = os.path.join(HERE, "hostemu_jacobian")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    fixed_lib = C.CDLL(os.path.join(d, "libjacobian_hostemu.so"))
    J = host_J(hostemu, model, roots, q)
    assert int(fixed_model.n_rb) == int(model.n_rb)
    for k in range(len(q)):
        Jf = np.full((int(fixed_model.n_rb), 6, q.shape[1]), np.nan, np.float32)
        assert fixed_lib.emu_jacobian(C.byref(fixed_model), fp(np.ascontiguousarray(root, np.float32)), fp(q[k]), fp(Jf)) == 0
        assert np.array_equal(bits(J[k, :, :, 6:]), bits(Jf))


# ---- 6. translation independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOT_IDS)
def test_results_do_not_depend_on_where_the_base_stands(robot, hostemu):
    r = fc.references(robot)
    dof, roots = fc.inputs(robot)
    q = dof[:16, 0::2]
    far = np.array(roots[:16])
    far[:, int(r.model.robot_actor), 0:3] += np.asarray(fc.FAR_SHIFT, np.float32)
    assert np.array_equal(bits(host_J(hostemu, r.model, far, q)), bits(host_J(hostemu, r.model, roots[:16], q)))
    assert np.array_equal(bits(host_M(hostemu, r.model, far, q)), bits(host_M(hostemu, r.model, roots[:16], q)))


# ---- 7. refusals of the host build --------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu):
    out = np.zeros(8192, np.float32)
    r = fc.references("boxer")
    dof, roots = fc.inputs("boxer")
    K, B = 2, int(r.model.n_rb)
    q, roots32 = np.ascontiguousarray(dof[:K, 0::2]), np.ascontiguousarray(roots[:K])
    jac = lambda model, roots, q, first, count, o: hostemu.emu_floating_jacobian(C.byref(model), K, fp(roots), fp(q), first, count, fp(o))
    mas = lambda model, roots, q, o: hostemu.emu_floating_mass_matrix(C.byref(model), K, fp(roots), fp(q), fp(o))
    # a fixed base; a fixed-base forest
    p = jc.references("franka_panda")
    pq = np.ascontiguousarray(jc.inputs("franka_panda")[0][:K, 0::2])
    proots = np.ascontiguousarray(np.tile(np.asarray(p[2], np.float32), (K, 1, 1)))
    assert jac(p[1], proots, pq, 0, int(p[1].n_rb), out) == -2 and mas(p[1], proots, pq, out) == -2
    actors, init = jc.two_point_robot_actors()
    forest = build_scene(list(actors), init)
    fm = forest.to_c()
    froots = np.ascontiguousarray(np.tile(np.asarray(forest.initial_state()[1], np.float32), (K, 1, 1)))
    fq = np.zeros((K, forest.n_dof), np.float32)
    assert jac(fm, froots, fq, 0, int(fm.n_rb), out) == -2 and mas(fm, froots, fq, out) == -2
    # a forest of two moving bases (conf/mppi/multi-jackal.yaml)
    two = build_scene(["jackal_a", "jackal_b"], [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    tm = two.to_c()
    assert int(tm.n_extra_bases) == 1
    troots = np.ascontiguousarray(np.tile(np.asarray(two.initial_state()[1], np.float32), (K, 1, 1)))
    tq = np.zeros((K, two.n_dof), np.float32)
    assert jac(tm, troots, tq, 0, int(tm.n_rb), out) == -7 and mas(tm, troots, tq, out) == -7
    # null pointers
    assert jac(r.model, roots32, q, 0, B, None) == -5 and mas(r.model, roots32, q, None) == -5
    # a range outside [0, n_rb)
    for first, count in ((-1, 1), (0, 0), (0, B + 1), (B, 1), (B - 1, 2), (1, 1 << 31 - 1)):
        assert jac(r.model, roots32, q, first, count, out) == -6, (first, count)
    assert not out.any()                                            # nothing was written
    n = q.shape[1]
    assert jac(r.model, roots32, q, 0, B, out) == 0 and out[:K * B * 6 * (6 + n)].any() and not out[K * B * 6 * (6 + n):].any()
    out[:] = 0.0
    assert mas(r.model, roots32, q, out) == 0 and out[:K * (6 + n) ** 2].any() and not out[K * (6 + n) ** 2:].any()
