"""The no-GPU half of the whole-robot tests: centre of mass, momentum, energy and the centroidal momentum matrix (inputs, references,
metrics and tolerances: centroidal_cases.py; the kernels on the GPU: test_gpu_centroidal.py).

 * the three entries are exported by the cross-compiled libmppi_hip.so and declared by the header and the binding, ABI stays 9; the four
   launch-table pointers stand at the end of TopoEntry and are filled once each under the NBASE == 1 guards - the fixed ones by the
   contact-free unit's function, the moving ones by the contact-scene unit's (the on-demand plugin units go through both); each
   routine has exactly two fronts;
 1 the reference is believed first: A_ref v = (p, L)_ref and T_ref = v^T M_ref v / 2 with floating_jacobian_cases.congruence_M to
   1e-12 of the quantity's scale; for a moving base A_ref is the shifted rows 0:6 of congruence_M;
 2 a pass means something: every pair of neighbouring envs differs by at least 100 tolerances in some quantity of the momentum row
   and in some half of the matrix (an env mix-up swaps a whole row of an entry);
 3 the device routines (csrc/mppi_device.hpp), compiled for the host, meet the tolerances on every robot and pose, at every env and
   entry; with gravity off V is exact zeros;
 4 under FAR_SHIFT of a moving base m, p, L, T and A are bit for bit unchanged and c moves by the shift to within one ulp of the
   shifted coordinate;
 5 a Panda with a moving base at rest carries the fixed Panda: T and p bit for bit (the base's own body adds zeros), and - once the
   base body's own share is taken out in fp64: its mass moves c, L is taken about another point, V gains its weight - c, L and V
   within the Panda's tolerances;
 6 the host build refuses what the library refuses, without writing;
 7 the wrapper raises PerStepOnly inside a horizon view and NotImplementedError with the library's text for the wrong base (a stub).
Four planted defects of the device routines (the base's own body left out; L taken about the base origin instead of c; a prismatic
column built as a revolute one; h x v dropped from the angular momentum) were each shown to fail row 3 on a scratch copy of the host
build: profiles/r22a_planted_defects.txt."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import centroidal_cases as cc
import floating_jacobian_cases as fc
import jacobian_cases as jc
from mppiisaac.backend import capi
from scenes import build_scene

HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None
_vp, _i = C.c_void_p, C.c_int
ENTRIES = ("mppi_sim_momentum", "mppi_sim_centroidal_matrix", "mppi_sim_floating_centroidal_matrix")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_entries_are_exported_and_declared():
    lib = C.CDLL(capi.LIB_PATH)     # loads without a GPU
    for name in ENTRIES:
        assert capi._SIGNATURES[name] == (_i, [_vp, _vp])
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)
    assert lib.mppi_abi_version() == capi.ABI_VERSION == 9 and capi.MOMENTUM_FLOATS == 12
    header = open(os.path.join(HERE, "..", "include", "mppi_hip.h")).read()
    assert "#define MPPI_MOMENTUM_FLOATS 12\n" in header
    assert "int mppi_sim_momentum(mppi_ctx_t *ctx, float *out_dev /* [K][12] */);" in header
    assert "int mppi_sim_centroidal_matrix(mppi_ctx_t *ctx, float *A_dev /* [K][6][n_dof] */);" in header
    assert "int mppi_sim_floating_centroidal_matrix(mppi_ctx_t *ctx, float *A_dev /* [K][6][6 + n_dof] */);" in header
    # the group stands at the end of the mppi_sim_* block of physics entries
    assert header.index("int mppi_sim_floating_wrench_forces(") < header.index("THE ROBOT AS A WHOLE") < header.index("int mppi_sim_momentum(") \
        < header.index("int mppi_sim_accumulate_cost(")
    said = header[header.index("THE ROBOT AS A WHOLE"):header.index("#define MPPI_MOMENTUM_FLOATS")]
    for words in ("mppi_sim_materialise", "world axes", "base_mass / base_h / base_Io", "the whole forest", "Free box and sphere actors", "DEVIATION",
                  "welded to a FIXED base", "column 0 the total mass", "1:4 the centre of mass", "4:7 the linear momentum", "7:10",
                  "angular momentum L about c", "10 the kinetic energy", "11 the potential energy V = -m g . c", "exactly 0", "0:7 and 7:13",
                  "added to c once", "do not depend on where the base stands", "A v = (p, L)", "Jacobian of the centre of mass",
                  "(root linvel, root angvel, qd)", "mppi_sim_floating_jacobian", "A[3:6] = M[3:6, :] - [r]x M[0:3, :]", "captured graph",
                  "MPPI_EINVAL", "n_extra_bases >", "names the\n * other entry", "Refused before any launch"):
        assert words in said, words
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper
    for name in ("acquire_momentum_tensor", "refresh_momentum_tensors", "centre_of_mass", "robot_momentum", "kinetic_energy", "potential_energy",
                 "acquire_centroidal_matrix_tensor", "refresh_centroidal_matrix_tensors", "acquire_floating_centroidal_matrix_tensor",
                 "refresh_floating_centroidal_matrix_tensors", "com_jacobian"):
        assert callable(getattr(IsaacGymWrapper, name))


def test_the_pointers_end_the_row_are_filled_once_under_the_guards_and_each_routine_has_two_fronts():
    csrc = os.path.join(HERE, "..", "mppi-isaac_amd", "csrc")
    kernels = open(os.path.join(csrc, "mppi_kernels.hpp")).read()
    entry = kernels[kernels.index("struct TopoEntry {"):]
    entry = entry[:entry.index("};")]
    order = [entry.index(f"(*{name})") for name in ("sim_floating_wrench_forces", "sim_momentum", "sim_centroidal_matrix", "sim_floating_momentum",
                                                      "sim_floating_centroidal_matrix")]
    assert order == sorted(order) and entry.rstrip().endswith("(*sim_floating_centroidal_matrix)(mppi_ctx *, float *);")       # nothing behind them
    for unit, names in (("free", ("momentum", "centroidal_matrix")), ("scene", ("floating_momentum", "floating_centroidal_matrix"))):
        fill = kernels[kernels.index(f"void fill_topo_entry_{unit}(TopoEntry &e) {{"):]
        fill = fill[:fill.index("\n}\n")]
        guarded = fill[fill.index("if constexpr (T::NBASE == 1)"):]
        for name in names:
            assert f"e.sim_{name} = &launch_sim_{name}_t<T>;" in guarded
            assert kernels.count(f"e.sim_{name} =") == 1
    for kernel in ("k_sim_momentum", "k_sim_centroidal_matrix", "k_sim_floating_centroidal_matrix"):
        assert f"__launch_bounds__(kWave) void {kernel}(" in kernels
    host = open(os.path.join(csrc, "mppi_hip.hip")).read()
    assert "out[2] = sizeof(mppi::TopoEntry)" in host               # a stale plugin is rebuilt
    assert 'mppi_plugin_fill_scene(mppi::TopoEntry *e) { fill_topo_entry_scene<mppi::Topo<' in host
    for name in ENTRIES:
        assert f'whole_robot_entry(c, "{name}", e)' in host and f'fail(MPPI_EINVAL, "{name}: null output")' in host
    device = open(os.path.join(csrc, "mppi_device.hpp")).read()
    for front in ("momentum_pass<false, T>(", "momentum_pass<true, T>(", "centroidal_matrix_pass<false, T>(", "centroidal_matrix_pass<true, T>("):
        assert device.count(front) == 1, front


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------------
def _references(case):
    return cc.moving_references(case) if isinstance(case, str) else cc.fixed_references(*case)


def _inputs(case):
    return cc.moving_inputs(case) if isinstance(case, str) else cc.fixed_inputs(*case)


ALL_CASES = cc.FIXED_CASES + list(cc.MOVING_ROBOTS)
CASE_IDS = [c if isinstance(c, str) else "-".join(c) for c in ALL_CASES]
robot_of = lambda case: case if isinstance(case, str) else case[0]


@pytest.mark.parametrize("case", ALL_CASES, ids=CASE_IDS)
def test_reference_is_well_posed(case, oracle64):
    r = _references(case)
    dof, roots = _inputs(case)
    moving = cc.is_moving(r.model)
    K, n = len(dof), dof.shape[1] // 2
    N = n + (6 if moving else 0)
    assert r.rows.shape == (K, 12) and r.A.shape == (K, 6, N) and r.v.shape == (K, N)
    assert bool(r.model.actors[r.model.robot_actor].gravity) and float(r.model.gravity[2]) < -9.0
    total = sum(float(r.model.bodies[i].mass) for i in range(n)) + (float(r.model.base_mass) if moving else 0.0)
    assert np.abs(r.rows[:, 0] - total).max() <= 1e-12 * total
    Av = np.einsum("kri,ki->kr", r.A, r.v)
    e_p, e_L = np.abs(Av[:, 0:3] - r.rows[:, 4:7]).max() / r.D["p"], np.abs(Av[:, 3:6] - r.rows[:, 7:10]).max() / r.D["L"]
    k8 = slice(0, 8)
    rts = np.asarray(roots[k8], np.float64) if moving else roots
    M = fc.congruence_M(oracle64, r.model, rts, dof[k8, 0::2].astype(np.float64), moving)
    e_T = np.abs(0.5 * np.einsum("ki,kij,kj->k", r.v[k8], M, r.v[k8]) - r.rows[k8, 10]).max() / r.D["T"]
    print(f"\n[{CASE_IDS[ALL_CASES.index(case)]}] A_ref v against (p, L)_ref: {e_p:.1e} / {e_L:.1e}; T_ref against v^T M_ref v / 2: {e_T:.1e}; scales "
          + ", ".join(f"{k} {v:.3g}" for k, v in r.D.items()))
    assert max(e_p, e_L, e_T) <= 1e-12
    if moving:
        a = int(r.model.robot_actor)
        shifted = cc.shifted_mass_rows(M, r.rows[k8, 1:4] - np.asarray(roots[k8], np.float64)[:, a, 0:3])
        e_A = np.abs(shifted - r.A[k8]).max() / max(r.D["A_lin"], r.D["A_ang"])
        print(f"[{case}] A_ref against the shifted rows 0:6 of congruence_M: {e_A:.1e}")
        assert e_A <= 1e-12
        assert not np.abs(r.A[:, 3:6, 0:3]).max() > 1e-12 * r.D["A_lin"]                # a translation carries no angular momentum about c
    g = np.array([r.model.gravity[j] for j in range(3)])
    assert np.abs(r.rows[:, 11] + r.rows[:, 0] * (r.rows[:, 1:4] @ g)).max() <= 1e-12 * r.D["V"]


# ---- 2. a pass means something ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=CASE_IDS)
def test_inputs_tell_the_envs_apart(case):
    r = _references(case)
    tol = cc.tolerances(robot_of(case))
    assert set(tol) == set(cc.QUANTITIES) and all(0.0 <= t <= cc.CAP for t in tol.values())
    steps = {}
    for name, ref in r.ref.items():
        if name == "m" or tol[name] == 0.0:
            continue                                                # the mass is the same in every env
        steps[name] = np.abs(np.diff(ref, axis=0)).reshape(len(ref) - 1, -1).max(1) / r.D[name] / tol[name]
    # an env mix-up swaps a whole row of an entry: every pair of neighbours must differ by 100 tolerances in some quantity of the momentum
    # row and in some half of the matrix (a scalar like T can come close between two envs by chance; the vectors cannot all do so)
    row = np.max([steps[k] for k in ("c", "p", "L", "T", "V") if k in steps], axis=0).min()
    mat = np.max([steps[k] for k in ("A_lin", "A_ang")], axis=0).min()
    print(f"\n[{CASE_IDS[ALL_CASES.index(case)]}] tolerances " + ", ".join(f"{k} {v:.0e}" for k, v in tol.items()) + "; fp32 route "
          + ", ".join(f"{k} {v:.1e}" for k, v in r.w32.items()) + "; neighbouring envs differ by at least (in tolerances) "
          + ", ".join(f"{k} {v.min():.0f}" for k, v in steps.items()) + f"; every pair by {row:.0f} in the row, {mat:.0f} in the matrix")
    assert row >= 100.0 and mat >= 100.0


# ---- the host build -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostemu():
    d = os.path.join(HERE, "hostemu_centroidal")
    subprocess.run(["make", "-C", d, "-s"], check=True)
    return C.CDLL(os.path.join(d, "libcentroidal_hostemu.so"))


def host(lib, model, roots, dof):
    """-> (rows [K][12], A [K][6][N]) of the host build; roots [A][13] (one root for all envs) or [K][A][13]"""
    K, n = len(dof), dof.shape[1] // 2
    roots = np.asarray(roots, np.float32)
    roots = np.ascontiguousarray(np.tile(roots, (K, 1, 1)) if roots.ndim == 2 else roots)
    q, qd = np.ascontiguousarray(dof[:, 0::2], np.float32), np.ascontiguousarray(dof[:, 1::2], np.float32)
    moving = cc.is_moving(model)
    rows = np.full((K, 12), np.nan, np.float32)
    A = np.full((K, 6, n + (6 if moving else 0)), np.nan, np.float32)
    assert lib.emu_momentum(C.byref(model), K, fp(roots), fp(q), fp(qd), fp(rows)) == 0
    assert lib.emu_centroidal_matrix(C.byref(model), int(moving), K, fp(roots), fp(q), fp(A)) == 0
    assert np.isfinite(rows).all() and np.isfinite(A).all()
    return rows, A


# ---- 3. the tolerances --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=CASE_IDS)
def test_device_functions_on_the_host_meet_the_tolerances(case, hostemu):
    r = _references(case)
    dof, roots = _inputs(case)
    tol = cc.tolerances(robot_of(case))
    rows, A = host(hostemu, r.model, roots, dof)
    e = cc.errors(cc.split(rows, A), r.ref, r.D)
    print("\n" + cc.report(f"{CASE_IDS[ALL_CASES.index(case)]}, host build: error (tolerance)", e, tol))
    assert cc.within(e, tol), {k: (v, tol[k]) for k, v in e.items() if v > tol[k]}
    if cc.is_moving(r.model):
        assert not A[:, 3:6, 0:3].any()                             # written as exact zeros


@pytest.mark.parametrize("case", [("franka_panda", "tilted"), ("omnipanda", "origin")], ids=["franka_panda-tilted", "omnipanda-origin"])
def test_without_gravity_the_potential_energy_is_exact_zeros(case, hostemu):
    scene = cc.fixed_scene(*case, gravity=False)
    dof, root = cc.fixed_inputs(*case)
    r = cc.references_at(scene, scene.to_c(), root, dof[:16], with_A=False)
    rows, _ = host(hostemu, r.model, root, dof[:16])
    assert not r.rows[:, 11].any() and not bits(rows[:, 11]).any()  # +0.0
    e = cc.errors(cc.split(rows, None), r.ref, r.D)
    assert e["V"] == 0.0 and cc.within(e, cc.tolerances(case[0]))


# ---- 4. what the results must not notice --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", cc.MOVING_ROBOTS)
def test_a_far_base_moves_the_centre_of_mass_and_nothing_else(robot, hostemu):
    r = cc.moving_references(robot)
    dof, roots = (a[:16] for a in cc.moving_inputs(robot))
    a = int(r.model.robot_actor)
    near, A_near = host(hostemu, r.model, roots, dof)
    far = np.array(roots)
    far[:, a, 0:3] += np.asarray(cc.FAR_SHIFT, np.float32)
    rows, A = host(hostemu, r.model, far, dof)
    keep = [0] + list(range(4, 11))
    assert np.array_equal(bits(rows[:, keep]), bits(near[:, keep])) and np.array_equal(bits(A), bits(A_near))      # m, p, L, T and A: bit for bit
    moved = rows[:, 1:4].astype(np.float64) - near[:, 1:4] - (far[:, a, 0:3].astype(np.float64) - roots[:, a, 0:3])
    ulp = np.spacing(np.maximum(np.abs(rows[:, 1:4]), np.abs(near[:, 1:4])).astype(np.float32)).astype(np.float64)
    print(f"\n[{robot}] c moved by the shift to within {np.abs(moved / ulp).max():.2f} ulp of the shifted coordinate")
    assert (np.abs(moved) <= ulp).all() and np.abs(rows[:, 1]).min() > 400.0


# ---- 5. a Panda with a moving base --------------------------------------------------------------------------------------------------
def test_floating_panda_at_rest_carries_the_fixed_panda(hostemu):
    fixed_scene = jc.scene_of("franka_panda")
    scene = build_scene(["panda"], [[0.0, 0.0, 0.0]], robot_overrides={"fixed": False})
    fixed_scene.robot.gravity = scene.robot.gravity = True
    model, fixed_model = scene.to_c(), fixed_scene.to_c()
    K = 12
    dof = np.ascontiguousarray(cc.fixed_inputs("franka_panda")[0][:K])
    _, root = scene.initial_state()
    _, fixed_root = fixed_scene.initial_state()
    assert not np.asarray(root)[:, 7:13].any() and np.array_equal(np.asarray(root), np.asarray(fixed_root))       # the base at rest, where the fixed one stands
    fl, A_fl = host(hostemu, model, root, dof)
    fx, A_fx = host(hostemu, fixed_model, fixed_root, dof)
    assert np.array_equal(bits(fl[:, 10]), bits(fx[:, 10])) and np.array_equal(bits(fl[:, 4:7]), bits(fx[:, 4:7]))   # T and p: the base adds zeros
    assert np.array_equal(bits(A_fl[:, 0:3, 6:]), bits(A_fx[:, 0:3]))                                                 # the joints' linear columns
    # the base's own body, in fp64: (m_b, c_b) of a base at rest with the root row's pose
    mb = float(model.base_mass)
    R = fc.quat_R(np.asarray(root, np.float64)[int(model.robot_actor), 3:7], np.float64)
    cb = np.asarray(root, np.float64)[int(model.robot_actor), 0:3] + R @ np.array(list(model.base_h)) / mb
    m, c, p, L, V = (fx[:, s].astype(np.float64) for s in (slice(0, 1), slice(1, 4), slice(4, 7), slice(7, 10), 11))
    g = np.array([model.gravity[j] for j in range(3)])
    c_want = (m * c + mb * cb) / (m + mb)
    L_want = L - np.cross(c_want - c, p)
    V_want = V - mb * (g @ cb)
    tol, D = cc.tolerances("franka_panda"), cc.fixed_references("franka_panda").D
    e = {"m": np.abs(fl[:, 0:1] - (m + mb)).max() / (D["m"] + mb), "c": np.abs(fl[:, 1:4] - c_want).max(), "L": np.abs(fl[:, 7:10] - L_want).max() / D["L"],
         "V": np.abs(fl[:, 11] - V_want).max() / D["V"]}
    print("\n" + cc.report("floating Panda at rest against the fixed Panda plus the base's own body", e, tol))
    assert mb > 0.5 and np.abs(c_want - c).max() > 1e-2 and cc.within(e, tol)


# ---- 6. refusals of the host build --------------------------------------------------------------------------------------------------
def test_host_build_refuses_what_the_library_refuses(hostemu):
    out = np.zeros(4096, np.float32)
    K = 2
    r = cc.moving_references("boxer")
    dof, roots = cc.moving_inputs("boxer")
    q, qd, roots32 = (np.ascontiguousarray(x) for x in (dof[:K, 0::2], dof[:K, 1::2], roots[:K]))
    mom = lambda model, roots, q, o: hostemu.emu_momentum(C.byref(model), K, fp(roots), fp(q), fp(q), fp(o))
    mat = lambda model, moving, roots, q, o: hostemu.emu_centroidal_matrix(C.byref(model), moving, K, fp(roots), fp(q), fp(o))
    # the wrong kind of base for a matrix entry; the momentum row serves both
    p = cc.fixed_references("franka_panda")
    pq = np.ascontiguousarray(cc.fixed_inputs("franka_panda")[0][:K, 0::2])
    proots = np.ascontiguousarray(np.tile(np.asarray(cc.fixed_inputs("franka_panda")[1], np.float32), (K, 1, 1)))
    assert mat(p.model, 1, proots, pq, out) == -2 and mat(r.model, 0, roots32, q, out) == -2
    # a forest of two moving bases: all three
    two = build_scene(["jackal_a", "jackal_b"], [[0.0, 0.0, 0.1], [1.5, 0.0, 0.1]])
    tm = two.to_c()
    assert int(tm.n_extra_bases) == 1
    troots = np.ascontiguousarray(np.tile(np.asarray(two.initial_state()[1], np.float32), (K, 1, 1)))
    tq = np.zeros((K, two.n_dof), np.float32)
    assert mom(tm, troots, tq, out) == -7 and mat(tm, 0, troots, tq, out) == -7 and mat(tm, 1, troots, tq, out) == -7
    # a null output
    assert mom(r.model, roots32, q, None) == -5 and mat(r.model, 1, roots32, q, None) == -5 and mat(p.model, 0, proots, pq, None) == -5
    assert not out.any()                                            # nothing was written
    # a fixed-base forest is served
    actors, init = jc.two_point_robot_actors()
    forest = build_scene(list(actors), init)
    froots = np.ascontiguousarray(np.tile(np.asarray(forest.initial_state()[1], np.float32), (K, 1, 1)))
    fq = np.ones((K, forest.n_dof), np.float32)
    assert mom(forest.to_c(), froots, fq, out) == 0 and out[:K * 12:12].all() and not out[K * 12:].any()
    n = q.shape[1]
    out[:] = 0.0
    assert mat(r.model, 1, roots32, q, out) == 0 and out[:K * 6 * (6 + n)].any() and not out[K * 6 * (6 + n):].any()


# ---- 7. the wrapper's refusals, through a stub --------------------------------------------------------------------------------------
def test_wrapper_refuses_a_horizon_view_and_the_wrong_base():
    from mppiisaac.planner.isaacgym_wrapper import IsaacGymWrapper, PerStepOnly
    texts = {"fixed": b"mppi_sim_centroidal_matrix: this robot has a moving base (the six base columns are not computed); use mppi_sim_floating_centroidal_matrix",
             "floating": b"mppi_sim_floating_centroidal_matrix: this robot has a fixed base (there are no base columns); use mppi_sim_centroidal_matrix",
             "momentum": b"mppi_sim_momentum: unsupported for a forest of several moving bases"}
    calls, last = [], []

    def entry(name):
        def call(ctx, out):
            calls.append(name)
            last[:] = [name]
            return capi.MPPI_EUNSUPPORTED
        return call
    own = {}
    sim = object.__new__(IsaacGymWrapper)
    sim._state_t = sim._state_t_own = own
    sim.num_envs, sim.device, sim._ctx = 4, "cpu", None
    sim._momentum = sim._centroidal_matrix = sim._floating_centroidal_matrix = None
    sim.scene = SimpleNamespace(n_dof=7, actor_index=lambda name: 0, robot=SimpleNamespace(name="panda"))
    sim._c_model = SimpleNamespace(robot_actor=0, actors=[SimpleNamespace(fixed=1)])
    sim._lib = SimpleNamespace(mppi_sim_momentum=entry("momentum"), mppi_sim_centroidal_matrix=entry("fixed"),
                               mppi_sim_floating_centroidal_matrix=entry("floating"), mppi_last_error=lambda: texts[last[0]])
    sim._reset_envs_if_needed = lambda: None
    t = sim.acquire_momentum_tensor("panda")
    A, Af = sim.acquire_centroidal_matrix_tensor("panda"), sim.acquire_floating_centroidal_matrix_tensor("panda")
    assert tuple(t.shape) == (4, 12) and tuple(A.shape) == (4, 6, 7) and tuple(Af.shape) == (4, 6, 13)
    assert not t.any() and not A.any() and not Af.any() and sim.acquire_momentum_tensor("panda") is t and sim.acquire_centroidal_matrix_tensor("panda") is A
    with pytest.raises(NotImplementedError, match="fixed base .* use mppi_sim_centroidal_matrix"):
        sim.refresh_floating_centroidal_matrix_tensors()
    with pytest.raises(NotImplementedError, match="moving base .* use mppi_sim_floating_centroidal_matrix"):
        sim.refresh_centroidal_matrix_tensors()
    with pytest.raises(NotImplementedError, match="moving base .* use mppi_sim_floating_centroidal_matrix"):
        sim.com_jacobian("panda")                                   # (a fixed robot actor: the fixed entry is the one asked)
    for call in (sim.refresh_momentum_tensors, sim.centre_of_mass, sim.robot_momentum, sim.kinetic_energy, sim.potential_energy):
        with pytest.raises(NotImplementedError, match="several moving bases"):
            call()
    assert calls == ["floating", "fixed", "fixed"] + ["momentum"] * 5 and not t.any()
    sim._state_t = {}                                               # a horizon view: other tensors than the simulator's own
    for call in (lambda: sim.acquire_momentum_tensor("panda"), sim.refresh_momentum_tensors, sim.centre_of_mass, sim.robot_momentum, sim.kinetic_energy,
                 sim.potential_energy, lambda: sim.acquire_centroidal_matrix_tensor("panda"), lambda: sim.acquire_floating_centroidal_matrix_tensor("panda"),
                 sim.refresh_centroidal_matrix_tensors, sim.refresh_floating_centroidal_matrix_tensors, lambda: sim.com_jacobian("panda")):
        with pytest.raises(RuntimeError, match="per-step only") as e:
            call()
        assert isinstance(e.value, PerStepOnly) and "centre of mass, momentum and energy" in str(e.value)
    assert len(calls) == 8
