"""The cost-program interpreter of every kernel that runs it, pinned to the fp64 oracle TERM BY TERM on a real MI355X: the table of
single-term programs of tests/cost_term_cases.py (its docstring derives the tolerances; tests/test_cost_term_cases.py shows on the
oracle that a pass means something) by three routes:

 A  mppi_eval_cost (k_eval_cost + GivenEnv) on 130 designed envs per row at the edges of each measurement;
 B  S[k] of mppi_rollout of every rollout kernel against oracle64.rollout under the same program, every sample (StaticEnv on the
    contact-free arm; SceneEnv on the floating base, in contact, with a held block, on the second of two moving bases);
 C  the octet kernels against the fp64 costs of their OWN dumped trajectory (mppi_rollout_trajectory), so that the costs - the
    contact forces at contact included - are checked without the dynamics in between.

One context per (scene, kernel), mppi_set_cost per row; every test prints one line per row with its worst deviation and its tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import cost_term_cases as T
from mppiisaac.backend import capi
from test_cost_term_cases import check_a
from test_gpu_rollout_matrix import environment

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    return capi.load_library()


class Ctx:
    def __init__(self, lib, m, cfg, kernel=T.AUTO):
        self.lib, self.ctx = lib, C.c_void_p()
        with environment(MPPI_ROLLOUT=kernel or None):
            capi.check(lib, lib.mppi_create(C.byref(m), C.byref(cfg), 0, C.byref(self.ctx)))

    def call(self, name, *args):
        capi.check(self.lib, getattr(self.lib, name)(self.ctx, *args))

    def get(self, name, shape):
        out = np.zeros(shape, np.float32)
        self.call(name, capi.fptr(out))
        return out

    def info(self):
        buf = C.create_string_buffer(512)
        self.call("mppi_kernel_info", buf, 512)
        return buf.value.decode() + " "

    def close(self):
        self.lib.mppi_destroy(self.ctx)


# ---- route A -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["push", "anymal"])
def test_route_a_eval_cost_at_the_edges_of_each_measurement(which, lib, oracle64):
    _, m, cfg = T.context_a(which)
    rows = [r for r in T.rows_a() if r.ctx == which]
    c = Ctx(lib, m, cfg)
    fails, got, worst_of = [], {}, {}
    for r in rows:
        cost = r.cost
        c.call("mppi_set_cost", C.byref(cost))
        out = np.full(T.N_ENVS + 2, -7.0, np.float32)           # two guard values behind the last env
        c.call("mppi_eval_cost", T.N_ENVS, capi.fptr(r.dof), capi.fptr(r.root), capi.fptr(r.rb), capi.fptr(r.cf), capi.fptr(out))
        assert (out[T.N_ENVS:] == -7.0).all(), r.name
        got[r.name] = out[:T.N_ENVS]
        worst, f = check_a(r, got[r.name], T.reference_a(oracle64, r))
        worst_of[r.klass] = max(worst_of.get(r.klass, 0.0), worst)
        print(f"A {which} {r.name}: worst {worst:.2e} (rtol = atol = {T.tol_a(r.klass):.0e})")
        fails += f
    c.close()
    for klass, w in worst_of.items():
        print(f"A {which} class {klass}: worst {w:.2e}, tolerance {T.tol_a(klass):.0e}")
    for r in rows:              # a box actor's body spelled RB is the row spelled ACTOR (pack_cost)
        if r.bit_equal_to and not np.array_equal(got[r.name], got[r.bit_equal_to], equal_nan=True):
            fails.append(f"{r.name}: not bit-equal to {r.bit_equal_to}")
    assert not fails, "\n".join(fails)


# ---- routes B and C: one run per (scene, kernel), shared ---------------------------------------------------------------------------
_RUNS = {}


def run(lib, name, kernel):
    """every row of the scene on one context of the kernel -> {"S": {row: S [K]}, "dump": {U key: (states, du)}} or a refusal"""
    if (name, kernel) in _RUNS:
        return _RUNS[name, kernel]
    s = T.scene_b(name)
    try:
        c = Ctx(lib, s.m, s.cfg, kernel)
    except capi.MppiHipError as e:
        # the one-lane kernels keep 64 samples' rows in LDS per wavefront: a scene that needs more than 160 KiB for them is refused
        assert kernel in s.may_refuse and "libmppi_hip error -3" in str(e) and "160 KiB" in str(e), (name, kernel, e)
        _RUNS[name, kernel] = {"refused": str(e)}
        return _RUNS[name, kernel]
    eps = torch.tensor(s.eps, dtype=torch.float32, device="cuda").contiguous()
    c.call("mppi_set_noise_dev", C.c_void_p(eps.data_ptr()))
    c.call("mppi_set_state", capi.fptr(s.dof), capi.fptr(s.root))
    out = {"S": {}, "dump": {}, "info": None}
    for row in s.rows:
        cost, U = row.cost, s.nominal_of(row)
        c.call("mppi_set_cost", C.byref(cost))
        c.call("mppi_set_nominal", capi.fptr(U))
        c.call("mppi_rollout")
        out["S"][row.name] = c.get("mppi_get_costs", (s.K,))
        out["info"] = out["info"] or c.info()
    if kernel in s.trajectory:
        m, K = s.m, s.K
        f32 = dict(dtype=torch.float32, device="cuda")
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for U in {s.nominal_of(row).tobytes(): s.nominal_of(row) for row in s.rows}.values():
            X = {"dof": torch.zeros((T.H * K, 2 * m.n_bodies), **f32), "root": torch.zeros((T.H * K, m.n_actors, 13), **f32),
                 "rb": torch.zeros((T.H * K, m.n_rb, 13), **f32), "cf": torch.zeros((T.H * K, m.n_rb, 3), **f32)}
            c.call("mppi_set_nominal", capi.fptr(U))
            c.call("mppi_rollout_trajectory")
            c.call("mppi_materialise_trajectory", ptr(X["dof"]), ptr(X["root"]), ptr(X["rb"]), ptr(X["cf"]))
            du = c.get("mppi_get_perturbations", (T.H, s.cfg.nu, K))
            states = {k: v.cpu().numpy().astype(np.float64).reshape((T.H, K) + tuple(v.shape[1:])) for k, v in X.items()}
            states["ctrl"] = T.control_cost(s, U, du)            # the step matrix's block C: lambda sum_t U^T Sigma^-1 du, fp64
            out["dump"][U.tobytes()] = states
    c.close()
    _RUNS[name, kernel] = out
    return out


CASES_B = [(name, kernel) for name in T.SCENES_B for kernel in T.KERNELS_B[name]]
CASES_C = [(name, kernel) for name in T.SCENES_B for kernel in T.TRAJECTORY_B[name]]
ident = lambda c: f"{c[0]}-{c[1] or 'default'}"


@pytest.mark.parametrize("case", CASES_B, ids=ident)
def test_route_b_rollout_costs_match_the_oracle_per_sample(case, lib):
    name, kernel = case
    s, refs = T.scene_b(name), T.references_b(name)
    out = run(lib, name, kernel)
    if "refused" in out:
        print(f"B {ident(case)}: mppi_create refuses the one-lane kernels of this scene ({out['refused']})")
        return
    assert f"rollout={s.kernels[kernel]} " in out["info"], (kernel, out["info"])
    fails = []
    for row in s.rows:
        S, ref = out["S"][row.name], refs[row.name]
        worst = np.abs(S.astype(np.float64) - ref.S).max() if np.isfinite(S).all() else np.inf
        print(f"B {ident(case)} {row.name}: worst {worst:.2e} = {worst / np.abs(ref.S).max() if np.abs(ref.S).max() else 0:.1e} of max |S| "
              f"(tolerance {ref.tol:.2e} = {ref.rel:.0e} of max |S|)")
        if not worst <= ref.tol:
            fails.append(f"{row.name}: off by {worst:.3e} > {ref.tol:.2e} in sample {int(np.argmax(np.abs(S - ref.S)))}")
        if row.exact_zero and not np.abs(s.nominal_of(row)).max() and np.any(S != 0.0):
            fails.append(f"{row.name}: not exactly 0 in sample {int(np.flatnonzero(S != 0.0)[0])}")
        if row.bit_equal_to and not np.array_equal(S, out["S"][row.bit_equal_to], equal_nan=True):
            fails.append(f"{row.name}: not bit-equal to {row.bit_equal_to}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case", CASES_C, ids=ident)
def test_route_c_octet_costs_match_fp64_costs_of_their_own_trajectory(case, lib, oracle64, oracle32):
    name, kernel = case
    s = T.scene_b(name)
    out = run(lib, name, kernel)
    assert f"rollout={s.kernels[kernel]} " in out["info"], (kernel, out["info"])
    fails = []
    for row in s.rows:
        states = out["dump"][s.nominal_of(row).tobytes()]
        S = out["S"][row.name].astype(np.float64)
        S64, S32 = T.rollout_costs_on(oracle64, s.m, row.cost, states), T.rollout_costs_on(oracle32, s.m, row.cost, states)
        tol = T.tolerance_c(S32, S64)
        err = np.abs(S - S64)
        k = int(np.argmax(err - tol)) if np.isfinite(S).all() else 0
        print(f"C {ident(case)} {row.name}: S in [{S64.min():.4g}, {S64.max():.4g}], worst {err.max():.2e}, "
              f"tolerance {tol.min():.2e} .. {tol.max():.2e} (10 x the oracle builds' {np.abs(S32 - S64).max():.2e}, floor 2e-6 (1 + |S|))")
        if not (np.isfinite(S).all() and (err <= tol).all()):
            fails.append(f"{row.name}: off by {err[k]:.3e} > {tol[k]:.2e} in sample {k}")
    assert not fails, "\n".join(fails)
