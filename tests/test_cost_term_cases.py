"""The conditions on the table of single-term cost programs (tests/cost_term_cases.py), on the oracle and on the host build alone:
a pass of tests/test_gpu_cost_terms.py means something only if the references are finite and away from the reference's own
discontinuities, every named edge is reached, the samples of a rollout row are spread by more than 100 x its tolerance and every
plausible plumbing error (a neighbouring index, one component more or less, an unshifted constant, the other robot's row, a
transposed rotation, no discount) moves a sample by more than 100 x its tolerance.  The same rows go through the device arithmetic
compiled for the host (tests/hostemu) at the tolerances of the GPU test, so the table can be debugged without a GPU."""
import ctypes as C

import numpy as np
import pytest

import cost_term_cases as T
from mppiisaac.backend import capi
from test_hostemu_parity import emu_rollout, fp

ROWS_A = T.rows_a()
# the edges the measurements are delicate at: each is reached by at least 8 envs of its class
EDGES = {"DIST": ("z-difference", "coincident", "one-ulp-apart", "400-m-out"), "TILT": ("gimbal", "atan2-cut", "norm-0.5", "norm-2", "negated"),
         "YAW_ABS": ("near-pi", "at-p3", "1e-5-off-p3", "tilted"),
         "ALIGN": ("parallel", "perpendicular", "antiparallel", "1e-3-off-antiparallel", "1e-6-m-ray", "z-difference", "zero-ray"),
         "FORCE_L1": ("negative-components", "zero-force", "neighbours-a-decade-apart"), "SPEED": ("zero-velocity", "one-component"),
         "DOF_SQ": ("on-the-references",), "ABS_DZ": ("above", "below", "equal", "one-ulp-above", "one-ulp-below"),
         "BELOW": ("above", "below", "equal", "one-ulp-above", "one-ulp-below")}


@pytest.fixture(scope="module")
def refs_a(oracle64, oracle32):
    return {r.name: (T.reference_a(oracle64, r), T.reference_a(oracle32, r)) for r in ROWS_A}


def ill_posed(row, ref32, ref64):
    """envs whose input sits on a discontinuity of the reference: its two builds part by more than 1e-3, or - TILT - both arguments
    of its atan2 vanish (on the fp32-rounded gimbal quaternion both builds take atan2(0, +-0) the same way, 0 or pi by the sign of a
    zero, and a last-bit difference in either argument decides between them)"""
    bad = np.isfinite(ref64) & ~(np.abs(ref32 - ref64) <= 1e-3)
    for t in row.terms:
        if t["op"] == capi.OP_TILT:
            r, i, j, k = (row.rb[:, t["idx"][0], 3 + c].astype(np.float64) for c in range(4))
            two_s = 2.0 / (r * r + i * i + j * j + k * k)
            bad |= np.maximum(np.abs(1.0 - two_s * (j * j + k * k)), np.abs(two_s * (i * j + k * r))) < 1e-6
    return np.flatnonzero(bad)


def test_route_a_references_are_finite_and_away_from_the_reference_s_jumps(refs_a, oracle64, oracle32):
    for r in ROWS_A:
        a, b = refs_a[r.name]
        want = np.zeros(T.N_ENVS, bool)
        if r.nonfinite is not None:
            want[r.nonfinite] = True
        np.testing.assert_array_equal(~np.isfinite(a), want, err_msg=r.name)       # not finite exactly in the designed envs
        np.testing.assert_array_equal(~np.isfinite(b), want, err_msg=r.name)
        assert ill_posed(r, b, a).size == 0, (r.name, ill_posed(r, b, a))
        assert r.dof.dtype == r.root.dtype == r.rb.dtype == r.cf.dtype == np.float32
        if len(r.terms) == 1:
            assert r.terms[0]["w"] in (1.0, -2.5)
    # the criterion rejects the row this table must not hold: TILT exactly on the gimbal (atan2(+-0, +-0) jumps by pi)
    tilt = next(r for r in ROWS_A if r.klass == "TILT")
    import copy
    on = copy.deepcopy(tilt)
    h = np.float32(np.sqrt(0.5))
    on.rb[:, on.terms[0]["idx"][0], 3:7] = [0.0, h, 0.0, h]
    a, b = T.reference_a(oracle64, on), T.reference_a(oracle32, on)
    assert ill_posed(on, b, a).size == T.N_ENVS, (a[0], b[0])


def test_route_a_every_edge_is_reached_by_eight_envs():
    for klass, names in EDGES.items():
        for edge in names:
            n = sum(len(np.unique(r.edges.get(edge, ()))) for r in ROWS_A if r.klass == klass)
            assert n >= 8, (klass, edge, n)
    assert {r.klass for r in ROWS_A} == set(T.ORACLE32_A)
    assert any(len(r.terms) == capi.MAX_TERMS for r in ROWS_A)
    # each source kind as operand 0 and as operand 1 of a DIST row; the same box body spelled RB and ACTOR
    kinds = {(a, t["src"][a]) for r in ROWS_A if r.klass == "DIST" for t in r.terms for a in (0, 1)}
    assert kinds == {(a, s) for a in (0, 1) for s in (T.RB, T.ACTOR, T.DOF_XY, T.CONST)}
    pair = [r for r in ROWS_A if r.bit_equal_to]
    assert len(pair) == 1
    twin = next(r for r in ROWS_A if r.name == pair[0].bit_equal_to)
    for k in ("dof", "root", "rb", "cf"):
        np.testing.assert_array_equal(getattr(pair[0], k), getattr(twin, k))
    # DOF_SQ: ranges longer than the eight reference values, with 0, 1 and 8 of them; the empty range
    dofsq = [r.terms[0] for r in ROWS_A if r.klass == "DOF_SQ"]
    assert {t["idx"][2] for t in dofsq if t["idx"][1] - t["idx"][0] > 8} == {0, 1, 8}
    assert any(t["idx"][0] == t["idx"][1] for t in dofsq) and {t["n"] for t in dofsq} == {0, 1}
    assert any(float(np.float32(p)) != float(p) for t in dofsq for p in t["p"])


def test_route_a_constants_are_current(refs_a):
    measured = {}
    for r in ROWS_A:
        a, b = refs_a[r.name]
        measured[r.klass] = max(measured.get(r.klass, 0.0), T.deviation_a(b, a).max())
    for klass, v in measured.items():
        print(f"route A {klass}: fp32 oracle within {v:.2e} (committed {T.ORACLE32_A[klass]:.2e}) -> rtol = atol = {T.tol_a(klass):.0e}")
    for klass, v in measured.items():
        c = T.ORACLE32_A[klass]
        assert 0.5 * c <= v <= 2.0 * c, (klass, v, c)


def eval_cost_on_host(hostemu, row):
    _, m, _ = T.context_a(row.ctx)
    out = np.full(T.N_ENVS, -1.0, np.float32)
    cost = row.cost
    with np.errstate(all="ignore"):
        assert hostemu.emu_eval_cost(C.byref(m), C.byref(cost), T.N_ENVS, fp(row.dof), fp(row.root), fp(row.rb), fp(row.cf), fp(out)) == 0
    return out


def check_a(row, got, ref):
    """-> (worst deviation in units of the tolerance's rtol = atol form, failures)"""
    tol, fails = T.tol_a(row.klass), []
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin):
        fails.append(f"{row.name}: non-finite in envs {np.flatnonzero(np.isfinite(got) != fin)}")
    err = np.abs(got[fin].astype(np.float64) - ref[fin]) / (1.0 + np.abs(ref[fin]))
    worst = np.nanmax(np.where(np.isfinite(err), err, np.inf))
    if not worst <= tol:
        fails.append(f"{row.name}: off by {worst:.3e} > {tol:.0e} in env {np.flatnonzero(fin)[np.argmax(err)]}")
    return worst, fails


def test_route_a_rows_through_the_host_build(hostemu, refs_a):
    fails, got = [], {}
    for r in ROWS_A:
        got[r.name] = eval_cost_on_host(hostemu, r)
        worst, f = check_a(r, got[r.name], refs_a[r.name][0])
        print(f"host A {r.name}: worst {worst:.2e} (tol {T.tol_a(r.klass):.0e})")
        fails += f
    for r in ROWS_A:
        if r.bit_equal_to:
            np.testing.assert_array_equal(got[r.name], got[r.bit_equal_to])
    assert not fails, "\n".join(fails)


# ---- route B -----------------------------------------------------------------------------------------------------------------------
def welded_alike(s, rb_a, rb_b):
    """two robot links on the same body with the same fixed rotation: TILT cannot tell them apart, DIST can"""
    la, lb = (s.m.links[i - s.scene.first_rb[s.m.robot_actor]] for i in (rb_a, rb_b))
    return la.body == lb.body and np.allclose(list(la.R), list(lb.R), atol=1e-12)


@pytest.mark.parametrize("name", T.SCENES_B)
def test_route_b_rows_are_spread_and_tell_the_mix_ups_apart(name, oracle64):
    s, refs = T.scene_b(name), T.references_b(name)
    assert len({r.name for r in s.rows}) == len(s.rows) and sum(r.nominal for r in s.rows) == (0 if name == "contact" else 1)
    assert s.cfg.rollout_var_discount == T.GAMMA and s.cfg.horizon == T.H and not s.cfg.noise_abs_cost and s.K <= 130
    assert np.abs(s.U0).min() > 0 or name == "contact"
    fails = []
    for row in s.rows:
        ref = refs[row.name]
        assert np.isfinite(ref.S).all() and np.isfinite(ref.S32).all(), row.name
        np.testing.assert_allclose(ref.S_states, ref.S, rtol=1e-12, atol=1e-12)     # the states route C's reference formula is fed here are the oracle's
        T_ = T.trajectory_of(oracle64, s, s.nominal_of(row))
        tol = ref.tol if s.separate == "B" else ref.tol_c.max()
        spread = ref.S.max() - ref.S.min()
        print(f"{name} {row.name}: S in [{ref.S.min():.4g}, {ref.S.max():.4g}], route B tolerance {ref.rel:.0e} of max |S| = {ref.tol:.2e}, "
              f"spread {spread:.2e} = {spread / tol if tol else np.inf:.0f} x the {'route B' if s.separate == 'B' else 'route C'} tolerance {tol:.2e}")
        if row.exact_zero:
            np.testing.assert_allclose(ref.S, T_["ctrl"], rtol=0, atol=1e-15)      # (S is the control cost alone)
        elif row.constant:
            assert spread <= ref.tol
        elif not spread >= 100.0 * tol:
            fails.append(f"{row.name}: spread {spread:.2e} < 100 x {tol:.2e}")
        listed = set(row.not_covered)
        assert len(listed) <= 1
        for mname, kind, tt, kw in T.mixups(s, row):
            if row.exact_zero and (kind != "index" or not oracle64.is_scene(s.m)):
                continue                      # a constant 0 has no components and no discount to tell apart; nothing touches anything without contact
            Sm = T.rollout_costs_on(oracle64, s.m, T.program(tt), T_, **kw)
            moved = np.nanmax(np.where(np.isfinite(Sm), np.abs(Sm - ref.S), np.inf))
            ok = moved > 100.0 * tol
            if mname in listed:
                assert not ok, (row.name, mname, "is listed as not covered but is")
                assert kind != "index" or welded_alike(s, row.t["idx"][0], tt["idx"][0]), (row.name, mname)
                print(f"    NOT COVERED by this row: {mname} moves a sample by {moved / tol:.0f} x the tolerance only")
            elif not ok:
                fails.append(f"{row.name}: mix-up {mname} moves a sample by {moved:.2e} = {moved / tol:.1f} x the tolerance only")
        assert listed <= {mx[0] for mx in T.mixups(s, row)}
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", T.SCENES_B)
def test_route_b_rows_through_the_host_build(name, hostemu):
    s, refs = T.scene_b(name), T.references_b(name)
    fails, got = [], {}
    for row in s.rows:
        ref = refs[row.name]
        S, _, _ = emu_rollout(hostemu, s.m, s.cfg, row.cost, s.dof, s.root, s.nominal_of(row), s.eps)
        got[row.name] = S
        worst = np.abs(S.astype(np.float64) - ref.S).max() if np.isfinite(S).all() else np.inf
        print(f"host B {name} {row.name}: worst {worst:.2e} (tol {ref.tol:.2e} = {ref.rel:.0e} of max |S|)")
        if not worst <= ref.tol:
            fails.append(f"{row.name}: off by {worst:.3e} > {ref.tol:.2e}")
    for row in s.rows:
        if row.bit_equal_to:
            np.testing.assert_array_equal(got[row.name], got[row.bit_equal_to], err_msg=row.name)
        if row.exact_zero and not np.abs(s.nominal_of(row)).max():
            np.testing.assert_array_equal(got[row.name], 0.0, err_msg=row.name)
    assert not fails, "\n".join(fails)
