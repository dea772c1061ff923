"""Well-posedness of the weighting matrix (tests/weighting_cases.py), on the reference alone - no GPU: a pass of
tests/test_gpu_weighting_matrix.py has to mean something.

  * the tolerances in the tables ARE ten times the deviation of the sequential fp32 restatement from the fp64 reference, rounded up to
    1-2-5, and stay under the caps;
  * every row that is not deliberately degenerate has an effective record (sample) count of at least four;
  * leaving out any record (sample) a row names as a boundary moves a compared output by at least ten times the row's tolerance;
  * counting the eta = 0 records of rows (e), (f) as live moves an output by at least ten times the tolerance;
  * the nominal is non-zero, the filter rows differ from the unfiltered update;
  * every branch threshold of combine_update is named by a row on each side (or shown to have one reachable side)."""
import collections

import numpy as np
import pytest

import weighting_cases as wc


@pytest.fixture(scope="module")
def shapes():
    cache = {}

    def get(HN, **over):
        key = (HN, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = wc.make_shape(HN, **over)
        return cache[key]
    return get


def run_row(row, shape):
    """per update of the row: (records, twin, lambda, U0, F, fp64 result, fp32 result)"""
    F = wc.savgol_matrix(shape.cfg.horizon).astype(np.float32) if row.filt else None
    U0, outs = wc.nominal(shape), []
    for lam in wc.row_lambda(row, shape):
        recs, twin = wc.make_records(row, shape, lam)
        r64 = wc.update64(recs, U0, lam, row.u_init, F)
        r32 = wc.update32(recs, U0, lam, row.u_init, F)
        outs.append((recs, twin, lam, U0, F, r64, r32))
        U0 = r64["U"].astype(np.float32)
    return outs


MEASURED = collections.defaultdict(lambda: {"eta": 0.0, "U": 0.0})


@pytest.mark.parametrize("row", wc.ROWS, ids=wc.ROW_IDS)
def test_route_a_rows_are_well_posed(row, shapes):
    assert wc.ROW_IDS.count(row.name) == 1
    shape = shapes(row.HN)
    assert np.abs(wc.nominal(shape)).min() > 0, "the nominal handed in is non-zero"
    tol = row.tol
    for recs, twin, lam, U0, F, r64, r32 in run_row(row, shape):
        assert recs.shape == (row.nrec, 2 + row.HN) and recs.dtype == np.float32
        dev = wc.deviation(r32, r64, shape.umax)
        key = row.cls[0] + ("-big" if row.big else "")
        for q in dev:
            MEASURED[key][q] = max(MEASURED[key][q], dev[q])
        print(f"{row.name} lambda {lam:g}: fp32 restatement off by eta {dev['eta']:.1e} (tol {tol['eta']:.0e}), U {dev['U']:.1e} (tol {tol['U']:.0e}); "
              f"effective records {wc.ess(r64['w']):.1f}")
        assert np.isfinite(r64["U"]).all() and np.isfinite(r64["action"]).all()
        if row.cls == "g":
            assert r64["eta"] == 0 and np.isposinf(r64["beta"])
            np.testing.assert_array_equal(r64["action"], U0[0])
            np.testing.assert_array_equal(r64["U"][:-1], U0[1:])
            np.testing.assert_array_equal(r64["U"][-1], np.float32(row.u_init))
            assert row.u_init != 0
            continue
        assert r32["beta"] == r64["beta"]
        for q in dev:
            assert 10 * dev[q] <= tol[q], f"{q}: the tolerance is less than ten times the fp32 deviation"
            assert tol[q] <= wc.CAP[q] * (1.0 if row.big else 0.1)
        if not row.degenerate:
            assert wc.ess(r64["w"]) >= 4
        live = recs[:, 1] > 0
        # the named boundary records carry weight: without any one of them an output moves
        for b in sorted({b % row.nrec for b in row.bounds}) if row.nrec > 1 else []:
            assert live[b]
            d = wc.deviation(wc.update64(np.delete(recs, b, axis=0), U0, lam, row.u_init, F), r64, shape.umax)
            assert d["U"] >= 10 * tol["U"] or d["eta"] >= 10 * tol["eta"], (b, d)
            assert d["U"] >= 10 * tol["U"], (b, d)
        if row.cls == "b":
            assert np.argmin(np.where(live, recs[:, 0], np.inf)) == row.min_at and (recs[:, 0] == recs[row.min_at, 0]).sum() == 1
        if row.cls in ("e", "f"):
            assert (~live).sum() >= row.nrec // 4 and twin[~live, 0].max() < recs[live, 0].min()
            assert np.isfinite(twin).all() and np.array_equal(twin[live], recs[live])
            if row.cls == "f":
                bad = recs[~live]
                assert np.isnan(bad[:, 2:]).any() and np.isposinf(bad[:, 2:]).any() and np.isneginf(bad[:, 2:]).any()
                kinds = int(np.isnan(bad[:, 0]).any()) + int(np.isposinf(bad[:, 0]).any()) + int(np.isneginf(bad[:, 0]).any())
                assert kinds == min(3, len(bad)), "NaN, +Inf and -Inf among the betas of the skipped records, as far as they reach"
                assert np.isfinite(recs[live]).all()
            as_live = twin.copy()
            as_live[~live, 1] = 1.0
            d = wc.deviation(wc.update64(as_live, U0, lam, row.u_init, F), r64, shape.umax)
            assert d["U"] >= 10 * tol["U"] and d["eta"] >= 10 * tol["eta"]
        if row.cls == "c":
            with np.errstate(under="ignore"):
                sc = np.exp(-(recs[:, 0].astype(np.float64) - r64["beta"]) / lam).astype(np.float32)
            tiny = np.finfo(np.float32).tiny
            assert (sc == 0).mean() > 0.3 and ((sc > 0) & (sc < tiny)).any(), "most factors underflow, some are denormal"
        if row.filt:
            d = wc.deviation(wc.update64(recs, U0, lam, row.u_init, None), r64, shape.umax)
            assert d["U"] >= 10 * tol["U"], "the filter changes the update"
        if row.u_init:
            assert abs(row.u_init) >= 10 * tol["U"] * shape.umax.max()
    if row.lam_scale:
        assert len(row.lam_scale) == 2 and min(row.lam_scale) == 1e-2 and max(row.lam_scale) == 1e2


def test_route_a_tolerances_are_the_sized_ones(shapes):
    """TOL = round125(10 x the fp32 restatement's deviation), per class; the deviation in the table is the one measured here (exponentials of
    different libms differ in the last bit: half to five quarters of it, and never more than a tenth of the tolerance)"""
    for row in wc.ROWS:
        shape = shapes(row.HN)
        key = row.cls[0] + ("-big" if row.big else "")
        for recs, twin, lam, U0, F, r64, r32 in run_row(row, shape):
            dev = wc.deviation(r32, r64, shape.umax)
            for q in dev:
                MEASURED[key][q] = max(MEASURED[key][q], dev[q])
    for key in sorted(MEASURED):
        print(f"class {key}: measured eta {MEASURED[key]['eta']:.2e} U {MEASURED[key]['U']:.2e}; table {wc.TOL[key]}")
    assert sorted(MEASURED) == sorted(wc.TOL)
    for key, m in MEASURED.items():
        for q in ("eta", "U"):
            tol, stated = wc.TOL[key][q]
            if key.startswith("g"):
                assert tol == 0 and m[q] == 0
                continue
            assert tol == wc.round125(10 * stated), (key, q)
            assert stated / 2 <= m[q] <= stated * 1.25 and 10 * m[q] <= tol, (key, q, m[q], stated)


def test_every_branch_of_the_combine_is_named_on_both_sides():
    seen = collections.defaultdict(set)
    for row in wc.ROWS:
        p = wc.combine_path(row.HN, row.nrec, row.NT)
        for k, v in p.items():
            seen[(row.NT, k)].add(v)
        seen["filter"].add(row.filt)
        seen["nrec"].add(row.nrec)
    for NT in (wc.NT_UPDATE, wc.NT_WORLD):
        for k in ("wide", "second_pass", "recompute", "wide_tail"):
            assert seen[(NT, k)] == {False, True}, (NT, k)
        # Gw HN <= 4 NT <= 4096 < kPartFloats = 6144 for every HN <= MPPI_MAX_H MPPI_MAX_NU: the cap has ONE reachable side
        assert seen[(NT, "part_capped")] == {False}
        assert all(not wc.combine_path(HN, 1, NT)["part_capped"] for HN in range(1, 769))
    assert seen[(wc.NT_UPDATE, "nvalid")] == {1, 2, 3, 4}
    assert seen[(wc.NT_WORLD, "rows_beyond_block")] == {False, True}
    assert seen[(wc.NT_UPDATE, "rows_beyond_block")] == {False}     # (HN <= 768 < 1024)
    assert seen["filter"] == {False, True}
    assert {1, 2, 7, 8, 9, 1023, 1024, 1025, 4095, 4096, 4097, 5000} == seen["nrec"]
    assert {wc.combine_path(r.HN, r.nrec, r.NT)["G"] for r in wc.ROWS if not wc.combine_path(r.HN, r.nrec, r.NT)["wide"]} >= {1, 7, 8}


# ---- route B: the conditions on the injected costs ----------------------------------------------------------------------------------------
def b_deviations(K, kind):
    S, du = wc.make_costs(kind, K, wc.B_LAMBDA), wc.b_du(K)
    umax = np.full(wc.B_H * 3, 1.5)
    U0 = (0.25 * umax.reshape(wc.B_H, 3) * np.random.default_rng(3).normal(size=(wc.B_H, 3))).astype(np.float32)
    want = wc.record64(S, du, wc.B_LAMBDA)
    b32, e32, N32 = wc.record32(S, du, wc.B_LAMBDA)
    d = wc.record_deviation((b32, e32, N32), want)
    up64 = wc.finish64(U0, want[0], want[1], want[2], 0.0)
    up32 = wc.update32(np.concatenate([[b32, e32], N32])[None, :], U0, wc.B_LAMBDA)
    d["U"] = wc.deviation(up32, up64, umax)["U"]
    d["S"] = 0.0
    for gamma in (1.0, 0.9):
        c = wc.stage_costs(S, wc.B_H, gamma)
        fin = np.isfinite(S)
        ref = wc.horizon_sum64(c, gamma)
        np.testing.assert_array_equal(np.isfinite(ref), fin)
        np.testing.assert_allclose(ref[fin], S[fin], rtol=1e-6)
        d["S"] = max(d["S"], float(np.max(np.abs(wc.horizon_sum32(c, gamma)[fin] - ref[fin]) / np.abs(ref[fin]))))
    return S, du, U0, umax, want, up64, b32, d


@pytest.mark.parametrize("K", wc.B_K)
def test_route_b_costs_are_well_posed(K):
    tol = {q: wc.TOL_B[q][0] for q in wc.TOL_B}
    for kind in wc.B_COSTS:
        S, du, U0, umax, want, up64, b32, d = b_deviations(K, kind)
        n_eff = wc.ess(want[3])
        print(f"K={K} {kind}: fp32 restatement off by " + ", ".join(f"{q} {v:.1e} (tol {tol[q]:.0e})" for q, v in d.items()) + f"; effective samples {n_eff:.1f}")
        assert b32 == want[0] and np.isfinite(up64["U"]).all()
        for q, v in d.items():
            assert 10 * v <= tol[q], (kind, q)
        assert tol["U"] <= 0.1 * wc.CAP["U"] and tol["eta"] <= 0.1 * wc.CAP["eta"] and tol["N"] <= 0.1 * wc.CAP["U"]
        if K >= 15:                 # (fewer samples: deliberately degenerate - a group with one live sample)
            assert n_eff >= 4, kind
        if kind == "planted" and K >= 8:
            assert (~np.isfinite(S)).sum() >= 2 and np.isfinite(S).sum() >= 2
        if kind == "min-last":
            assert np.argmin(S) == K - 1
        if kind == "min-tail-first":
            assert np.argmin(S) == 16 * ((K - 1) // 16)
        if kind == "wide" and K >= 64:
            with np.errstate(under="ignore"):
                w32 = want[3].astype(np.float32)
            assert (w32 == 0).mean() > 0.1
        if kind == "equal":
            assert (want[3] == 1).all()
        # without any one of the boundary samples (first, first and last live one of the tail group) an output moves
        for k in wc.B_BOUNDS(K) if K > 1 and kind != "planted" else []:
            keep = np.arange(K) != k
            less = wc.record64(S[keep], du[:, keep], wc.B_LAMBDA)
            moved = wc.deviation(wc.finish64(U0, less[0], less[1], less[2], 0.0), up64, umax)
            assert moved["U"] >= 10 * tol["U"] or moved["eta"] >= 10 * tol["eta"], (kind, k, moved)


def test_route_b_tolerances_are_the_sized_ones():
    m = {q: 0.0 for q in wc.TOL_B}
    for K in wc.B_K:
        for kind in wc.B_COSTS:
            d = b_deviations(K, kind)[-1]
            m = {q: max(m[q], d[q]) for q in m}
    print("route B: measured", {q: f"{v:.2e}" for q, v in m.items()}, "table", wc.TOL_B)
    for q, (tol, stated) in wc.TOL_B.items():
        assert tol == wc.round125(10 * stated), q
        assert stated / 2 <= m[q] <= stated * 1.25 and 10 * m[q] <= tol, (q, m[q], stated)


# ---- route C: the fused kernels' records on the oracle's rollouts of the same scenes ---------------------------------------------------------
def c_case(oracle64, K, H):
    from scenes import point_reach
    scene, m, cfg, cost, dof, root = point_reach(K=K, H=H, lambda_=wc.C_LAMBDA)
    S, du, _ = oracle64.rollout(m, cfg, cost, dof, root, wc.c_nominal(cfg), oracle64.sample(cfg))
    return S.astype(np.float32), du.astype(np.float32).reshape(-1, K)


def c_deviation(S, du):
    want = wc.record64(S, du, wc.C_LAMBDA)
    return want, wc.record_deviation(wc.record32(S, du, wc.C_LAMBDA), want)


def test_route_c_cases_are_well_posed_and_their_tolerances_sized(oracle64):
    m = {"eta": 0.0, "N": 0.0}
    for K in wc.C_K:
        for H in wc.C_H:
            S, du = c_case(oracle64, K, H)
            groups = wc.fold_groups(K, 8 if ((K + 15) // 16) % 16 == 0 else 1) + [(0, K)]
            for a, b in groups:
                want, d = c_deviation(S[a:b], du[:, a:b])
                print(f"K={K} H={H} samples {a}..{b - 1}: fp32 restatement off by eta {d['eta']:.1e}, N {d['N']:.1e}; effective samples {wc.ess(want[3]):.1f}")
                assert wc.ess(want[3]) >= 4
                m = {q: max(m[q], d[q]) for q in m}
    big = {"eta": 0.0, "N": 0.0}
    for which, K in wc.C_FOLD_TABLE.items():
        S, du = c_case(oracle64, K, 2)
        nw = (K + 15) // 16
        groups = wc.fold_groups(K, 8 if which == "eight-groups" else 1)
        assert (nw % 16 == 0) == (which == "eight-groups") and all((b - a) // 16 > wc.FOLD_TABLE for a, b in groups)
        assert (K > 131072) == (which == "eight-groups")
        for a, b in groups:
            want, d = c_deviation(S[a:b], du[:, a:b])
            beyond = want[3][16 * wc.FOLD_TABLE:].sum() / want[1]
            print(f"{which} K={K} samples {a}..{b - 1}: fp32 restatement off by eta {d['eta']:.1e}, N {d['N']:.1e}; beyond the table {beyond:.1e} of the weight")
            assert wc.ess(want[3]) >= 4 and beyond >= 100 * wc.TOL_C_BIG["eta"][0]
            # the first record beyond kFoldTable: without it the group's record moves
            keep = np.ones(b - a, bool)
            keep[16 * wc.FOLD_TABLE:16 * wc.FOLD_TABLE + 16] = False
            less = wc.record64(S[a:b][keep], du[:, a:b][:, keep], wc.C_LAMBDA)
            assert abs(less[1] - want[1]) / want[1] >= 10 * wc.TOL_C_BIG["eta"][0]
            big = {q: max(big[q], d[q]) for q in big}
    print("route C: measured", m, "table", wc.TOL_C, "| beyond the fold table: measured", big, "table", wc.TOL_C_BIG)
    for table, meas, cap in ((wc.TOL_C, m, 0.1), (wc.TOL_C_BIG, big, 1.0)):
        for q, (tol, stated) in table.items():
            assert tol == wc.round125(10 * stated), q
            assert stated / 2 <= meas[q] <= stated * 1.25 and 10 * meas[q] <= tol, (q, meas[q], stated)
            assert tol <= cap * (wc.CAP["eta"] if q == "eta" else wc.CAP["U"])
