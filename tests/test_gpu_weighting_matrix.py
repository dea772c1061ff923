"""The MPPI weighting kernels against the fp64 reference ON THE DEVICE'S OWN INPUTS (tests/weighting_cases.py): no dynamics oracle in
the loop, so what is left between the device and the reference is fp32 summation and __expf, and the tolerances are the sized ones of
weighting_cases.TOL* - two to three orders of magnitude under the end-to-end ones (U 1e-3 |u_max|, eta 2e-3).

  route A  synthetic records [nrec][2 + HN] -> mppi_update (k_combine: combine_update<1024>) and mppi_update_step_world with a K = 1
           world (k_combine_world: combine_update<512>; from csrc/mppi_hip.hip: every contact-free fixed-base context has a
           launch_combine_world, the 12-command tree included - the test asserts that the contexts of these rows are no contact
           scene, and that the world moved); U, action, (beta, eta) against the fp64 combine of the same records
  route B  exact costs S into the record kernels over du of a rollout: mppi_sim_accumulate_cost + mppi_reduce (k_reduce_quad; k_reduce
           under MPPI_ROLLOUT=lane) and mppi_reduce_horizon_costs (k_horizon_reduce_quad, discount 1.0 and 0.9); the mode-0 shard
           record and, after mppi_update, U, action, (beta, eta) against the fp64 record of the S and du read back
  route C  the fused kernels' own records (lane, quad, oct, oct-pair by exact name) and, under MPPI_FOLD=1, every folded record of
           fold_group against the fp64 record of its samples; the two counts beyond fold_group's table of 1024 records

beta is compared bit for bit everywhere.  Every test prints its measured maxima next to the tolerances before it asserts."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import weighting_cases as wc
from mppiisaac.backend import capi
from scenes import point_reach

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def environment(**kv):
    """MPPI_ROLLOUT / MPPI_FOLD are read by mppi_create"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


class Ctx:
    """one context through the raw C-ABI"""

    def __init__(self, lib, m, cfg, dof, root, cost=None, kernel=None, fold=False):
        self.lib, self.cfg, self.ctx = lib, cfg, C.c_void_p()
        with environment(MPPI_ROLLOUT=kernel, MPPI_FOLD="1" if fold else None):
            capi.check(lib, lib.mppi_create(C.byref(m), C.byref(cfg), 0, C.byref(self.ctx)))
        self.K, self.H, self.nu = cfg.num_samples, cfg.horizon, cfg.nu
        self.RF = 2 + self.H * self.nu
        if cost is not None:
            self.call("mppi_set_cost", C.byref(cost))
        buf = C.create_string_buffer(512)
        self.call("mppi_kernel_info", buf, 512)
        self.info = buf.value.decode() + " "
        self.call("mppi_set_state", capi.fptr(np.ascontiguousarray(dof, np.float32)), capi.fptr(np.ascontiguousarray(root, np.float32)))

    def call(self, name, *args):
        capi.check(self.lib, getattr(self.lib, name)(self.ctx, *args))

    def get(self, name, shape):
        out = np.zeros(shape, np.float32)
        self.call(name, capi.fptr(out))
        return out

    def set_U(self, U):
        self.call("mppi_set_nominal", capi.fptr(np.ascontiguousarray(U, np.float32)))

    def update_outputs(self):
        be = self.get("mppi_get_weights_stats", (2,))
        return {"U": self.get("mppi_get_nominal", (self.H, self.nu)).astype(np.float64), "action": self.get("mppi_get_action", (self.nu,)).astype(np.float64),
                "beta": float(be[0]), "eta": float(be[1])}

    def close(self):
        self.lib.mppi_destroy(self.ctx)


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return capi.load_library()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr())


MAXIMA = {}


def note(cls, **figures):
    m = MAXIMA.setdefault(cls, {})
    for k, v in figures.items():
        m[k] = max(m.get(k, 0.0), v)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for cls in sorted(MAXIMA):
        print(f"\nmeasured maxima, class {cls}: " + ", ".join(f"{k} {v:.1e}" for k, v in sorted(MAXIMA[cls].items())), end="")
    print()


def check_update(tag, got, want, umax, tol, cls):
    """beta bit for bit, eta relative, U and action in units of |u_max|; prints before it asserts"""
    assert np.isfinite(got["U"]).all() and np.isfinite(got["action"]).all() and np.isfinite(got["eta"]), f"{tag}: non-finite update {got}"
    d = wc.deviation(got, want, umax)
    print(f"{tag}: eta {d['eta']:.1e} (tol {tol['eta']:.0e}) | U, action {d['U']:.1e} (tol {tol['U']:.0e} |u_max|) | beta {got['beta']!r} vs {want['beta']!r}")
    note(cls, **d)
    assert np.float32(got["beta"]) == np.float32(want["beta"]), f"{tag}: beta {got['beta']!r} != {want['beta']!r}"
    assert d["eta"] <= tol["eta"] and d["U"] <= tol["U"], f"{tag}: {d} beyond {tol}"


# ---- route A ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts(lib):
    """(planner, world or None, shape) per (HN, world, u_init): the contexts supply (H, nu) only, no rollout runs"""
    cache = {}

    def get(HN, world, u_init):
        key = (HN, world, u_init)
        if key not in cache:
            shape = wc.make_shape(HN, u_init=u_init)
            p = Ctx(lib, shape.m, shape.cfg, shape.dof, shape.root)
            w = None
            if world:
                ws = wc.make_shape(HN, K=1)
                w = Ctx(lib, ws.m, ws.cfg, shape.dof, shape.root)
                w.call("mppi_sim_reset")
                assert "step=scene" not in p.info and "step=scene" not in w.info, "a contact scene falls back to mppi_update: k_combine"
            cache[key] = (p, w, shape)
        return cache[key]
    yield get
    for p, w, _ in cache.values():
        p.close()
        if w is not None:
            w.close()


@pytest.mark.parametrize("row", wc.ROWS, ids=wc.ROW_IDS)
def test_combine_of_synthetic_records(row, lib, contexts):
    p, w, shape = contexts(row.HN, row.world, row.u_init)
    H, nu = p.H, p.nu
    F = wc.savgol_matrix(H).astype(np.float32) if row.filt else None
    p.call("mppi_set_filter", capi.fptr(np.ascontiguousarray(F)) if F is not None else None)
    U0 = wc.nominal(shape)
    p.set_U(U0)
    try:
        for lam in wc.row_lambda(row, shape):
            if row.lam_scale:
                p.call("mppi_set_lambda", C.c_double(lam))
            recs, _ = wc.make_records(row, shape, lam)
            d_recs = dev(recs)
            if row.world:
                dof0 = np.zeros(2 * shape.m.n_bodies, np.float32)
                p.call("mppi_get_state", capi.fptr(dof0), None)
                capi.check(lib, lib.mppi_update_step_world(p.ctx, ptr(d_recs), row.nrec, w.ctx))
            else:
                p.call("mppi_update", ptr(d_recs), row.nrec)
            got = p.update_outputs()
            want = wc.update64(recs, U0, lam, row.u_init, F)
            tag = f"{row.name} ({'k_combine_world' if row.world else 'k_combine'}, lambda {lam:g}: {row.why})"
            if row.cls == "g":      # include/mppi_hip.h, mppi_update: the nominal kept and shifted, u_init appended, the old first row
                print(f"{tag}: beta {got['beta']}, eta {got['eta']}")
                assert np.isposinf(got["beta"]) and got["eta"] == 0.0
                np.testing.assert_array_equal(got["action"], U0[0])
                np.testing.assert_array_equal(got["U"][:-1], U0[1:])
                np.testing.assert_array_equal(got["U"][-1], np.float32(row.u_init))
            else:
                check_update(tag, got, want, shape.umax, row.tol, "A " + row.cls[0] + ("-big" if row.big else ""))
            if row.world:           # the world was stepped with the action and its state fed back: the fused tail ran to its end
                dof1 = np.zeros_like(dof0)
                p.call("mppi_get_state", capi.fptr(dof1), None)
                assert np.isfinite(dof1).all() and not np.array_equal(dof0, dof1)
            U0 = got["U"].astype(np.float32)
    finally:
        if row.lam_scale:
            p.call("mppi_set_lambda", C.c_double(shape.lam))
        p.call("mppi_set_filter", None)


# ---- route B ---------------------------------------------------------------------------------------------------------------------------
def b_context(lib, K, path):
    kernel, _, gamma = wc.B_PATHS[path]
    scene, m, cfg, cost, dof, root = point_reach(K=K, H=wc.B_H, lambda_=wc.B_LAMBDA, rollout_var_discount=gamma)
    g = Ctx(lib, m, cfg, dof, root, cost=cost, kernel=kernel)
    umax = np.tile([max(abs(cfg.u_max[j]), abs(cfg.u_min[j])) for j in range(cfg.nu)], cfg.horizon)
    return g, umax


@pytest.mark.parametrize("path", sorted(wc.B_PATHS))
@pytest.mark.parametrize("K", wc.B_K)
def test_records_of_injected_costs(K, path, lib):
    import torch
    kernel, served, gamma = wc.B_PATHS[path]
    g, umax = b_context(lib, K, path)
    try:
        # the kernel that serves the path (csrc/mppi_hip.hip mppi_reduce / mppi_reduce_horizon_costs): a context of the one-lane
        # rollout keeps records of 64 samples (k_reduce), every other one records of 16 (k_reduce_quad, k_horizon_reduce_quad)
        assert ("rollout=lane " in g.info) == (served == "k_reduce"), g.info
        H, nu = g.H, g.nu
        U0 = (0.25 * umax.reshape(H, nu) * np.random.default_rng(3).normal(size=(H, nu))).astype(np.float32)
        g.call("mppi_sample", C.c_uint32(0))
        g.set_U(U0)
        g.call("mppi_rollout")                                   # fills du; its costs are replaced below
        du = g.get("mppi_get_perturbations", (H, nu, K))
        if K >= 64:
            clamped = np.mean(np.abs(U0[:, :, None] + du) >= umax.reshape(H, nu)[:, :, None] * (1 - 1e-6))
            assert 0.01 <= clamped <= 0.8, "the noise reaches the clamp in some entries"
        rec_out = torch.zeros(g.RF, dtype=torch.float32, device="cuda")
        for kind in wc.B_COSTS:
            S_in = wc.make_costs(kind, K, wc.B_LAMBDA)
            g.set_U(U0)
            g.call("mppi_sim_reset")                             # S = 0, control cost = 0
            if path.startswith("accumulate"):
                d_S = dev(S_in)
                g.call("mppi_sim_accumulate_cost", 0, ptr(d_S))
                g.call("mppi_reduce", ptr(rec_out))
            else:
                c = wc.stage_costs(S_in, H, gamma)
                d_c = dev(c)
                g.call("mppi_reduce_horizon_costs", ptr(d_c), ptr(rec_out))
            S = g.get("mppi_get_costs", (K,))
            np.testing.assert_array_equal(g.get("mppi_get_perturbations", (H, nu, K)), du)
            tag = f"K={K} {path} ({served}) {kind}"
            if path.startswith("accumulate"):
                np.testing.assert_array_equal(S, S_in)
            else:
                np.testing.assert_array_equal(np.isfinite(S), np.isfinite(S_in))
                fin = np.isfinite(S)
                rel = np.max(np.abs(S[fin] - wc.horizon_sum64(c, gamma)[fin]) / np.abs(wc.horizon_sum64(c, gamma)[fin]))
                print(f"{tag}: S {rel:.1e} (tol {wc.TOL_B['S'][0]:.0e})")
                note("B", S=rel)
                assert rel <= wc.TOL_B["S"][0]
            want = wc.record64(S, du, wc.B_LAMBDA)
            rec = rec_out.cpu().numpy()
            d = wc.record_deviation((rec[0], rec[1], rec[2:]), want)
            print(f"{tag}: record eta {d['eta']:.1e} (tol {wc.TOL_B['eta'][0]:.0e}) | N {d['N']:.1e} (tol {wc.TOL_B['N'][0]:.0e}) | beta {rec[0]!r}")
            note("B", **d)
            assert np.isfinite(rec).all() and rec[0] == np.float32(want[0])
            assert d["eta"] <= wc.TOL_B["eta"][0] and d["N"] <= wc.TOL_B["N"][0], (tag, d)
            g.call("mppi_update", None, 1)
            ref = wc.finish64(U0, want[0], want[1], want[2], 0.0)
            check_update(tag + " update", g.update_outputs(), ref, umax, {q: wc.TOL_B[q][0] for q in ("eta", "U")}, "B")
    finally:
        g.close()


# ---- route C ---------------------------------------------------------------------------------------------------------------------------
def c_run(lib, K, H, kernel, fold):
    """one rollout of the point robot -> (S, du, the shard record of mppi_reduce, the folded records or None, info)"""
    import torch
    scene, m, cfg, cost, dof, root = point_reach(K=K, H=H, lambda_=wc.C_LAMBDA)
    g = Ctx(lib, m, cfg, dof, root, cost=cost, kernel=kernel, fold=fold)
    try:
        assert f"rollout={kernel} " in g.info, g.info
        n_fold = lib.mppi_shard_record_count(g.ctx)
        folded = None
        if n_fold:
            folded = torch.zeros((n_fold, g.RF), dtype=torch.float32, device="cuda")
            g.call("mppi_set_record_out", ptr(folded))
        g.call("mppi_sample", C.c_uint32(0))
        g.set_U(wc.c_nominal(cfg))
        g.call("mppi_rollout")
        rec_out = torch.zeros(g.RF, dtype=torch.float32, device="cuda")
        g.call("mppi_reduce", ptr(rec_out))
        S, du = g.get("mppi_get_costs", (K,)), g.get("mppi_get_perturbations", (H, g.nu, K))
        return S, du, rec_out.cpu().numpy(), None if folded is None else folded.cpu().numpy(), g.info
    finally:
        g.close()


def check_record(tag, rec, want, tol, cls):
    d = wc.record_deviation((rec[0], rec[1], rec[2:]), want)
    print(f"{tag}: eta {d['eta']:.1e} (tol {tol['eta'][0]:.0e}) | N {d['N']:.1e} (tol {tol['N'][0]:.0e}) | beta {rec[0]!r}")
    note(cls, **d)
    assert np.isfinite(rec).all() and rec[0] == np.float32(want[0]), (tag, rec[0], want[0])
    assert d["eta"] <= tol["eta"][0] and d["N"] <= tol["N"][0], (tag, d)


@pytest.mark.parametrize("H", wc.C_H)
@pytest.mark.parametrize("K", wc.C_K)
@pytest.mark.parametrize("kernel", wc.C_KERNELS)
def test_records_of_the_fused_kernels(kernel, K, H, lib):
    for fold in (False, True) if kernel != "lane" else (False,):
        S, du, rec, folded, info = c_run(lib, K, H, kernel, fold)
        assert np.isfinite(S).all()
        tag = f"{kernel} K={K} H={H}" + (" MPPI_FOLD=1" if fold else "")
        check_record(tag + " shard record", rec, wc.record64(S, du, wc.C_LAMBDA), wc.TOL_C, "C")
        if fold:
            assert folded is not None and len(folded) == (8 if ((K + 15) // 16) % 16 == 0 else 1)
            for gi, (a, b) in enumerate(wc.fold_groups(K, len(folded))):
                check_record(f"{tag} folded record {gi} (samples {a}..{b - 1})", folded[gi], wc.record64(S[a:b], du[:, :, a:b].reshape(-1, b - a), wc.C_LAMBDA), wc.TOL_C, "C")


@pytest.mark.parametrize("which", sorted(wc.C_FOLD_TABLE))
def test_fold_of_more_records_than_the_table_holds(which, lib):
    """fold_group keeps 1024 rescaling factors in LDS and recomputes those of the records beyond; here every group has more records than
    that, and the records beyond the table carry weight (asserted): dropping them, or a wrong recomputed factor, fails"""
    K = wc.C_FOLD_TABLE[which]
    S, du, rec, folded, info = c_run(lib, K, 2, "quad", True)
    assert np.isfinite(S).all() and folded is not None
    groups = wc.fold_groups(K, len(folded))
    assert len(folded) == (8 if which == "eight-groups" else 1) and f" waves={(K + 15) // 16} " in info, (len(folded), info)
    for gi, (a, b) in enumerate(groups):
        assert (b - a + 15) // 16 > wc.FOLD_TABLE          # (the record count of the group comes from the library's own counts above)
        want = wc.record64(S[a:b], du[:, :, a:b].reshape(-1, b - a), wc.C_LAMBDA)
        beyond = want[3][16 * wc.FOLD_TABLE:].sum() / want[1]
        print(f"{which} group {gi}: {(b - a + 15) // 16} wave records, those beyond the table carry {beyond:.1e} of the weight")
        assert beyond >= 100 * wc.TOL_C_BIG["eta"][0]
        check_record(f"{which} K={K} folded record {gi}", folded[gi], want, wc.TOL_C_BIG, "C-big")
    check_record(f"{which} K={K} shard record", rec, wc.record64(S, du, wc.C_LAMBDA), wc.TOL_C_BIG, "C-big")
