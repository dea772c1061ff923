"""Every contact-free rollout kernel - one lane per sample (`lane`), four (`quad`), eight (`oct`), eight with helper wavefronts
(`oct-pair`, csrc/mppi_oct_pair.hpp) and whatever mppi_create selects by itself - against the fp64 oracle at the edges of the
helper kernel: horizons shorter than its prefetch pipeline and as long as its control table, sample counts around a workgroup
and around one workgroup per CU, the general control path (prior / null sample, absolute control cost, nu < bodies, a mixed
command map), a visualised link that is not the cost link, folded records over consecutive launches, non-finite costs.

ONE table (CASES); per case the oracle runs once and every kernel of the case is compared with it PER SAMPLE, EVERY SAMPLE, at the
contact-free tolerances of tests/test_gpu_parity.py: S 1e-4 relative, du 1e-6, visualisation rows 1e-4, action and every row of the
updated nominal 1e-3 |u_max|, (beta, eta) 2e-3 relative.  The kernel that ran is asserted by exact name and wavefront count from
mppi_kernel_info; where both `oct` and `oct-pair` run a case their results are compared for EQUALITY.
Cases of several launches on one context compare nominal, action, beta and eta with the oracle's own closed loop, and the per-sample
quantities of a later launch with the oracle's rollout from the nominal the device started that launch from.

test_matrix_cases_are_well_posed (no GPU) checks on the oracle alone that a pass means something: costs finite and of one sign,
the fp32 build of the oracle within 1e-5 of the fp64 one on every sample (a tenth of the tolerance), no sample with more than 0.9
of the softmax weight (the update would be one sample's du and hide the row sums), a non-zero nominal, controls that reach the
clamp in some but not all entries, a prior that differs from zero, from the nominal and from step to step."""
import contextlib
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

from mppiisaac.backend import capi
from scenes import panda_reach, point_reach

FLT_MAX = float(np.finfo(np.float32).max)
LANE, QUAD, OCT, PAIR, AUTO = "lane", "quad", "oct", "oct-pair", "default"
FOUR = (LANE, QUAD, OCT, PAIR)
TOL = {"S": 1e-4, "du": 1e-6, "viz": 1e-4, "U": 1e-3, "action": 1e-3, "beta_eta": 2e-3}   # (U, action: times |u_max|)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    make: object                 # panda_reach / point_reach
    K: int                       # samples: K + cu * (CUs of the device)
    H: int
    kernels: tuple
    cu: int = 0
    over: tuple = ()             # MPPIConfig fields, as (name, value) pairs
    prior: bool = False          # use_priors with a prior sequence
    cmd_map: bool = False        # nu = 5 commands drive the 7 joints through a mixed two-term map
    viz: str = ""                # visualised link (default: the scene's, which is the cost link)
    fold: bool = False           # MPPI_FOLD=1
    iters: int = 1               # consecutive mppi_command calls on one context
    shards: tuple = ()           # sample counts of the shards of one K_total (records combined by mppi_update)
    u0: float = 0.25             # amplitude of the nominal plan, in units of |u_max|


# the softmax temperature of the matrix: 0.5 (panda; the shipped 0.05 leaves one sample with all the weight from K = 24, H = 31 on)
# and 5 (point robot: costs of 70 to 160).  The control-cost term grows with the temperature and with the nominal: at 2.0 it pulls
# panda costs across zero, where a relative tolerance means nothing - the cases that need more temperature take a smaller nominal.
def P(name, K, H, kernels, **kw):
    over = dict(lambda_=0.5)
    over.update(kw.pop("over", {}))
    return Case(f"panda-{name}", panda_reach, K, H, kernels, over=tuple(sorted(over.items())), **kw)


def Q(name, K, H, kernels, **kw):
    over = dict(lambda_=5.0)
    over.update(kw.pop("over", {}))
    return Case(f"point-{name}", point_reach, K, H, kernels, over=tuple(sorted(over.items())), **kw)


PRIOR = dict(prior=True, over=dict(use_priors=True, sample_null_action=True))
CASES = []
# 1. horizon: the helper's prefetch pipeline is two rows deep (H = 1, 2, 3), its table has 32 rows (H = 31, 32); beyond, the kernel
#    without helpers runs whatever was asked for.  K = 40 / 77: the last workgroup is half empty / one owner short of three samples
#    (long horizons spread the costs: a higher temperature keeps several samples in the update, a smaller nominal keeps its
#    control-cost term, which grows with the temperature, from spreading them again)
LONG_P, LONG_Q = dict(u0=0.05, over=dict(lambda_=1.0)), dict(u0=0.03, over=dict(lambda_=20.0))
for H in (1, 2, 3):
    CASES += [P(f"H{H}", 40, H, FOUR), Q(f"H{H}", 77, H, FOUR)]
for H in (31, 32):
    CASES += [P(f"H{H}", 40, H, FOUR), Q(f"H{H}", 77, H, FOUR, **LONG_Q)]
for H in (33, 64):
    CASES += [P(f"H{H}", 40, H, FOUR + (AUTO,), **LONG_P), Q(f"H{H}", 77, H, FOUR + (AUTO,), **LONG_Q)]
# 2. sample count: one owner wavefront, both, a second workgroup (its second owner entirely dead at K = 17), the aligned and the
#    tail path of the record; one workgroup per CU exactly, one sample fewer, one and sixteen more (forced: more workgroups than CUs)
for K in (8, 9, 15, 16, 17, 31, 33):
    CASES += [P(f"K{K}", K, 12, (AUTO, OCT, QUAD, LANE)), Q(f"K{K}", K, 10, (AUTO, OCT, QUAD, LANE))]
CASES += [P("K16cu-1", -1, 12, (AUTO, OCT), cu=16), P("K16cu", 0, 12, (AUTO, OCT, QUAD, LANE), cu=16),
          P("K16cu+1", 1, 12, (AUTO, PAIR), cu=16), P("K16cu+16", 16, 12, (AUTO, PAIR), cu=16),
          Q("K16cu", 0, 10, (AUTO, OCT, QUAD, LANE), cu=16), Q("K16cu+1", 1, 10, (AUTO, PAIR), cu=16)]
# 3. control path: absolute control cost; prior (sample K - 2) and null sample (K - 1) in one wavefront (K = 16: 14, 15; K = 1000:
#    998, 999), in the two owner wavefronts of one workgroup (K = 9: 7 | 8), in two workgroups (K = 17: 15 | 16); the same on two
#    shards of one K_total, both in the second shard (16 + 17) and with the shard boundary elsewhere (24 + 9)
CASES += [P("abs-cost", 1000, 20, FOUR, over=dict(noise_abs_cost=True)), Q("abs-cost", 77, 15, FOUR, over=dict(noise_abs_cost=True))]
for K in (9, 16, 17, 1000):
    CASES.append(P(f"prior-K{K}", K, 20, FOUR, **PRIOR))
CASES += [Q("prior-K17", 17, 15, FOUR, **PRIOR), Q("prior-K9", 9, 15, FOUR, **PRIOR),
          P("prior-shards16+17", 33, 20, FOUR, shards=(16, 17), **PRIOR), P("prior-shards24+9", 33, 20, FOUR, shards=(24, 9), **PRIOR)]
# 4. command map: five commands, seven joints, two terms per joint (not the identity, nu != bodies)
CASES.append(P("cmd-map", 100, 20, FOUR, cmd_map=True, over=dict(noise_sigma=(0.1 * np.eye(5)).tolist())))
CASES.append(P("cmd-map-prior", 33, 20, FOUR, cmd_map=True, prior=True,
               over=dict(noise_sigma=(0.1 * np.eye(5)).tolist(), use_priors=True, sample_null_action=True)))
# 5. the visualised link is not the cost link (the second hand-over ring)
CASES += [P("viz-link4", 100, 20, FOUR, viz="panda_link4"), P("viz-link4-H32", 24, 32, FOUR, viz="panda_link4")]
# 6. folded records: 16 workgroups (eight fold groups) and 13 (one), three launches on one context
#    (the fold counters must be back at zero for the next launch), and the same loop without the fold
FOLD = dict(fold=True, iters=3)
CASES += [P("fold-K256", 256, 12, (QUAD, OCT, PAIR), **FOLD), P("fold-K200", 200, 12, (QUAD, OCT, PAIR), **FOLD),
          Q("fold-K256", 256, 10, (QUAD, OCT, PAIR), **FOLD), Q("fold-K77", 77, 10, (QUAD, OCT, PAIR), **FOLD), P("loop-K200", 200, 12, FOUR, iters=3)]
IDS = [c.name for c in CASES]


@dataclasses.dataclass
class Built:
    case: Case
    scene: object
    m: object
    cfg: object
    cost: object
    dof: np.ndarray
    root: np.ndarray
    U0: np.ndarray
    prior: object
    umax: float


def build(case, cus):
    K = case.K + case.cu * cus
    scene, m, cfg, cost, dof, root = case.make(K=K, H=case.H, **dict(case.over))
    if case.cmd_map:
        m.nu = 5
        for i in range(m.n_bodies):
            m.cmd_col[i][0], m.cmd_col[i][1] = i % 5, (i + 2) % 5
            m.cmd_coef[i][0], m.cmd_coef[i][1] = 1.0, 0.5
        assert cfg.nu == 5
    if case.viz:
        cfg.viz_link, cfg.want_rollouts = scene.link_names.index(case.viz), 1
        assert cfg.viz_link != cost.link[0]
    umax = max(abs(cfg.u_max[0]), abs(cfg.u_min[0]))
    H, nu = case.H, cfg.nu
    U0 = (case.u0 * umax * np.random.default_rng(0).normal(size=(H, nu))).astype(np.float32)
    prior = None
    if case.prior:
        prior = (0.5 * umax * np.cos(0.7 * np.arange(H)[:, None] + np.arange(nu)[None, :] + 0.3)).astype(np.float32)
    return Built(case, scene, m, cfg, cost, np.asarray(dof, np.float32), np.asarray(root, np.float32), U0, prior, umax)


def run_oracle(o, b, eps, iters=None):
    """the closed loop of `iters` control iterations at one state on the oracle: per iteration everything the GPU run returns"""
    U, outs = b.U0.astype(np.float64), []
    for _ in range(iters or b.case.iters):
        S, du, viz = o.rollout(b.m, b.cfg, b.cost, b.dof, b.root, U, eps, prior=b.prior, want_viz=bool(b.cfg.want_rollouts))
        U1, action, be = o.update(b.cfg, o.record(b.cfg, S, du), U)
        outs.append({"S": S, "du": du, "viz": viz, "U": U1, "action": action, "beta_eta": be})
        U = U1
    return outs


# ---- the conditions on the inputs, on the oracle alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matrix_cases_are_well_posed(case, oracle64, oracle32):
    assert IDS.count(case.name) == 1
    b = build(case, 256)
    cfg, K = b.cfg, b.cfg.num_samples
    assert not case.shards or sum(case.shards) == K
    eps = oracle64.sample(cfg)
    o64, o32 = run_oracle(oracle64, b, eps), run_oracle(oracle32, b, eps)
    for it, (a, c) in enumerate(zip(o64, o32)):
        S = a["S"]
        assert np.isfinite(S).all() and ((S > 0).all() or (S < 0).all()), "costs finite and of one sign"
        rel = np.abs(c["S"] - S) / np.abs(S)
        eta = a["beta_eta"][1]
        print(f"{case.name} it {it}: S in [{S.min():.3f}, {S.max():.3f}], fp32 oracle within {rel.max():.1e}, eta {eta:.3f}")
        assert rel.max() <= 1e-5, "the fp32 oracle leaves the fp64 one by more than a tenth of the tolerance"
        assert 1.0 / eta <= 0.9, "one sample carries more than 0.9 of the weight: the update hides the row sums"
    assert np.abs(b.U0).min() > 0
    u = b.U0[:, :, None].astype(np.float64) + eps
    lo, hi = np.array([cfg.u_min[j] for j in range(cfg.nu)]), np.array([cfg.u_max[j] for j in range(cfg.nu)])
    clamped = np.mean((u > hi[None, :, None]) | (u < lo[None, :, None]))
    print(f"{case.name}: {100 * clamped:.1f} % of the controls reach the clamp")
    assert 0.01 <= clamped <= 0.80
    if case.prior:
        assert cfg.use_priors and cfg.sample_null_action
        # (every row of it, by a twentieth of the control range in some control at least)
        far = lambda d: np.abs(d).max(axis=1).min() > 0.05 * b.umax
        assert far(b.prior) and far(b.prior - b.U0) and far(np.diff(b.prior, axis=0))
        # ... and it is in use: the prior sample's perturbation is prior - U, not the noise
        np.testing.assert_allclose(o64[0]["du"][:, :, K - 2], np.clip(b.prior, lo, hi) - b.U0, atol=1e-12)
        np.testing.assert_allclose(o64[0]["du"][:, :, K - 1], np.clip(0.0, lo, hi) - b.U0, atol=1e-12)


# ---- the GPU side ------------------------------------------------------------------------------------------------------------------
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


def expected_kernel(kernel, K, H, cus):
    """name and wavefront count mppi_kernel_info must report (mppi_create's selection, csrc/mppi_hip.hip)"""
    w16 = (K + 15) // 16
    if kernel == LANE:
        return LANE, (K + 63) // 64
    if kernel == QUAD or K < 8:
        return QUAD, w16
    if kernel == OCT:
        return OCT, 2 * w16
    if kernel != PAIR and (K + 7) // 8 > 4 * cus:          # (the octet kernel is selected up to one wavefront per SIMD)
        return QUAD, w16
    if H <= 32 and (kernel == PAIR or w16 <= cus):          # the control table has 32 rows; one workgroup per CU unless forced
        return PAIR, 4 * w16
    return OCT, 2 * w16


class Gpu:
    """one context through the raw C-ABI"""

    def __init__(self, lib, b, kernel, cfg=None, fold=False):
        self.lib, self.cfg = lib, cfg if cfg is not None else b.cfg
        self.ctx = C.c_void_p()
        with environment(MPPI_ROLLOUT=None if kernel == AUTO else kernel, MPPI_FOLD="1" if fold else None):
            capi.check(lib, lib.mppi_create(C.byref(b.m), C.byref(self.cfg), 0, C.byref(self.ctx)))
        self.K, self.H, self.nu = self.cfg.num_samples, self.cfg.horizon, self.cfg.nu
        if b.cost is not None:
            self.call("mppi_set_cost", C.byref(b.cost))
        buf = C.create_string_buffer(512)
        self.call("mppi_kernel_info", buf, 512)
        self.info = buf.value.decode() + " "
        self.call("mppi_sample", C.c_uint32(0))
        self.eps = self.get("mppi_get_noise", (self.H, self.nu, self.K))
        self.call("mppi_set_state", capi.fptr(b.dof), capi.fptr(b.root))
        self.call("mppi_set_nominal", capi.fptr(b.U0))
        if b.prior is not None:
            self.call("mppi_set_prior", capi.fptr(b.prior))

    def call(self, name, *args):
        capi.check(self.lib, getattr(self.lib, name)(self.ctx, *args))

    def get(self, name, shape):
        out = np.zeros(shape, np.float32)
        self.call(name, capi.fptr(out))
        return out

    def rollout_outputs(self):
        out = {"S": self.get("mppi_get_costs", (self.K,)), "du": self.get("mppi_get_perturbations", (self.H, self.nu, self.K))}
        out["viz"] = self.get("mppi_get_rollouts", (self.H, self.K, 3)) if self.cfg.want_rollouts else None
        return out

    def update_outputs(self, out):
        out["beta_eta"] = self.get("mppi_get_weights_stats", (2,))
        out["U"] = self.get("mppi_get_nominal", (self.H, self.nu))
        out["action"] = self.get("mppi_get_action", (self.nu,))
        return out

    def close(self):
        self.lib.mppi_destroy(self.ctx)


def assert_kernel(g, kernel, cus):
    name, waves = expected_kernel(kernel, g.K, g.H, cus)
    assert f"rollout={name} " in g.info and f" waves={waves} " in g.info, (kernel, g.info)
    return name


def run_gpu(lib, b, kernel, cus):
    """-> (kernel name, eps, per iteration the outputs) of one context, or of the shards of one K_total put together"""
    case = b.case
    if not case.shards:
        g = Gpu(lib, b, kernel, fold=case.fold)
        name = assert_kernel(g, kernel, cus)
        assert lib.mppi_shard_record_count(g.ctx) == ((8 if ((g.K + 15) // 16) % 16 == 0 else 1) if case.fold and name != LANE else 0)
        outs = []
        for _ in range(case.iters):
            U_in, action = g.get("mppi_get_nominal", (g.H, g.nu)), np.zeros(g.nu, np.float32)
            g.call("mppi_command", capi.fptr(action))
            outs.append(g.update_outputs(g.rollout_outputs()))
            outs[-1]["U_in"] = U_in
            np.testing.assert_array_equal(action, outs[-1]["action"])
        g.close()
        return name, g.eps, outs
    import torch
    RF = 2 + b.cfg.horizon * b.cfg.nu
    records = torch.zeros((len(case.shards), RF), dtype=torch.float32, device="cuda")
    gs, parts, off = [], [], 0
    for r, n in enumerate(case.shards):
        cfg = type(b.cfg).from_buffer_copy(b.cfg)
        cfg.num_samples, cfg.k_offset = n, off
        assert cfg.k_total == b.cfg.num_samples
        off += n
        g = Gpu(lib, b, kernel, cfg=cfg)
        name = assert_kernel(g, kernel, cus)
        g.call("mppi_rollout")
        parts.append(g.rollout_outputs())
        g.call("mppi_reduce", C.c_void_p(records[r].data_ptr()))
        gs.append(g)
    out = {"S": np.concatenate([p["S"] for p in parts]), "du": np.concatenate([p["du"] for p in parts], axis=2),
           "viz": np.concatenate([p["viz"] for p in parts], axis=1) if parts[0]["viz"] is not None else None}
    ups = []
    for g in gs:
        g.call("mppi_update", C.c_void_p(records.data_ptr()), len(gs))
        ups.append(g.update_outputs({}))
        g.close()
    for u in ups[1:]:                       # every shard combines the same records: the same update, bit for bit
        for k in u:
            np.testing.assert_array_equal(u[k], ups[0][k], err_msg=k)
    out.update(ups[0], U_in=b.U0)
    return name, np.concatenate([g.eps for g in gs], axis=2), [out]


def compare(tag, got, want, umax, tol=None):
    """prints the measured maxima next to the tolerances (TOL, or the table `tol` of a module that measured its own), then
    asserts; -> the list of failures"""
    tols = TOL if tol is None else tol
    fails, cells = [], []
    for key in ("S", "du", "viz", "U", "action", "beta_eta"):
        if want[key] is None:
            continue
        g, w = got[key].astype(np.float64), np.asarray(want[key], np.float64)
        assert g.shape == w.shape, (key, g.shape, w.shape)
        if key in ("S", "beta_eta"):
            err, tol, unit = np.abs(g - w) / np.abs(w), tols[key], "rel"
        else:
            err, tol, unit = np.abs(g - w), tols[key] * (umax if key in ("U", "action") else 1.0), "abs"
        worst = err.max() if np.isfinite(g).all() else np.inf
        cells.append(f"{key} {worst:.1e} ({unit} tol {tol:.1e})")
        if not worst <= tol:
            fails.append(f"{tag}: {key} off by {worst:.3e} > {tol:.1e} at {np.unravel_index(np.argmax(np.nan_to_num(err, nan=np.inf)), err.shape)}")
    print(f"{tag}: " + " | ".join(cells))
    return fails


@pytest.fixture(scope="module")
def device():
    import torch
    assert torch.cuda.is_available()
    return capi.load_library(), torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_match_the_oracle_per_sample(case, device, oracle64):
    lib, cus = device
    b = build(case, cus)
    runs, fails, want = {}, [], None
    for kernel in case.kernels:
        name, eps, outs = run_gpu(lib, b, kernel, cus)
        if want is None:                    # the oracle runs once per case, on the noise the device sampled
            np.testing.assert_allclose(eps, oracle64.sample(b.cfg), atol=1e-6)
            eps0, want = eps, run_oracle(oracle64, b, eps)
        np.testing.assert_array_equal(eps, eps0)
        for it, (got, ref) in enumerate(zip(outs, want)):
            if it > 0:
                # Later launches of one context: nominal, action, beta and eta against the oracle's own closed loop; the PER-SAMPLE
                # quantities against the oracle's rollout from the nominal the device started this launch from.  The perturbation
                # of a clamped control is u_lim - U: the difference of the two loops' nominals (fp32 / fp64 updates, within the
                # nominal's tolerance) passes straight into it, and 1e-6 is a tolerance for equal inputs.
                np.testing.assert_array_equal(got["U_in"], outs[it - 1]["U"])
                S, du, viz = oracle64.rollout(b.m, b.cfg, b.cost, b.dof, b.root, got["U_in"], eps, prior=b.prior, want_viz=bool(b.cfg.want_rollouts))
                ref = dict(ref, S=S, du=du, viz=viz)
            fails += compare(f"{case.name} K={b.cfg.num_samples} H={case.H} asked {kernel} ran {name} it {it}", got, ref, b.umax)
        runs.setdefault(name, outs)
    assert len(want) == case.iters
    if OCT in runs and PAIR in runs:        # the helpers issue the same operations on the same values in the same order
        for got, ref in zip(runs[PAIR], runs[OCT]):
            for key in got:
                if got[key] is not None and ref.get(key) is not None:
                    np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{case.name}: oct-pair vs oct, {key}")
    assert not fails, "\n".join(fails)


# ---- non-finite costs --------------------------------------------------------------------------------------------------------------
def planted(K):
    """non-finite values at the first and the last sample, a whole 16-sample group, a whole wavefront of 64"""
    v = np.zeros(K, np.float32)
    v[0], v[K - 1] = np.nan, np.inf
    v[16:32] = np.inf
    v[64:128] = np.where(np.arange(64) % 3 == 0, np.nan, -np.inf)
    v[40] = -np.inf
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("route,kernel", [("horizon", AUTO), ("horizon", QUAD), ("accumulate", AUTO), ("accumulate", QUAD), ("accumulate", LANE)])
def test_nonfinite_host_costs_are_rejected_as_the_oracle_rejects_them(route, kernel, device, oracle64):
    """NaN, +Inf and -Inf among the costs a host-side Objective returns (mppi_reduce_horizon_costs: the stage costs of all H * K
    env-steps; mppi_sim_accumulate_cost + mppi_reduce: one value per sample): the records (k_horizon_reduce_quad, k_reduce_quad,
    k_reduce) and the combine skip them as oracle.record does - beta, eta, nominal and action from the remaining samples."""
    import torch
    lib, cus = device
    K, H = 200, 12
    b = build(P("nonfinite", K, H, (kernel,)), cus)
    plant = planted(K)
    g = Gpu(lib, b, kernel)
    if route == "horizon":
        g.call("mppi_rollout_trajectory")
        c = torch.full((H, K), 0.25, dtype=torch.float32, device="cuda") * torch.linspace(0.5, 1.5, K, device="cuda")[None, :]
        c[H // 2] += torch.from_numpy(plant).cuda()
        c[H - 1, 150] = float("nan")
        plant[150] = np.nan
        g.call("mppi_reduce_horizon_costs", C.c_void_p(c.data_ptr()), None)
    else:
        g.call("mppi_rollout")
        c = torch.from_numpy(plant).cuda()
        g.call("mppi_sim_accumulate_cost", 0, C.c_void_p(c.data_ptr()))
        g.call("mppi_reduce", None)
    torch.cuda.synchronize()
    S, du = g.get("mppi_get_costs", (K,)), g.get("mppi_get_perturbations", (H, g.nu, K))
    g.call("mppi_update", None, 1)
    got = g.update_outputs({})
    g.close()
    np.testing.assert_array_equal(np.isfinite(S), plant == 0)
    assert np.isnan(S[np.isnan(plant)]).all() and (S[plant == np.inf] == np.inf).all() and (S[plant == -np.inf] == -np.inf).all()
    Uo, ao, beo = oracle64.update(b.cfg, oracle64.record(b.cfg, S, du), b.U0)
    assert 1.0 / beo[1] <= 0.9 and np.isfinite(Uo).all()
    want = {"S": None, "du": None, "viz": None, "U": Uo, "action": ao, "beta_eta": beo}
    fails = compare(f"non-finite host costs, {route}, {kernel}", got, want, b.umax)
    assert not fails, "\n".join(fails)


# the reach weights scaled so that about half of the trajectory costs exceed FLT_MAX.  (The temperature stays: at costs of 1e38 the
# cheapest finite sample carries all the weight, eta = 1 - the update that is compared is that sample's du.  Scaling the temperature
# along would scale the control-cost term, whose partial sums overflow fp32 on their own.)
OVERFLOW = {"panda": (panda_reach, 1000, 20, 5.009e37), "point": (point_reach, 77, 15, 3.57e36)}


def build_overflow(which, cus=256):
    make, K, H, scale = OVERFLOW[which]
    b = build((P if make is panda_reach else Q)("overflow", K, H, FOUR), cus)
    for i in range(2):
        b.cost.w[i] *= scale
    return b


def overflow_reference(o, b, eps):
    """fp64 costs, which of them fp32 cannot hold, and how far the nearest one is from that threshold"""
    S, du, _ = o.rollout(b.m, b.cfg, b.cost, b.dof, b.root, b.U0, eps)
    S = S.astype(np.float64)
    over = ~np.isfinite(S) | (S > FLT_MAX)
    gap = np.min(np.abs(S[np.isfinite(S)] / FLT_MAX - 1.0))
    return S, du, over, gap


@pytest.mark.parametrize("which", sorted(OVERFLOW))
def test_overflow_cases_are_well_posed(which, oracle64, oracle32):
    b = build_overflow(which)
    eps = oracle64.sample(b.cfg)
    S, du, over, gap = overflow_reference(oracle64, b, eps)
    S32, _, _ = oracle32.rollout(b.m, b.cfg, b.cost, b.dof, b.root, b.U0, eps)
    print(f"{which}: {over.sum()} of {len(S)} costs beyond FLT_MAX, the nearest {gap:.1e} (relative) from it")
    assert 0.3 <= over.mean() <= 0.7 and gap >= 1e-4
    np.testing.assert_array_equal(~np.isfinite(S32), over)          # the fp32 oracle names the same samples
    assert (S > 0).all() and np.max(np.abs(S32[~over] - S[~over]) / S[~over]) <= 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(OVERFLOW))
def test_costs_beyond_fp32_are_rejected_in_the_fused_kernels(which, device, oracle64):
    """Costs that overflow fp32 inside the fused rollout (the stage costs are positive, so the discounted sum passes FLT_MAX exactly when
    the total does): the device's set of non-finite samples is the oracle's set of costs beyond FLT_MAX, the others agree per sample,
    the update is the oracle's over the finite samples, nothing non-finite reaches the nominal.
    A true NaN in SINGLE samples of a fused rollout has no route that leaves product code alone: state, goal and weights are shared
    by all samples and the noise comes from the sampler; NaN in records and in the combine is covered by the host-cost routes above
    and by the all-rejected case below."""
    lib, cus = device
    b = build_overflow(which, cus)
    want = None
    for kernel in b.case.kernels:
        g = Gpu(lib, b, kernel)
        name = assert_kernel(g, kernel, cus)
        action = np.zeros(g.nu, np.float32)
        g.call("mppi_command", capi.fptr(action))
        got = g.update_outputs(g.rollout_outputs())
        g.close()
        if want is None:
            S, du, over, gap = overflow_reference(oracle64, b, g.eps)
            assert gap >= 1e-4
            Uo, ao, beo = oracle64.update(b.cfg, oracle64.record(b.cfg, np.where(over, np.inf, S), du), b.U0)
            want = {"S": None, "du": du, "viz": None, "U": Uo, "action": ao, "beta_eta": beo}
        np.testing.assert_array_equal(~np.isfinite(got["S"]), over, err_msg=f"{which} {name}: the set of rejected samples")
        rel = np.abs(got["S"][~over] - S[~over]) / S[~over]
        print(f"{which} overflow, {name}: {over.sum()} of {len(S)} rejected, finite costs within {rel.max():.1e} (rel tol 1e-04)")
        assert rel.max() <= TOL["S"]
        assert np.isfinite(got["U"]).all() and np.isfinite(got["action"]).all()
        fails = compare(f"{which} overflow, {name}", got, want, b.umax)
        assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["panda", "point"])
def test_all_samples_rejected_keeps_the_nominal(which, device):
    """A NaN goal: every cost is NaN, every sample is rejected.  The oracle divides 0 / 0 there; the device's behaviour is stated in
    include/mppi_hip.h (mppi_update): eta = 0, the nominal is kept - then shifted, u_init appended -, the action is the old first
    row, nothing non-finite reaches the nominal.  All four kernels, two sample counts (aligned / tail path of the record)."""
    lib, cus = device
    for K in (32, 77):
        b = build((P if which == "panda" else Q)("nan-goal", K, 12, FOUR), cus)
        b.root[b.cost.actor[0], 0:3] = np.nan
        for kernel in FOUR:
            g = Gpu(lib, b, kernel)
            name = assert_kernel(g, kernel, cus)
            action = np.zeros(g.nu, np.float32)
            g.call("mppi_command", capi.fptr(action))
            got = g.update_outputs(g.rollout_outputs())
            g.close()
            assert not np.isfinite(got["S"]).any(), name
            assert np.isfinite(got["du"]).all() and got["beta_eta"][1] == 0.0 and np.isposinf(got["beta_eta"][0]), (name, got["beta_eta"])
            np.testing.assert_array_equal(action, b.U0[0], err_msg=name)
            np.testing.assert_array_equal(got["U"][:-1], b.U0[1:], err_msg=name)
            np.testing.assert_array_equal(got["U"][-1], np.float32(b.cfg.u_init), err_msg=name)
