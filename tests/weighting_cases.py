"""The MPPI weighting on its own - the record kernels (wave_record, quad_record, oct_record2, record_rows), the fold inside the
rollout kernels (fold_group) and the combine / update (combine_update behind k_combine, k_combine_world, k_reduce_exchange) -
without the dynamics: case tables, builders of synthetic records and costs, the fp64 reference in plain numpy and its sequential
fp32 restatement.  No GPU import: tests/test_weighting_cases.py checks on the reference alone that a pass means something,
tests/test_gpu_weighting_matrix.py runs the tables on the device.

Compared quantities (every reference is computed in fp64 FROM THE SAME fp32 INPUTS the device reads, so what is left is fp32
summation and __expf):
  beta       the minimum of fp32 inputs: bit for bit
  eta        relative error
  N_j        |N_j - N_ref_j| / sum_k w_k |du_jk|  (records of routes B and C; the denominator in fp64)
  U, action  absolute error in units of |u_max| of the column
  S          relative error (the horizon route of B alone: S = sum_t gamma^t c_t + ctrl)

Tolerances are SIZED, not chosen: every class of rows is run through the fp32 restatement below (weights from an fp32 argument and
an fp32 exponential, sums sequential in fp32) and through the fp64 reference on identical inputs; the tolerance of the class is ten
times the largest deviation seen, rounded up to 1-2-5.  TOL holds (tolerance, measured fp32 deviation) per class and quantity;
tests/test_weighting_cases.py re-measures and refuses a table that has gone stale.  Caps: nothing above the end-to-end tolerances
(U, action 1e-3 |u_max|; eta 2e-3), nothing above a tenth of those except the rows of at least 4096 records and of more than
131072 samples (classes "big")."""
import dataclasses

import numpy as np

from mppiisaac.planner.mppi import make_config, savgol_matrix
from mppiisaac.utils.config_store import load_config
from scenes import build_scene

# ---- the geometry of combine_update, restated (csrc/mppi_kernels.hpp) ---------------------------------------------------------------
NT_UPDATE, NT_WORLD = 1024, 512          # kCombineThreads (k_combine, k_reduce_exchange), kCombineWorldThreads (k_combine_world)
MAX_SCALE = 4096                         # kMaxScale: entries of the weight table in LDS
FOLD_TABLE = 1024                        # kFoldTable: entries of fold_group's table
GROUPS, PART_FLOATS = 8, 8 * 64 * 12     # kCombineGroups, kPartFloats
WIDE_LOADS = {NT_UPDATE: 16, NT_WORLD: 24}


def combine_path(HN, nrec, NT):
    """which way combine_update<NT> takes for nrec records of 2 + HN floats"""
    Q = (HN + 3) // 4
    Gw = min(NT // Q, 32)
    part_capped = Gw * HN > PART_FLOATS
    if part_capped:
        Gw = PART_FLOATS // HN
    wide = Q <= NT and nrec <= MAX_SCALE and Gw >= 2
    G = Gw if wide else (min(NT // HN, GROUPS) if HN <= NT else 1)
    return dict(wide=wide, G=G, nvalid=HN - 4 * (Q - 1), part_capped=part_capped, second_pass=nrec > NT, recompute=nrec > MAX_SCALE,
                wide_tail=wide and nrec > WIDE_LOADS[NT] * G, rows_beyond_block=HN > NT)


# ---- contexts: the smallest scene that yields each H * nu ----------------------------------------------------------------------------
JACKAL_WHEELS = {"left_wheel_joints": ["front_left_wheel", "rear_left_wheel"], "right_wheel_joints": ["front_right_wheel", "rear_right_wheel"]}
ROBOTS = {"jackal": (["jackal", "goal"], [[0.0, 0.0, 0.1]], "jackal", JACKAL_WHEELS),          # nu = 2 (a contact scene: k_combine only)
          "point": (["point_robot", "goal"], [[0.0, 0.0, 0.05]], "pointbot", None),           # nu = 3
          "panda": (["panda_stick", "goal"], [[0.0, 0.0, 0.0]], "panda", None),               # nu = 7
          "omnipanda": (["omnipanda", "goal"], [[0.0, 0.0, 0.0]], "omnipanda", None)}         # nu = 12: the 12-command tree
SHAPES = {2: ("jackal", 1), 9: ("point", 3), 15: ("point", 5), 140: ("panda", 20), 448: ("panda", 64), 768: ("omnipanda", 64)}


@dataclasses.dataclass
class Shape:
    m: object
    cfg: object
    dof: np.ndarray
    root: np.ndarray
    umax: np.ndarray      # [H * nu]: |u_max| of every entry of the nominal
    lam: float            # the temperature of the robot's conf/mppi file


def make_shape(HN, K=16, **over):
    """model + MPPI config (conf/mppi/<robot>.yaml with K, H overridden) of the context that supplies (H, nu)"""
    robot, H = SHAPES[HN]
    actors, init, conf, rover = ROBOTS[robot]
    scene = build_scene(actors, init, robot_overrides=rover)
    ex = load_config({"defaults": [{"mppi": conf}, {"isaacgym": "normal"}]})
    ex.mppi.num_samples, ex.mppi.horizon, ex.mppi.use_priors, ex.mppi.sample_null_action = K, H, False, False
    for k, v in over.items():
        setattr(ex.mppi, k, v)
    cfg = make_config(ex.mppi)
    assert cfg.horizon * cfg.nu == HN
    dof, root = scene.initial_state()
    umax = np.tile([max(abs(cfg.u_max[j]), abs(cfg.u_min[j])) for j in range(cfg.nu)], H)
    return Shape(scene.to_c(), cfg, np.asarray(dof, np.float32), np.asarray(root, np.float32), umax, float(cfg.lambda_))


def nominal(shape):
    """a non-zero nominal, a quarter of the control range in size"""
    H, nu = shape.cfg.horizon, shape.cfg.nu
    U = 0.25 * shape.umax.reshape(H, nu) * np.random.default_rng(0).normal(size=(H, nu))
    return np.where(np.abs(U) < 1e-3 * shape.umax.reshape(H, nu), 1e-3 * shape.umax.reshape(H, nu), U).astype(np.float32)


# ---- the reference: fp64, plain numpy -------------------------------------------------------------------------------------------------
def record64(S, du, lam):
    """[beta, eta, N] of the samples S [K] (fp32 values), du [HN][K]: a sample whose cost is not finite has weight 0.
    -> (beta, eta, N [HN], w [K], scale [HN] = sum_k w_k |du_jk|)"""
    S, du = np.asarray(S, np.float64), np.asarray(du, np.float64).reshape(-1, len(S))
    fin = np.isfinite(S)
    if not fin.any():
        return np.inf, 0.0, np.zeros(du.shape[0]), np.zeros(len(S)), np.zeros(du.shape[0])
    beta = S[fin].min()
    w = np.zeros(len(S))
    w[fin] = np.exp(-(S[fin] - beta) / lam)
    duf = du[:, fin]
    return beta, w.sum(), duf @ w[fin], w, np.abs(duf) @ w[fin]


def combine64(recs, lam):
    """records [n][2 + HN] (fp32 values) -> (beta, eta, N, w [n]): a record with eta == 0 is skipped, its beta and its N included"""
    r = np.asarray(recs, np.float64)
    live = r[:, 1] > 0
    if not live.any():
        return np.inf, 0.0, np.zeros(r.shape[1] - 2), np.zeros(len(r))
    beta = r[live, 0].min()
    w = np.zeros(len(r))
    w[live] = np.exp(-(r[live, 0] - beta) / lam) * r[live, 1]
    sc = np.exp(-(r[live, 0] - beta) / lam)
    return beta, w.sum(), sc @ r[live, 2:], w


def finish64(U0, beta, eta, N, u_init, F=None):
    """U += N / eta (nothing when eta == 0), filter, action = first row, shift, append u_init"""
    U = np.asarray(U0, np.float64).copy()
    H, nu = U.shape
    if eta > 0:
        U = U + N.reshape(H, nu) / eta
    if F is not None:
        U = np.asarray(F, np.float64) @ U
    out = np.vstack([U[1:], np.full((1, nu), float(np.float32(u_init)))])
    return {"U": out, "action": U[0].copy(), "beta": beta, "eta": eta}


def update64(recs, U0, lam, u_init=0.0, F=None):
    beta, eta, N, w = combine64(recs, lam)
    out = finish64(U0, beta, eta, N, u_init, F)
    out["w"] = w
    return out


# ---- the same in fp32, sequentially: what sizes the tolerances -------------------------------------------------------------------------
f32 = np.float32


def _weights32(b, beta, lam):
    """exp(-(b - beta) * (1 / lambda)) with an fp32 argument, an fp32 reciprocal and the fp32 exponential the way __expf takes it:
    exp2 of the argument times log2(e), the product rounded to fp32"""
    inv = f32(1.0 / lam)
    with np.errstate(under="ignore"):
        arg = (-(b.astype(f32) - f32(beta)) * inv).astype(f32)
        return np.exp2((arg * f32(1.4426950408889634)).astype(f32)).astype(f32)


def record32(S, du, lam):
    S, du = np.asarray(S, f32), np.asarray(du, f32).reshape(-1, len(S))
    fin = np.isfinite(S)
    if not fin.any():
        return np.inf, 0.0, np.zeros(du.shape[0])
    beta = S[fin].min()
    w = _weights32(S[fin], beta, lam)
    eta, N, cols = f32(0), np.zeros(du.shape[0], f32), np.ascontiguousarray(du[:, fin].T)
    for wk, col in zip(w, cols):
        eta = f32(eta + wk)
        N = (N + wk * col).astype(f32)
    return float(beta), float(eta), N.astype(np.float64)


def update32(recs, U0, lam, u_init=0.0, F=None):
    r = np.asarray(recs, f32)
    live = r[:, 1] > 0
    U = np.asarray(U0, f32).copy()
    H, nu = U.shape
    beta, eta = np.inf, f32(0)
    if live.any():
        beta = r[live, 0].min()
        sc = _weights32(r[live, 0], beta, lam)
        N = np.zeros(r.shape[1] - 2, f32)
        for e, s, row in zip(r[live, 1], sc, r[live, 2:]):
            eta = f32(eta + e * s)
            N = (N + row * s).astype(f32)
        U = (U + (N / eta).reshape(H, nu)).astype(f32)
    if F is not None:
        Ff, V = np.asarray(F, f32), np.zeros_like(U)
        for s in range(H):
            V = (V + Ff[:, s:s + 1] * U[s:s + 1, :]).astype(f32)
        U = V
    out = np.vstack([U[1:], np.full((1, nu), f32(u_init))])
    return {"U": out.astype(np.float64), "action": U[0].astype(np.float64), "beta": float(beta), "eta": float(eta)}


def deviation(got, want, umax):
    """-> {"eta": relative, "U": max over nominal and action in units of |u_max|} of two update results"""
    nu = len(want["action"])
    eta = abs(got["eta"] - want["eta"]) / want["eta"] if want["eta"] > 0 else abs(got["eta"])
    u = max(np.max(np.abs(got["U"] - want["U"]) / umax.reshape(-1, nu)), np.max(np.abs(got["action"] - want["action"]) / umax[:nu]))
    return {"eta": float(eta), "U": float(u)}


def record_deviation(got, want):
    """(beta, eta, N) against record64's tuple -> {"eta": relative, "N": max_j |N_j - ref_j| / sum_k w_k |du_jk|}"""
    beta, eta, N, w, scale = want
    return {"eta": abs(got[1] - eta) / eta, "N": float(np.max(np.abs(np.asarray(got[2], np.float64) - N) / scale))}


def round125(x):
    """x rounded up to 1, 2 or 5 times a power of ten"""
    e = np.floor(np.log10(x))
    for m in (1.0, 2.0, 5.0, 10.0):
        if x <= m * 10.0 ** e * (1 + 1e-12):
            return float(f"{m * 10.0 ** e:.0e}")


def ess(w):
    """effective number of samples (records) of the weights w: 1 / sum (w / eta)^2"""
    w = np.asarray(w, np.float64)
    return float(w.sum() ** 2 / np.sum(w ** 2)) if w.sum() > 0 else 0.0


# ---- route A: synthetic records into the combine ---------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Row:
    name: str
    HN: int
    nrec: int
    cls: str                 # a spread | b boundary | c wide | d- negative | d+ 1e6 | e eta = 0 | f eta = 0 non-finite | g all eta = 0
    why: str                 # the branch of combine_update this row is for
    world: bool = False      # through mppi_update_step_world with a K = 1 world (combine_update<512>), else mppi_update (<1024>)
    bounds: tuple = (0, -1)  # records named as boundaries: they carry weight, and leaving one out must move an output
    min_at: int = None       # class b: the record that holds the minimum beta
    spread: float = 3.0      # class a: the betas are spread over this many lambda
    filt: bool = False       # (h) mppi_set_filter with savgol_matrix(H)
    u_init: float = 0.0      # (i)
    lam_scale: tuple = ()    # mppi_set_lambda(scale * configured) before each of several updates on ONE context

    @property
    def NT(self):
        return NT_WORLD if self.world else NT_UPDATE

    @property
    def big(self):
        return self.nrec >= MAX_SCALE

    @property
    def degenerate(self):
        """fewer than four live records cannot have an effective record count of four; all-rejected has none"""
        return self.nrec < 4 or self.cls == "g"

    @property
    def tol(self):
        return {q: TOL[self.cls[0] + ("-big" if self.big else "")][q][0] for q in ("eta", "U")}


SMALL = dict(spread=0.5)     # up to nine records: nearly equal weights, so that four of them are effective
ROWS = [
    # (a) betas spread over a few lambda
    Row("a-HN2-n1", 2, 1, "a", "one record; nvalid 2 in the last quad", bounds=(0,)),
    Row("a-HN9-n2", 9, 2, "a", "nvalid 1 in the last quad", **SMALL),
    Row("a-HN15-n7", 15, 7, "a", "nvalid 3 in the last quad", **SMALL),
    Row("a-HN140-n8", 140, 8, "a", "the workload's shape: eight folded records; nvalid 4", **SMALL),
    Row("a-HN448-n9", 448, 9, "a", "nrec < kWideLoads G: the up-front loads alone", **SMALL),
    Row("a-HN768-n9", 768, 9, "a", "HN = MPPI_MAX_H MPPI_MAX_NU: Gw = 5, Gw HN = 3840 < kPartFloats", **SMALL),
    Row("a-HN768-n1023", 768, 1023, "a", "nrec > kWideLoads G = 80: the wide tail loop; nrec < NT"),
    Row("a-HN140-n1024", 140, 1024, "a", "nrec = NT: every record in the registers of the first pass"),
    Row("a-HN140-n1025", 140, 1025, "a", "nrec > NT: the second trip of both passes", bounds=(0, 1023, 1024)),
    Row("a-HN15-n4095", 15, 4095, "a", "nrec < kMaxScale, ragged quad, Gw = 32"),
    Row("a-HN140-n4096", 140, 4096, "a", "nrec = kMaxScale: the last wide count", bounds=(0, 4095)),
    Row("a-HN140-n4097", 140, 4097, "a", "nrec > kMaxScale: narrow path, G = 7, the factor of record 4096 recomputed", bounds=(0, 4095, 4096)),
    Row("a-HN768-n5000", 768, 5000, "a", "narrow path, G = 1", bounds=(0, 4095, 4096, -1)),
    Row("a-HN2-n5000", 2, 5000, "a", "narrow path, G = 8", bounds=(0, 4096, -1)),
    # (b) the minimum beta in a boundary record, the weight concentrated in the boundary records
    Row("b-HN140-n1024-min1023", 140, 1024, "b", "minimum in record NT - 1, the last", bounds=(0, 1, 2, 1023), min_at=1023),
    Row("b-HN140-n1025-min1024", 140, 1025, "b", "minimum in record NT, the last: found by the second trip alone", bounds=(0, 1, 1023, 1024), min_at=1024),
    Row("b-HN140-n4096-min4095", 140, 4096, "b", "minimum in record kMaxScale - 1, the last", bounds=(0, 1023, 1024, 4095), min_at=4095),
    Row("b-HN140-n4097-min4096", 140, 4097, "b", "minimum in record kMaxScale, the last: its factor is recomputed", bounds=(0, 1024, 4095, 4096), min_at=4096),
    Row("b-HN15-n5000-min4999", 15, 5000, "b", "minimum in the last record, beyond the table", bounds=(0, 4095, 4096, 4999), min_at=4999),
    # (c) betas spread over 200 lambda: most factors underflow, some are denormal
    Row("c-HN140-n1024", 140, 1024, "c", "underflowing factors, wide path", spread=200.0),
    Row("c-HN15-n4097", 15, 4097, "c", "underflowing factors, narrow path and the recomputed factor", spread=200.0),
    # (d) negative betas; betas of 1e6 with differences of order lambda
    Row("d-HN140-n1025", 140, 1025, "d-", "negative betas"),
    Row("d-HN448-n1023", 448, 1023, "d+", "betas of 1e6"),
    # (e) every third record has eta = 0, finite N, beta below the live minimum: ignored, beta included
    Row("e-HN140-n9", 140, 9, "e", "skipped records among the up-front loads", **SMALL),
    Row("e-HN15-n1025", 15, 1025, "e", "skipped records in both trips of the passes"),
    Row("e-HN140-n4097", 140, 4097, "e", "skipped records on the narrow path", bounds=(0, 4095, 4096)),
    # (f) as (e) with NaN / +-Inf in N and beta of the skipped records: a finite update over the live ones
    Row("f-HN15-n8", 15, 8, "f", "non-finite skipped records, ragged quad", **SMALL),
    Row("f-HN140-n9", 140, 9, "f", "non-finite skipped records among the up-front loads", **SMALL),
    Row("f-HN768-n1023", 768, 1023, "f", "non-finite skipped records in the wide tail loop"),
    Row("f-HN140-n4097", 140, 4097, "f", "non-finite skipped records on the narrow path", bounds=(0, 4095, 4096)),
    # (g) every record eta = 0: the nominal kept and shifted, u_init appended, the action the old first row
    Row("g-HN140-n8", 140, 8, "g", "all rejected, wide path", u_init=0.05),
    Row("g-HN9-n4097", 9, 4097, "g", "all rejected, narrow path", u_init=0.3),
    # (h) filter on
    Row("h-HN140-n9", 140, 9, "a", "mode 1 with the filter, H = 20", filt=True, **SMALL),
    Row("h-HN15-n7", 15, 7, "a", "mode 1 with the filter, H = 5 (window 5)", filt=True, **SMALL),
    # (i) u_init
    Row("i-HN140-n8", 140, 8, "a", "u_init = 0.1 appended", u_init=0.1, **SMALL),
    # lambda changed by mppi_set_lambda between two updates on one context
    Row("l-HN140-n9", 140, 9, "a", "mppi_set_lambda: 1e-2 and 1e2 times the configured temperature", lam_scale=(1e-2, 1e2), spread=0.5),
    # combine_update<512> behind k_combine_world
    Row("w-HN140-n9", 140, 9, "a", "NT = 512: HN < NT, Gw = 14", world=True, **SMALL),
    Row("w-HN140-n1023", 140, 1023, "a", "NT = 512: nrec > NT, nrec > kWideLoads G = 336", world=True, bounds=(0, 511, 512, -1)),
    Row("w-HN448-n1025", 448, 1025, "a", "NT = 512: Gw = 4, wide tail loop", world=True, bounds=(0, 511, 512, -1)),
    Row("w-HN768-n9", 768, 9, "a", "NT = 512: HN = 768 > NT, wide with Gw = 2", world=True, **SMALL),
    Row("w-HN768-n4097", 768, 4097, "a", "NT = 512: HN > NT on the narrow path, G = 1, two trips over the rows", world=True, bounds=(0, 4095, 4096)),
    Row("w-f-HN448-n9", 448, 9, "f", "NT = 512: non-finite skipped records", world=True, **SMALL),
    Row("w-h-HN140-n9", 140, 9, "a", "NT = 512: the filter", world=True, filt=True, **SMALL),
]
ROW_IDS = [r.name for r in ROWS]

# (tolerance, largest deviation of the sequential fp32 restatement from the fp64 reference over the rows of the class); "-big": the
# rows of at least kMaxScale records.  tolerance = round125(10 * deviation)
TOL = {
    "a": {"eta": (1e-05, 5.3e-07), "U": (1e-06, 7.0e-08)},
    "a-big": {"eta": (2e-05, 1.1e-06), "U": (5e-07, 5.0e-08)},
    "b": {"eta": (1e-06, 9.3e-08), "U": (1e-06, 8.5e-08)},
    "b-big": {"eta": (2e-05, 1.6e-06), "U": (1e-06, 6.3e-08)},
    "c": {"eta": (5e-06, 2.3e-07), "U": (2e-06, 1.6e-07)},
    "c-big": {"eta": (5e-06, 2.9e-07), "U": (2e-06, 1.3e-07)},
    "d": {"eta": (5e-06, 5.0e-07), "U": (5e-07, 4.9e-08)},
    "e": {"eta": (1e-06, 6.7e-08), "U": (5e-07, 4.0e-08)},
    "e-big": {"eta": (1e-05, 5.1e-07), "U": (5e-07, 3.6e-08)},
    "f": {"eta": (5e-06, 3.1e-07), "U": (1e-06, 5.5e-08)},
    "f-big": {"eta": (1e-05, 9.9e-07), "U": (5e-07, 3.1e-08)},
    "g": {"eta": (0.0, 0.0), "U": (0.0, 0.0)},          # nothing is summed: the kept nominal is compared for equality
    "g-big": {"eta": (0.0, 0.0), "U": (0.0, 0.0)},
}
CAP = {"eta": 2e-3, "U": 1e-3}                            # the end-to-end tolerances; a tenth of them for every class that is not "-big"


def row_lambda(row, shape):
    return [shape.lam * s for s in row.lam_scale] or [shape.lam]


def make_records(row, shape, lam=None):
    """-> (records [nrec][2 + HN] float32, the same with the eta = 0 records finite - row (f)'s twin, else the records themselves)"""
    lam = shape.lam if lam is None else lam
    rng = np.random.default_rng(1 + ROW_IDS.index(row.name))
    n, HN = row.nrec, row.HN
    bounds = sorted({b % n for b in row.bounds})
    base = {"d-": -300.0, "d+": 1.0e6}.get(row.cls, 50.0)
    if row.cls == "b":
        beta = base + lam * rng.uniform(3.0, 6.0, n)
        beta[bounds] = base + lam * rng.uniform(0.25, 0.5, len(bounds))
        beta[row.min_at] = base
    else:
        beta = base + lam * rng.uniform(0.0, row.spread, n)
        beta[bounds] = base - (1.0 if n >= 1000 else 0.0) * lam - lam * 0.01 * np.arange(len(bounds))
    eta = rng.uniform(6.0, 10.0, n)
    N = eta[:, None] * 0.3 * shape.umax[None, :] * rng.normal(size=(n, HN))
    recs = np.concatenate([beta[:, None], eta[:, None], N], axis=1).astype(np.float32)
    twin = recs
    if row.cls in ("e", "f", "g"):
        dead = np.ones(n, bool) if row.cls == "g" else (np.arange(n) % 3 == 1) & ~np.isin(np.arange(n), bounds)
        recs[dead, 0] = np.float32(base - 5.0 * lam)
        recs[dead, 1] = 0.0
        recs[dead, 2:] *= 100.0
        twin = recs.copy()
        if row.cls == "f":
            bad = np.array([np.nan, np.inf, -np.inf, 1.0], np.float32)
            idx = np.flatnonzero(dead)
            pos = np.arange(len(idx))
            recs[idx, 0] = np.where(np.isfinite(bad[pos % 4]), recs[idx, 0], bad[pos % 4])
            for i, r in enumerate(idx):
                cols = 2 + (np.arange(HN)[(np.arange(HN) + i) % 2 == 0] if i % 3 else np.arange(HN))
                recs[r, cols] = bad[(cols + i) % 3]
    return recs, twin


# ---- route B: injected costs into the record kernels -----------------------------------------------------------------------------------
B_K = (1, 15, 16, 17, 63, 64, 65, 100, 102, 1024)
B_COSTS = ("spread", "equal", "min-last", "min-tail-first", "wide", "negative", "big", "planted")
# path -> (MPPI_ROLLOUT, entry point, rollout_var_discount): the record kernel that serves it
B_PATHS = {"accumulate": (None, "k_reduce_quad", 1.0), "accumulate-lane": ("lane", "k_reduce", 1.0),
           "horizon": (None, "k_horizon_reduce_quad", 1.0), "horizon-0.9": (None, "k_horizon_reduce_quad", 0.9)}
B_LAMBDA = 5.0    # the point robot's temperature in tests/test_gpu_rollout_matrix.py
B_H = 5           # point robot, H * nu = 15 rows: no multiple of four
B_BOUNDS = lambda K: sorted({0, 16 * ((K - 1) // 16), K - 1})   # first sample, first and last live sample of the tail group


def b_du(K, umax=1.5):
    """a stand-in for the perturbations of a rollout [B_H * 3][K], some at the clamp (the conditions are checked on it; the device
    weights its own)"""
    rng = np.random.default_rng(7)
    U0 = 0.25 * umax * rng.normal(size=(B_H * 3, 1))
    return (np.clip(U0 + rng.normal(size=(B_H * 3, K)), -umax, umax) - U0).astype(np.float32)
TOL_B = {"eta": (5e-6, 4.8e-7), "N": (5e-6, 3.4e-7), "U": (2e-6, 1.5e-7), "S": (2e-6, 2.0e-7)}


def planted(K):
    """the pattern of tests/test_gpu_rollout_matrix.py: non-finite values at the first and the last sample, a whole group of 16, a
    whole wavefront of 64 (as far as K reaches)"""
    v = np.zeros(K, np.float32)
    v[0], v[K - 1] = np.nan, np.inf
    v[16:32] = np.inf
    v[64:128] = np.where(np.arange(64) % 3 == 0, np.nan, -np.inf)[:max(0, min(K, 128) - 64)]
    if K > 40:
        v[40] = -np.inf
    return v


def make_costs(kind, K, lam):
    """a cost vector S [K] float32 of route B"""
    rng = np.random.default_rng(100 + B_COSTS.index(kind))
    tail0 = 16 * ((K - 1) // 16)               # the first sample of the last group of 16
    S = 50.0 + lam * rng.uniform(0.0, 3.0, K)
    if kind == "equal":
        S[:] = 50.0
    elif kind == "min-last":
        S[K - 1] = 50.0 - lam
    elif kind == "min-tail-first":
        S[tail0] = 50.0 - lam
    elif kind == "wide":
        S = 50.0 + lam * np.where(np.arange(K) % 2 == 0, rng.uniform(0.0, 2.0, K), rng.uniform(0.0, 200.0, K))
        S[[0, tail0, K - 1]] = 50.0 - 0.1 * lam * np.arange(3)
    elif kind == "negative":
        S = S - 400.0
    elif kind == "big":
        S = S + 1.0e6
    S = S.astype(np.float32)
    if kind == "planted" and K >= 8:
        S = S + planted(K)
        S[[3, min(K - 2, 33)]] = np.float32(50.0)   # (live samples next to the rejected ones)
    return S


def stage_costs(S, H, gamma):
    """c [H][K] float32 with sum_t gamma^t c_t close to S (the horizon route: the device's own fp32 sum is what is weighted)"""
    t = np.arange(H, dtype=np.float64)
    a = 1.0 + 0.5 * np.cos(t)
    share = (a / a.sum() / float(gamma) ** t)[:, None]
    c = (share * np.where(np.isfinite(S), S, 0.0).astype(np.float64)[None, :]).astype(np.float32)
    c[H // 2, ~np.isfinite(S)] = S[~np.isfinite(S)]
    return c


def horizon_sum64(c, gamma, S0=None, ctrl=None):
    c = np.asarray(c, np.float64)
    acc = ((float(gamma) ** np.arange(c.shape[0]))[:, None] * c).sum(0)
    return (0.0 if S0 is None else np.asarray(S0, np.float64)) + acc + (0.0 if ctrl is None else np.asarray(ctrl, np.float64))


def horizon_sum32(c, gamma):
    c = np.asarray(c, f32)
    acc, disc, g = np.zeros(c.shape[1], f32), f32(1), f32(gamma)
    for t in range(c.shape[0]):
        acc = (disc * c[t] + acc).astype(f32)
        disc = f32(disc * g)
    return acc


# ---- route C: the fused kernels' own records and the fold --------------------------------------------------------------------------------
C_KERNELS = ("lane", "quad", "oct", "oct-pair")
C_LAMBDA = 20.0


def c_nominal(cfg):
    umax = max(abs(cfg.u_max[0]), abs(cfg.u_min[0]))
    return (0.05 * umax * np.random.default_rng(0).normal(size=(cfg.horizon, cfg.nu))).astype(np.float32)
C_K, C_H = (16, 17, 200, 256), (1, 10)
# fold_group's table holds kFoldTable = 1024 wave records per group: just over it in each of eight groups (the record count a multiple
# of 16), and over it in ONE group (not a multiple of 16) - point robot, H = 2, quad kernel, MPPI_FOLD=1
C_FOLD_TABLE = {"eight-groups": 16 * 8 * (FOLD_TABLE + 8), "one-group": 16 * (FOLD_TABLE + 9)}
TOL_C = {"eta": (5e-6, 4.4e-7), "N": (1e-6, 9.8e-8)}
TOL_C_BIG = {"eta": (5e-5, 2.8e-6), "N": (5e-6, 3.0e-7)}


def fold_groups(K, n_groups):
    """sample ranges of the folded records: group g owns the wave records [g n, (g + 1) n) of 16 samples each"""
    nw = (K + 15) // 16
    if n_groups == 1:
        return [(0, K)]
    assert nw % n_groups == 0
    n = nw // n_groups
    return [(16 * g * n, min(K, 16 * (g + 1) * n)) for g in range(n_groups)]
