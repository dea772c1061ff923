"""Per-env state entry points of the batched simulator (mppi_sim_set_states, mppi_sim_set_states_indexed, mppi_sim_reset_indexed),
the part that needs no GPU: the symbols exist in the header, the built library and the binding, and the inputs of
test_gpu_per_env_states.py are well posed ON THE ORACLE ALONE - a pass there means something:
  * everything finite;
  * the fp32 oracle within a TENTH of every tolerance of test_gpu_step_matrix.TOL, on every env at every step (a condition on the
    inputs: the seeds of per_env_states.py are chosen by this test, the tolerances are not touched);
  * every env told apart from its neighbour and from env 0 by more than 100 x a tolerance (an index mix-up cannot pass);
  * the START states differ between envs in the dof rows, in every moving base row and in every free actor row, so that q_, qd_,
    base_ and fr_ are each exercised; quaternions are unit; the rows that are not per env are the shared ones in every env."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mppiisaac.backend import capi
from per_env_states import (INDEXED, KMAX, SCENES, SEED_OTHER, STEP_CASES, STEP_IDS, mixed_starts, per_env_actors, reference, reference_mixed,
                            scene_case, starts, touched)
from test_gpu_step_matrix import KEYS, TOL, deviations, told_apart

NEW = ("mppi_sim_set_states", "mppi_sim_set_states_indexed", "mppi_sim_reset_indexed")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "mppi_hip.h")).read()
    lib = C.CDLL(capi.LIB_PATH)          # (loads without a GPU)
    for name in NEW:
        assert re.search(r"^int " + name + r"\(mppi_ctx_t \*ctx,", header, re.M), f"{name} is not declared in mppi_hip.h"
        assert name in capi.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "#define MPPI_ABI_VERSION 9" in header and capi.ABI_VERSION == 9
    for name in NEW:                     # a NULL context is refused before anything is touched
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = capi._SIGNATURES[name]
    assert lib.mppi_sim_set_states(None, None, None) < 0
    assert lib.mppi_sim_set_states_indexed(None, None, 0, None, None) < 0
    assert lib.mppi_sim_reset_indexed(None, None, 0) < 0


@pytest.mark.parametrize("scene", SCENES)
def test_starts_differ_in_every_per_env_row(scene):
    for seed in (None, SEED_OTHER):
        b, dof, root = starts(scene) if seed is None else starts(scene, seed)
        m = b.m
        assert dof.shape == (KMAX, 2 * m.n_bodies) and root.shape == (KMAX, m.n_actors, 13) and dof.dtype == root.dtype == np.float32
        assert np.isfinite(dof).all() and np.isfinite(root).all()
        np.testing.assert_allclose(np.linalg.norm(root[:, :, 3:7].astype(np.float64), axis=-1), 1.0, atol=2e-7)
        mine = per_env_actors(m)
        assert len(mine) == {"panda": 0, "boxer": 2, "jackals": 2, "pick": 1}[scene], mine     # base + block; two bases; the block
        for a in range(m.n_actors):
            if a not in mine:
                assert (root[:, a] == b.root.reshape(m.n_actors, 13)[a]).all(), f"actor {a} is shared by the envs"
        for k in range(1, KMAX):
            for j in (k - 1, 0):
                assert (dof[k] != dof[j]).any(), (k, j)
                for a in mine:
                    assert (root[k, a] != root[j, a]).any(), (k, j, a)
    if scene in ("panda", "boxer"):     # the second set differs from the first where an indexed call writes it
        for K in (65, 80):
            ids, dofm, rootm = mixed_starts(scene, K)
            assert sorted(ids) == sorted({0, 15, 16, 63, 64, K - 1}) and ids != sorted(ids) and ids == touched(K)
            _, dof, root = starts(scene)
            for k in range(K):
                assert (dofm[k] != dof[k]).any() == (k in ids)
                for a in per_env_actors(starts(scene)[0].m):
                    assert (rootm[k, a] != root[k, a]).any() == (k in ids)


def well_posed(tag, r64, r32, klass, K):
    assert all(np.isfinite(v).all() for v in r64.values()) and all(np.isfinite(v).all() for v in r32.values())
    dev = deviations(r32, r64)
    print(f"{tag}: fp32 oracle vs fp64 oracle: " + " | ".join(f"{k} {dev[k].max():.1e} (tol/10 {TOL[klass][k] / 10:.0e})" for k in KEYS)
          + f" | worst share of TOL {max(dev[k].max() / TOL[klass][k] for k in KEYS if TOL[klass][k] > 0):.3f}")
    for k in KEYS:
        assert dev[k].max() <= TOL[klass][k] / 10.0, f"{tag}: {k}: the fp32 oracle leaves the fp64 one by more than a tenth of the tolerance"
    for k in range(1, K):
        assert told_apart(r64, klass, k, k - 1) and told_apart(r64, klass, k, 0), f"{tag}: env {k} is not told apart from env {k - 1} / env 0"


@pytest.mark.parametrize("case", STEP_CASES, ids=STEP_IDS)
def test_step_cases_from_per_env_starts_are_well_posed(case, oracle64, oracle32):
    assert STEP_IDS.count(case.name) == 1 and case.K <= KMAX and case.N == scene_case(case.scene).N
    well_posed(case.name, reference(oracle64, case.scene, case.K), reference(oracle32, case.scene, case.K), case.klass, case.K)


@pytest.mark.parametrize("scene,K", INDEXED)
def test_indexed_cases_are_well_posed(scene, K, oracle64, oracle32):
    r64, base = reference_mixed(oracle64, scene, K), reference(oracle64, scene, K)
    well_posed(f"{scene}-K{K}-indexed", r64, reference_mixed(oracle32, scene, K), scene_case(scene).klass, K)
    for k in touched(K):                 # what the indexed call wrote shows: a call that wrote nothing cannot pass
        both = {key: np.concatenate([r64[key][:, k:k + 1], base[key][:, k:k + 1]], axis=1) for key in r64}
        assert told_apart(both, scene_case(scene).klass, 0, 1), f"env {k}: the second start is not told apart from the first"
