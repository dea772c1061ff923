"""The contact-free octet rollout with helper wavefronts (k_rollout_oct_pair, csrc/mppi_oct_pair.hpp) against the octet kernel
without helpers (MPPI_ROLLOUT=oct) on the same state: the helpers issue the same operations on the same values in the same order,
so costs, visualisation rows, perturbations and the update (beta, eta, U, action) are compared for EQUALITY, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from mppiisaac.backend import capi
from scenes import panda_reach, point_reach

pytestmark = pytest.mark.gpu


def kernel_info(lib, ctx):
    buf = C.create_string_buffer(512)
    capi.check(lib, lib.mppi_kernel_info(ctx, buf, 512))
    return dict(kv.split("=", 1) for kv in buf.value.decode().split())


def iteration(lib, make, K, H, null):
    """sample, rollout, reduce and update of one fresh context at a non-zero nominal plan; everything the iteration computed"""
    scene, m, cfg, cost, dof, root = make(K=K, H=H, sample_null_action=null)
    ctx = C.c_void_p()
    capi.check(lib, lib.mppi_create(C.byref(m), C.byref(cfg), 0, C.byref(ctx)))

    def call(name, *args):
        capi.check(lib, getattr(lib, name)(ctx, *args))

    def get(name, shape):
        out = np.zeros(shape, np.float32)
        call(name, capi.fptr(out))
        return out

    call("mppi_set_cost", C.byref(cost))
    info = kernel_info(lib, ctx)
    call("mppi_sample", C.c_uint32(0))                                       # (the configuration's halton set)
    d, r = np.ascontiguousarray(dof, np.float32), np.ascontiguousarray(root, np.float32)
    call("mppi_set_state", capi.fptr(d), capi.fptr(r))
    U0 = (0.05 * np.random.default_rng(0).normal(size=(H, cfg.nu))).astype(np.float32)
    call("mppi_set_nominal", capi.fptr(U0))
    call("mppi_rollout")
    out = {"S": get("mppi_get_costs", (K,)), "du": get("mppi_get_perturbations", (H, cfg.nu, K))}
    if cfg.want_rollouts:
        out["viz"] = get("mppi_get_rollouts", (H, K, 3))
    call("mppi_reduce", None)
    call("mppi_update", None, 1)
    out["beta_eta"] = get("mppi_get_weights_stats", (2,))
    out["U"] = get("mppi_get_nominal", (H, cfg.nu))
    out["action"] = get("mppi_get_action", (cfg.nu,))
    lib.mppi_destroy(ctx)
    return info, out


@pytest.mark.parametrize("null", [True, False])
@pytest.mark.parametrize("make,K,H", [(panda_reach, 4096, 20), (panda_reach, 1000, 20), (panda_reach, 24, 20), (point_reach, 77, 15),
                                      (point_reach, 1024, 15)])
def test_helper_kernel_equals_the_octet_kernel_bit_for_bit(make, K, H, null, monkeypatch):
    assert torch.cuda.is_available()
    lib = capi.load_library()
    monkeypatch.delenv("MPPI_ROLLOUT", raising=False)
    info_new, new = iteration(lib, make, K, H, null)
    monkeypatch.setenv("MPPI_ROLLOUT", "oct")
    info_old, old = iteration(lib, make, K, H, null)
    # the two runs really used the two kernels
    assert info_new["rollout"] == "oct-pair" and int(info_new["waves"]) == 4 * ((K + 15) // 16), info_new
    assert info_old["rollout"] == "oct" and int(info_old["waves"]) == 2 * ((K + 15) // 16), info_old
    assert np.isfinite(old["S"]).all() and sorted(new) == sorted(old)
    for name in sorted(old):
        diff = np.abs(new[name].astype(np.float64) - old[name])
        print(f"{make.__name__} K={K} null={null} {name}: max abs difference {diff.max():.3e}")
    for name in sorted(old):
        np.testing.assert_array_equal(new[name], old[name], err_msg=name)


def test_more_samples_than_workgroups_fit_keep_the_kernel_without_helpers(monkeypatch):
    """four wavefronts of more than 256 registers need a CU to themselves: K = 8192 is 512 workgroups on 256 CUs"""
    lib = capi.load_library()
    monkeypatch.delenv("MPPI_ROLLOUT", raising=False)
    scene, m, cfg, cost, dof, root = panda_reach(K=8192, H=20)
    ctx = C.c_void_p()
    capi.check(lib, lib.mppi_create(C.byref(m), C.byref(cfg), 0, C.byref(ctx)))
    info = kernel_info(lib, ctx)
    lib.mppi_destroy(ctx)
    assert info["rollout"] == "oct" and int(info["waves"]) == 1024, info
