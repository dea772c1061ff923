"""The octet rollout kernels (MPPI_ROLLOUT=oct-pair, =oct and the trajectory dump) against fixtures recorded from the build that
held every per-joint scalar replicated over the eight lanes of a sample (tools/make_lane_scalar_golden.py,
tests/golden/lane_scalars): with the scalars one joint per lane the same operations meet the same operands, so costs,
perturbations, visualisation rows, the update and every q / qd of the dump are compared for EQUALITY of their bit patterns.

The cases (tests/lane_scalar_cases.py) are the smallest in which that form can go wrong.  On the all-revolute arm (panda_stick:
seven joints, two vectors, one pad lane - the instantiation that holds its scalars one joint per lane): K = 24 (a second owner
wavefront whose upper samples do not exist) with H = 3 and K = 16 with H = 1 (table rows t + 2 past the horizon); the same arm
with a five-command mixed map (targets formed per lane from the lane's own row of the map) and with the point cost (q0, q1
replicated out of a joint vector for the hand-over and the stage cost).  Trees with prismatic joints keep the replicated form
(the generic instantiation): nine bodies with two prismatic fingers on a branch (panda_gripper) and three prismatic / revolute
bodies with the point cost (point_robot) show that it computes what it did.  Every case holds a joint at its stop, velocities
clamped at vmax and the saturated second solve in every owner wavefront (the recording script refuses a fixture otherwise;
test_fixtures_hold_every_path re-reads the first two from the fixtures, without a GPU)."""
import os

import numpy as np
import pytest

import lane_scalar_cases as L
from mppiisaac.backend import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lane_scalars")


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {kernel: {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(kernel + ".")} for kernel in L.KERNELS}


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return capi.load_library()


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_fixtures_hold_every_path(name):
    make, K, H = L.CASES[name]
    scene, m, cfg, cost, dof, root = make(K, H)
    for kernel, want in fixture(name).items():
        assert want["S"].dtype == np.uint32 and want["S"].shape == (K,) and want["dump_dof"].shape == (H, K, 2 * m.n_bodies)
        q, qd = L.dump_q_qd(want["dump_dof"].view(np.float32))
        stops, clamps = L.path_counts(m, q, qd)
        assert stops > 0 and clamps > 0, (name, kernel, stops, clamps)
        assert ("viz" in want) == bool(cfg.want_rollouts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(L.CASES))
def test_octet_kernels_reproduce_the_recorded_bits(name, lib):
    make, K, H = L.CASES[name]
    golden, runs = fixture(name), {}
    for kernel in L.KERNELS:
        info, got = L.run_gpu(lib, make, K, H, kernel)
        assert info["rollout"] == kernel and int(info["waves"]) == (4 if kernel == "oct-pair" else 2) * ((K + 15) // 16), info
        runs[kernel] = got
        want = golden[kernel]
        assert sorted(got) == sorted(want)
        for key in sorted(want):
            differ = int((got[key].view(np.uint32) != want[key]).sum())
            print(f"{name} {kernel} {key}: {differ} of {want[key].size} values differ from the fixture")
        for key in sorted(want):
            np.testing.assert_array_equal(got[key].view(np.uint32), want[key], err_msg=f"{name} {kernel}: {key}")
    # the eight lanes' copies of every broadcast scalar agree: the kernel with helpers and the one without store from different lanes
    for key in runs["oct"]:
        np.testing.assert_array_equal(runs["oct-pair"][key].view(np.uint32), runs["oct"][key].view(np.uint32), err_msg=f"{name}: oct-pair vs oct, {key}")
