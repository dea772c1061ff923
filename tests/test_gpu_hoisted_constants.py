"""The octet rollout kernels (MPPI_ROLLOUT=oct-pair, =oct and the trajectory dump) against fixtures recorded from the build that
read the drive mode, (h, kd), `substeps`, the gravity flag and the link bodies from the staged model every substep / horizon step
(tools/make_hoisted_constants_golden.py, tests/golden/hoisted_constants).  With those per-launch constants formed once in front
of the horizon loop the same operations meet the same operands, so costs, perturbations, visualisation rows, the update and every
q / qd of the dump are compared for EQUALITY of their bit patterns, and oct-pair must equal oct.

The fixtures of tests/golden/lane_scalars all use the velocity drive, two substeps, gravity off and the default links: a hoist
that ignores one of the flags passes them.  The cases here change ONE of these at a time on the arm of lane_scalar_cases.panda_stick
(K = 24, H = 3: two workgroups, the second with an owner wavefront without a live sample; K = 16, H = 1): the effort drive, gravity
on (under either drive), one and three substeps, the cost link on an inner body with the visualised link on another one (the
owner hands over two poses), and the generic instantiation (panda_gripper) with gravity on.  The recording script refuses a pair
of fixtures that does not differ where it must (PAIRS), so a constant that is read but ignored cannot pass;
test_fixture_pairs_differ re-reads that from the fixtures, without a GPU."""
import os

import numpy as np
import pytest

import lane_scalar_cases as L
from mppiisaac.backend import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hoisted_constants")
LANE_GOLDEN = os.path.join(HERE, "golden", "lane_scalars")
EFFORT_KD = 10.0   # the damping of the effort drive (isaacgym_wrapper.DRIVE_GAINS)


def _gravity(m, on):
    m.actors[m.robot_actor].gravity = int(on)


def effort(K, H, gravity=False):
    scene, m, cfg, cost, dof, root = L.panda_stick(K, H)
    m.drive_mode, m.drive_kd = capi.DRIVE_EFFORT, EFFORT_KD
    _gravity(m, gravity)
    return scene, m, cfg, cost, dof, root


def effort_gravity(K, H):
    return effort(K, H, gravity=True)


def gravity(K, H):
    scene, m, cfg, cost, dof, root = L.panda_stick(K, H)
    _gravity(m, True)
    return scene, m, cfg, cost, dof, root


def _substeps(n):
    def make(K, H):
        scene, m, cfg, cost, dof, root = L.panda_stick(K, H)
        m.substeps = n   # (dt stays: h = dt / substeps)
        return scene, m, cfg, cost, dof, root
    return make


def links(K, H):
    """the cost link on body 3, the visualised link on body 5: the owner hands over two poses per step (own_viz)"""
    scene, m, cfg, cost, dof, root = L.panda_stick(K, H)
    cost.link[0] = scene.rigid_body_index("panda", "panda_link4")
    cfg.viz_link = scene.link_names.index("panda_link6")
    cfg.want_rollouts = 1
    assert m.links[cost.link[0]].body == 3 and m.links[cfg.viz_link].body == 5
    return scene, m, cfg, cost, dof, root


def gripper_gravity(K, H):
    scene, m, cfg, cost, dof, root = L.panda_gripper(K, H)
    _gravity(m, True)
    return scene, m, cfg, cost, dof, root


CASES = {"effort-K24-H3": (effort, 24, 3), "effort_gravity-K24-H3": (effort_gravity, 24, 3), "gravity-K24-H3": (gravity, 24, 3),
         "substeps1-K24-H3": (_substeps(1), 24, 3), "substeps3-K24-H3": (_substeps(3), 24, 3), "links-K24-H3": (links, 24, 3),
         "effort_gravity-K16-H1": (effort_gravity, 16, 1), "substeps3-K16-H1": (_substeps(3), 16, 1), "links-K16-H1": (links, 16, 1),
         "gripper_gravity-K24-H3": (gripper_gravity, 24, 3)}
# (a, b, keys): fixtures a and b must differ in every one of `keys`.  "lane:<name>" is a fixture of tests/golden/lane_scalars:
# the same arm under the velocity drive, two substeps, gravity off, the default links
PAIRS = [("effort-K24-H3", "lane:panda_stick-K24-H3", ("S", "dump_dof")),            # effort against velocity
         ("effort_gravity-K24-H3", "effort-K24-H3", ("S", "dump_dof")),             # gravity on against off, effort drive
         ("gravity-K24-H3", "lane:panda_stick-K24-H3", ("S", "dump_dof")),           # ... velocity drive
         ("substeps1-K24-H3", "lane:panda_stick-K24-H3", ("S", "dump_dof")),         # 1 against 2 substeps
         ("substeps3-K24-H3", "lane:panda_stick-K24-H3", ("S", "dump_dof")),         # 3 against 2
         ("substeps1-K24-H3", "substeps3-K24-H3", ("S", "dump_dof")),               # 1 against 3
         ("links-K24-H3", "lane:panda_stick-K24-H3", ("S", "viz")),                  # another cost link, another visualised link
         ("effort_gravity-K16-H1", "lane:panda_stick-K16-H1", ("S", "dump_dof")),
         ("substeps3-K16-H1", "lane:panda_stick-K16-H1", ("S", "dump_dof")),
         ("links-K16-H1", "lane:panda_stick-K16-H1", ("S", "viz")),
         ("gripper_gravity-K24-H3", "lane:panda_gripper-K24-H3", ("S", "dump_dof"))]


def fixture(name):
    path = os.path.join(LANE_GOLDEN, name[5:] + ".npz") if name.startswith("lane:") else os.path.join(GOLDEN, name + ".npz")
    z = np.load(path)
    return {kernel: {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(kernel + ".")} for kernel in L.KERNELS}


def differing(a, b, keys):
    """per kernel and key: how many bit patterns of the two runs `a`, `b` ({kernel: {key: uint32 array}}) differ"""
    return {(kernel, key): int((np.asarray(a[kernel][key]).view(np.uint32) != np.asarray(b[kernel][key]).view(np.uint32)).sum())
            for kernel in L.KERNELS for key in keys}


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    return capi.load_library()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_shapes(name):
    make, K, H = CASES[name]
    scene, m, cfg, cost, dof, root = make(K, H)
    for kernel, want in fixture(name).items():
        assert want["S"].dtype == np.uint32 and want["S"].shape == (K,) and want["dump_dof"].shape == (H, K, 2 * m.n_bodies)
        assert ("viz" in want) == bool(cfg.want_rollouts)
        assert all(np.isfinite(v.view(np.float32)).all() for v in want.values()), (name, kernel)


@pytest.mark.parametrize("a,b,keys", PAIRS)
def test_fixture_pairs_differ(a, b, keys):
    fa, fb = fixture(a), fixture(b)
    for key in ("eps",):   # the same noise on both sides: what differs comes from the changed constant
        for kernel in L.KERNELS:
            np.testing.assert_array_equal(fa[kernel][key], fb[kernel][key])
    counts = differing(fa, fb, keys)
    assert all(n > 0 for n in counts.values()), (a, b, counts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_octet_kernels_reproduce_the_recorded_bits(name, lib):
    make, K, H = CASES[name]
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
    for key in runs["oct"]:
        np.testing.assert_array_equal(runs["oct-pair"][key].view(np.uint32), runs["oct"][key].view(np.uint32), err_msg=f"{name}: oct-pair vs oct, {key}")
