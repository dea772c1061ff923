#!/usr/bin/env python3
"""Fixtures of tests/test_gpu_hoisted_constants.py: what the octet rollout kernels compute, bit for bit, when the per-launch
constants of the owner's step - the drive mode, (h, kd), `substeps`, the gravity flag, the bodies of the cost link and of the
visualised link - are NOT the ones every fixture of tests/golden/lane_scalars uses.  Recorded ONCE on the GPU by the build that read
them from the staged model where they are used; a later build must reproduce every bit.

Per case of tests/test_gpu_hoisted_constants.py (CASES) and per kernel (MPPI_ROLLOUT=oct-pair, =oct): what
tools/make_lane_scalar_golden.py records (lane_scalar_cases.run_gpu), stored as the raw bit patterns of the float32 values in
tests/golden/hoisted_constants/<case>.npz.

The script REFUSES to write anything unless every pair of PAIRS differs where it must (gravity on against off, effort against
velocity, 1 against 3 substeps, the moved links), on identical noise: a constant that is read but ignored cannot pass.
--cpu: the fp32 oracle on the same cases and the same pairs (q, qd after every step; the link case: the bodies of its links) - no
GPU needed.
Usage: python tools/make_hoisted_constants_golden.py [--cpu]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mppi-isaac_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import lane_scalar_cases as L  # noqa: E402
import test_gpu_hoisted_constants as T  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


def require(cond, what):
    if not cond:
        sys.exit(f"REFUSED: {what}")


def oracle_rollout(o, make, K, H):
    scene, m, cfg, cost, dof, root = make(K, H)
    q, qd, _ = L.oracle_paths(o, m, cfg, cost, dof, root, L.nominal(cfg), o.sample(cfg))
    require(np.isfinite(q).all() and np.isfinite(qd).all(), "the oracle's rollout is not finite")
    return m, cfg, cost, np.stack([q, qd])


def cpu_main():
    o = Oracle("f32")
    lane = {"lane:" + n: v for n, v in L.CASES.items()}
    rolled = {}

    def get(name):
        if name not in rolled:
            make, K, H = (lane if name.startswith("lane:") else T.CASES)[name]
            rolled[name] = oracle_rollout(o, make, K, H)
        return rolled[name]

    for a, b, keys in T.PAIRS:
        (ma, ca, ka, xa), (mb, cb, kb, xb) = get(a), get(b)
        if "dump_dof" in keys:
            n = int((xa.astype(np.float32) != xb.astype(np.float32)).sum())
            print(f"{a} against {b} (oracle fp32): {n} of {xa.size} q / qd values differ")
            require(n > 0, f"{a} and {b}: the oracle's trajectories are equal")
        else:   # the links moved: the states are the same, the poses handed over are other bodies'
            ba, bb = (ma.links[ka.link[0]].body, ma.links[ca.viz_link].body), (mb.links[kb.link[0]].body, mb.links[cb.viz_link].body)
            print(f"{a} against {b}: (cost link body, visualised link body) {ba} against {bb}")
            require(np.array_equal(xa, xb) and ba[0] != bb[0] and ba[1] != bb[1] and ba[0] != ba[1], f"{a} and {b}: the links did not move")


def main():
    if "--cpu" in sys.argv[1:]:
        return cpu_main()
    import torch
    from mppiisaac.backend import capi
    require(torch.cuda.is_available(), "no GPU")
    lib = capi.load_library()
    recorded = {}
    for name, (make, K, H) in T.CASES.items():
        runs = {}
        for kernel in L.KERNELS:
            info, out = L.run_gpu(lib, make, K, H, kernel)
            require(info["rollout"] == kernel, f"{name}: asked for {kernel}, ran {info}")
            require(all(np.isfinite(v).all() for v in out.values()), f"{name} {kernel}: non-finite output")
            runs[kernel] = {key: np.ascontiguousarray(v).view(np.uint32) for key, v in out.items()}
        for key in runs[L.KERNELS[0]]:
            require(np.array_equal(runs[L.KERNELS[0]][key], runs[L.KERNELS[1]][key]), f"{name}: {L.KERNELS} differ in {key}")
        recorded[name] = runs
    for a, b, keys in T.PAIRS:
        fa, fb = recorded[a], recorded[b] if b in recorded else T.fixture(b)
        require(all(np.array_equal(fa[k]["eps"], fb[k]["eps"]) for k in L.KERNELS), f"{a} and {b}: not the same noise")
        counts = T.differing(fa, fb, keys)
        print(f"{a} against {b}: values that differ {counts}")
        require(all(n > 0 for n in counts.values()), f"{a} and {b} do not differ in {[k for k, n in counts.items() if n == 0]}")
    os.makedirs(T.GOLDEN, exist_ok=True)
    for name, runs in recorded.items():
        path = os.path.join(T.GOLDEN, name + ".npz")
        np.savez_compressed(path, **{f"{kernel}.{key}": v for kernel, out in runs.items() for key, v in out.items()})
        print(f"wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
