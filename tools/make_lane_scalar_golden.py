#!/usr/bin/env python3
"""Fixtures of tests/test_gpu_lane_scalars.py: what the octet rollout kernels compute, bit for bit, at the smallest shapes in which
their per-joint scalars (drive torque, integration, stops, velocity clamp, sine / cosine, the saturated second solve) take every
path.  Recorded ONCE on the GPU by the build whose arithmetic is the yardstick; a later build must reproduce every bit.

Per case of tests/lane_scalar_cases.py (CASES) and per kernel (MPPI_ROLLOUT=oct-pair, =oct): one mppi_rollout + update from the
case's state, nominal and the configuration's own noise - S, du, the visualisation rows, beta / eta, the nominal after the update
and the action - and one trajectory dump (mppi_rollout_trajectory: every q, qd after every step, the control cost, du), stored as
the raw bit patterns of the float32 values in tests/golden/lane_scalars/<case>.npz.

The script REFUSES to write a fixture unless the recorded rollout itself contains, bit for bit, a joint position equal to a stop
and a |velocity| equal to vmax (read from the dump), and - on the CPU oracle, fp32, on the recorded noise - a saturated drive (a
second solve) in every owner wavefront's samples.   --cpu: only the oracle's side of those conditions (no GPU needed).
Usage: python tools/make_lane_scalar_golden.py [--cpu]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mppi-isaac_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import lane_scalar_cases as L  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lane_scalars")


def require(cond, what):
    if not cond:
        sys.exit(f"REFUSED: {what}")


def oracle_conditions(o, name, make, K, H, eps=None):
    scene, m, cfg, cost, dof, root = make(K, H)
    eps = o.sample(cfg) if eps is None else eps
    q, qd, logs = L.oracle_paths(o, m, cfg, cost, dof, root, L.nominal(cfg), eps)
    stops, clamps = L.path_counts(m, q, qd)
    waves = [bool((logs[w:w + 8] != 0).any()) for w in range(0, K, 8)]
    mixed = bool((logs == 0).any())
    print(f"{name} (oracle fp32): {stops} positions at a stop, {clamps} velocities at vmax, saturated sample-substeps "
          f"{int((logs != 0).sum())} of {logs.size}, per owner wavefront {waves}")
    require(stops > 0 and clamps > 0, f"{name}: the oracle's rollout has no stop / no clamped velocity")
    require(all(waves) and mixed, f"{name}: not every owner wavefront takes the second solve, or no substep goes without it")
    return m


def main():
    cpu_only = "--cpu" in sys.argv[1:]
    o = Oracle("f32")
    if cpu_only:
        for name, (make, K, H) in L.CASES.items():
            oracle_conditions(o, name, make, K, H)
        return
    import torch
    from mppiisaac.backend import capi
    require(torch.cuda.is_available(), "no GPU")
    lib = capi.load_library()
    os.makedirs(OUT, exist_ok=True)
    for name, (make, K, H) in L.CASES.items():
        runs = {}
        for kernel in L.KERNELS:
            info, out = L.run_gpu(lib, make, K, H, kernel)
            require(info["rollout"] == kernel, f"{name}: asked for {kernel}, ran {info}")
            runs[kernel] = out
        ref = runs[L.KERNELS[0]]
        m = oracle_conditions(o, name, make, K, H, eps=ref["eps"].astype(np.float64))
        for kernel, out in runs.items():
            require(all(np.isfinite(v).all() for v in out.values()), f"{name} {kernel}: non-finite output")
            q, qd = L.dump_q_qd(out["dump_dof"])
            stops, clamps = L.path_counts(m, q, qd)
            print(f"{name} {kernel} (GPU dump): {stops} positions at a stop, {clamps} velocities at vmax")
            require(stops > 0 and clamps > 0, f"{name} {kernel}: the recorded rollout has no stop / no clamped velocity")
            for key in out:
                require(np.array_equal(out[key].view(np.uint32), ref[key].view(np.uint32)), f"{name}: {kernel} and {L.KERNELS[0]} differ in {key}")
        arrays = {f"{kernel}.{key}": np.ascontiguousarray(v).view(np.uint32) for kernel, out in runs.items() for key, v in out.items()}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
