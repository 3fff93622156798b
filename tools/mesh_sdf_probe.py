#!/usr/bin/env python3
"""GPU: point-triangle pairs per second of the mesh distance kernels (include/dexr_mesh_sdf.h) in both precisions, against the same
formulas in torch (chunked brute force on the GPU) and in numpy (tests/mesh_reference.py on the CPU, a 16^3 subset).

    python tools/mesh_sdf_probe.py [--out DIR]            every step, each a process of its own under `timeout`; DIR gets the lines too
    python tools/mesh_sdf_probe.py --step kernel32_64     one step; prints one JSON line

The mesh is the icosphere of 20 480 triangles (k = 5, r = 0.05), sampled on 64^3 and 128^3 samples of the box +-0.08.  Timing: device
events around the enqueued float32 entry (after a warm-up of the same shape, the median of three), a host clock around the float64
host entry, which ends in a device synchronise and holds the copies of its samples (32 MB at most against seconds of kernel).  The
driver stops at the first step that fails or runs into its limit and starts nothing after it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

BOX = 0.08
STEPS = [("kernel32_64", 120), ("kernel32_128", 180), ("kernel64_64", 180), ("kernel64_128", 300), ("torch32_64", 300), ("torch64_64", 300),
         ("numpy_16", 300)]


def _mesh():
    import mesh_reference as mr
    from dex_retargeting_amd import collision

    v, f = mr.icosphere(5, 0.05)
    return v, f, collision.TriangleMesh(v, f)


def _grid(n):
    return (n, n, n), np.full(3, -BOX), np.full(3, 2 * BOX / (n - 1))


def step_kernel32(n):
    import torch

    v, f, mesh = _mesh()
    dm = mesh.device_mesh(torch.cuda.current_device())
    shape, o, h = _grid(n)
    buf = torch.empty(shape, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dm.sample_grid_dev(shape, o, h, buf.data_ptr(), stream=st)  # warm-up of this shape
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dm.sample_grid_dev(shape, o, h, buf.data_ptr(), stream=st)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    pairs = n ** 3 * len(f)
    t = float(np.median(times))
    return dict(samples=n ** 3, triangles=len(f), pairs=pairs, seconds=t, all_seconds=times, pairs_per_second=pairs / t,
                checksum=float(buf.double().abs().sum().item()))


def step_kernel64(n):
    v, f, mesh = _mesh()
    dm = mesh.device_mesh()
    dm.sample_grid((16, 16, 16), *_grid(16)[1:])  # warm-up: the code object and the allocator
    shape, o, h = _grid(n)
    times = []
    for _ in range(2 if n <= 64 else 1):
        t0 = time.perf_counter()
        vals = dm.sample_grid(shape, o, h)
        times.append(time.perf_counter() - t0)
    pairs = n ** 3 * len(f)
    t = float(np.median(times))
    return dict(samples=n ** 3, triangles=len(f), pairs=pairs, seconds=t, all_seconds=times, pairs_per_second=pairs / t,
                checksum=float(np.abs(vals.astype(np.float64)).sum()))


def _torch_sdf(a, ab, ac, p):
    """the formulas of include/dexr_mesh_sdf.h on (P, 1, 3) against (1, T, 3), in the tensors' dtype; the winding sum in float64"""
    import torch

    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    ap = p - a
    bp, cp = ap - ab, ap - ac
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    w6, den = e43 / (e43 + e56), va + vb + vc
    v, w = vb / den, vc / den
    conds = [(va <= 0) & (e43 >= 0) & (e56 >= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (d6 >= 0) & (d5 <= d6), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
             (d3 >= 0) & (d4 <= d3), (d1 <= 0) & (d2 <= 0)]
    vals = [(one - w6, w6), (zero, d2 / (d2 - d6)), (zero, one), (d1 / (d1 - d3), zero), (one, zero), (zero, zero)]
    for c, (vv, ww) in zip(conds, vals):  # the last region first: an earlier one overrides
        v, w = torch.where(c, vv, v), torch.where(c, ww, w)
    e = ap - v[..., None] * ab - w[..., None] * ac
    q = dot(e, e).min(1).values
    la, lb, lc = ap.norm(dim=-1), bp.norm(dim=-1), cp.norm(dim=-1)
    det = -dot(ap, torch.cross(bp, cp, dim=-1))
    omega = 2 * torch.atan2(det, la * lb * lc + dot(ap, bp) * lc + dot(bp, cp) * la + dot(cp, ap) * lb)
    wn = omega.double().sum(1) * 0.07957747154594767
    u = q.sqrt()
    return torch.where(wn >= 0.5, -u, u)


def step_torch(n, dtype_name):
    import torch

    import mesh_reference as mr

    dtype = getattr(torch, dtype_name)
    v, f = mr.icosphere(5, 0.05)
    a, ab, ac = (torch.tensor(x, dtype=dtype, device="cuda")[None] for x in mr.records(v, f))
    shape, o, h = _grid(n)
    pts = torch.tensor(mr.grid_points(shape, o, h), dtype=dtype, device="cuda")
    chunk = 2048  # 2048 x 20480 pairs: the temporaries of a chunk stay within a few GB
    _torch_sdf(a, ab, ac, pts[:chunk, None])  # warm-up
    torch.cuda.synchronize()
    out = torch.empty(len(pts), dtype=dtype, device="cuda")
    t0 = time.perf_counter()
    for s in range(0, len(pts), chunk):
        out[s:s + chunk] = _torch_sdf(a, ab, ac, pts[s:s + chunk, None])
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    pairs = len(pts) * len(f)
    return dict(samples=len(pts), triangles=len(f), pairs=pairs, seconds=t, pairs_per_second=pairs / t, chunk=chunk,
                checksum=float(out.double().abs().sum().item()))


def step_numpy():
    import mesh_reference as mr

    v, f = mr.icosphere(5, 0.05)
    shape, o, h = _grid(16)
    pts = mr.grid_points(shape, o, h)
    t0 = time.perf_counter()
    d, _ = mr.sdf(v, f, pts, np.float64)
    t = time.perf_counter() - t0
    pairs = len(pts) * len(f)
    return dict(samples=len(pts), triangles=len(f), pairs=pairs, seconds=t, pairs_per_second=pairs / t, checksum=float(np.abs(d).sum()))


def run_step(name):
    if name.startswith("kernel32_"):
        return step_kernel32(int(name.split("_")[1]))
    if name.startswith("kernel64_"):
        return step_kernel64(int(name.split("_")[1]))
    if name.startswith("torch32_"):
        return step_torch(int(name.split("_")[1]), "float32")
    if name.startswith("torch64_"):
        return step_torch(int(name.split("_")[1]), "float64")
    if name == "numpy_16":
        return step_numpy()
    raise SystemExit(f"unknown step {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--only", default="", help="comma-separated steps of the driver (default: all)")
    ap.add_argument("--out", default=None, help="directory that also gets the lines as mesh_sdf_probe.jsonl (default: print only)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(dict(step=args.step, **run_step(args.step))), flush=True)
        return 0
    log = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        log = open(os.path.join(args.out, "mesh_sdf_probe.jsonl"), "a")
    only = [s for s in args.only.split(",") if s]
    for name, limit in STEPS:
        if only and name not in only:
            continue
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        print(f"{name}: exit {r.returncode} {line}", flush=True)
        if r.returncode != 0:
            print(r.stderr[-2000:], flush=True)
            line = json.dumps(dict(step=name, failed=r.returncode))
        if log:
            log.write(line + "\n")
            log.flush()
        if r.returncode != 0:
            return 1  # nothing more is started on the GPU after a step that failed
    return 0


if __name__ == "__main__":
    sys.exit(main())
