#!/usr/bin/env python3
"""GPU: the time of the distance transform (include/dexr_distance_transform.h) on 64^3, 128^3 and 256^3 samples for clouds of 1e4 and
1e6 points, against the same field in torch on the same GPU (chunked cdist of the samples against the occupied voxel centres, then
min), against scipy.ndimage.distance_transform_edt on the host where scipy is installed, and beside SdfGrid.from_mesh.

    python tools/edt_probe.py [--out DIR]          every step, each a process of its own under `timeout`; DIR gets the lines too
    python tools/edt_probe.py --step edt_128_1e6   one step; prints one JSON line

The cloud is a noisy spherical shell (radius 0.05, noise 1 mm) in the box +-0.08, what a depth camera sees of a ball.  Timing: device
events around the enqueued entry after a warm-up of the same shape, the median of three.  `total` is dexr_edt_points_dev (clearing
the counts, the voxelisation, three passes, the finishing kernel); `passes` is dexr_edt_occupancy_dev, unsigned, on the occupancy that
cloud produces (three passes and the finishing kernel, nothing that depends on the number of points); `voxelisation` is their
DIFFERENCE, not a timing of its own.  The driver stops at the first step that fails or runs into its limit and starts nothing after
it."""
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
SIZES, COUNTS = (64, 128, 256), ("1e4", "1e6")
STEPS = [(f"edt_{n}_{c}", 120) for n in SIZES for c in COUNTS] + [(f"torch_{n}_{c}", 420) for n in SIZES for c in COUNTS]
STEPS += [(f"scipy_{n}", 300) for n in SIZES] + [("mesh_64", 300)]


def _grid(n):
    return (n, n, n), np.full(3, -BOX), 2 * BOX / (n - 1)


def _cloud(torch, count):
    g = torch.Generator(device="cuda").manual_seed(count)
    u = torch.randn((count, 3), generator=g, device="cuda")
    u = u / u.norm(dim=1, keepdim=True) * 0.05 + torch.randn((count, 3), generator=g, device="cuda") * 1e-3
    return u.float().contiguous()


def _median_of_three(torch, run):
    run()  # warm-up of this shape
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(times)), times


def _transform(torch, n, count):
    """-> (values, count grid, seconds total, seconds passes, their runs)"""
    from dex_retargeting_amd import _lib

    shape, o, h = _grid(n)
    pts = _cloud(torch, count)
    v = torch.empty(shape, dtype=torch.float32, device="cuda")
    c = torch.empty(shape, dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.edt_workspace_bytes(shape), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    md = h * (3 * (n - 1) ** 2) ** 0.5
    total = _median_of_three(torch, lambda: _lib.edt_points_dev(pts.data_ptr(), count, shape, o, h, 1, 0.0, md, v.data_ptr(), 0, c.data_ptr(),
                                                                ws.data_ptr(), ws.numel(), stream=st))
    occ = (c > 0).to(torch.uint8).contiguous()
    v2 = torch.empty_like(v)
    passes = _median_of_three(torch, lambda: _lib.edt_occupancy_dev(occ.data_ptr(), shape, h, False, 0.0, md, v2.data_ptr(), 0, ws.data_ptr(),
                                                                    ws.numel(), stream=st))
    assert torch.equal(v, v2)
    return v, c, total, passes


def step_edt(n, count):
    import torch

    v, c, total, passes = _transform(torch, n, count)
    return dict(samples=n ** 3, points=count, occupied=int((c > 0).sum().item()), kept=int(c.sum().item()), seconds_total=total[0],
                seconds_passes=passes[0], seconds_voxelisation_by_difference=total[0] - passes[0], all_total=total[1], all_passes=passes[1],
                checksum=float(v.double().sum().item()))


def step_torch(n, count):
    import torch

    v, c, _, _ = _transform(torch, n, count)
    shape, o, h = _grid(n)
    centres = torch.nonzero(c > 0).double()
    ax = torch.arange(n, device="cuda", dtype=torch.float64)
    samples = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    chunk = max(1, min(len(samples), (1 << 28) // max(1, len(centres))))  # a chunk's distance matrix: 2^28 float32 at most
    cf, sf = centres.float(), samples.float()  # index units: small integers, exact in float32
    torch.cdist(sf[:chunk], cf).min(1)  # warm-up
    torch.cuda.synchronize()
    out = torch.empty(len(samples), dtype=torch.float32, device="cuda")
    t0 = time.perf_counter()
    for s in range(0, len(samples), chunk):
        out[s:s + chunk] = torch.cdist(sf[s:s + chunk], cf).min(1).values
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    err = float(((out.double() * h).reshape(shape) - v.double()).abs().max().item())
    return dict(samples=n ** 3, points=count, occupied=len(centres), pairs=len(samples) * len(centres), chunk=chunk, seconds=t,
                max_abs_difference_to_the_kernels=err)


def step_scipy(n):
    try:
        from scipy import ndimage
    except ImportError:
        return dict(samples=n ** 3, scipy="absent")
    import torch

    v, c, _, _ = _transform(torch, n, 10 ** 6)
    free = (c == 0).cpu().numpy()
    t0 = time.perf_counter()
    d = ndimage.distance_transform_edt(free)
    t = time.perf_counter() - t0
    h = _grid(n)[2]
    return dict(samples=n ** 3, points=10 ** 6, seconds=t, threads=1, max_abs_difference_to_the_kernels=float(np.abs(d * h - v.cpu().numpy()).max()))


def step_mesh():
    """a different field, same consumer: the signed distance to the icosphere's surface against the unsigned distance to its vertices"""
    import torch

    import mesh_reference as mr
    from dex_retargeting_amd import collision

    verts, faces = mr.icosphere(5, 0.05)
    mesh = collision.TriangleMesh(verts, faces)
    shape, o, h = _grid(64)
    pts = torch.tensor(verts, dtype=torch.float32, device="cuda")
    out = {}
    for name, make in (("from_mesh_float32", lambda: collision.SdfGrid.from_mesh(mesh, o, h, shape, precision="float32")),
                       ("from_points", lambda: collision.SdfGrid.from_points(pts, o, h, shape, radius=0.0))):
        make()  # warm-up
        t0 = time.perf_counter()
        g = make()
        out[f"seconds_{name}"] = time.perf_counter() - t0  # a host clock: both end in a copy of the samples to the host
        out[f"checksum_{name}"] = float(np.abs(g.values.astype(np.float64)).sum())
    return dict(samples=64 ** 3, triangles=len(faces), points=len(verts), note="a different field, same consumer", **out)


def run_step(name):
    kind, *rest = name.split("_")
    if kind == "edt":
        return step_edt(int(rest[0]), int(float(rest[1])))
    if kind == "torch":
        return step_torch(int(rest[0]), int(float(rest[1])))
    if kind == "scipy":
        return step_scipy(int(rest[0]))
    if name == "mesh_64":
        return step_mesh()
    raise SystemExit(f"unknown step {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--only", default="", help="comma-separated steps of the driver (default: all)")
    ap.add_argument("--out", default=None, help="directory that also gets the lines as edt_probe.jsonl (default: print only)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(dict(step=args.step, **run_step(args.step))), flush=True)
        return 0
    log = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        log = open(os.path.join(args.out, "edt_probe.jsonl"), "a")
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
