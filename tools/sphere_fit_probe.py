#!/usr/bin/env python3
"""GPU: the sphere fit (include/dexr_sphere_fit.h) on the links of a Shadow-sized hand -- 24 links, 8 spheres each, every link a
tessellated capsule or box (no asset needed), sampled by `collision.link_grid` at 32 and at 48 samples along the longest side --
against the same greedy search in numpy on the host (tests/sphere_fit_reference.py) and in torch on the same GPU (chunked `cdist`
membership, `argmax` per round), and the launches of the largest body: 64^3 samples, all interior, 128 spheres.

    python tools/sphere_fit_probe.py [--out DIR]          every step, each a process of its own under `timeout`; DIR gets the lines too
    python tools/sphere_fit_probe.py --step kernel_48     one step; prints one JSON line

Timing: device events around the one enqueued call (after a warm-up of the same shapes, the median of three); a host clock around
the numpy and the torch searches (torch ends in a device synchronise).  The grids are made before the clock starts.  `launch_64`:
every round enqueues the same two launches whatever is covered already (the walk of a candidate does not depend on the mask), so the
call with ONE sphere -- the first kernel, one gain launch, one apply launch -- bounds the longest single launch from above, and the
call with 128 spheres divided by 128 is the mean of a round.  The driver stops at the first step that fails or runs into its limit."""
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

K = 8
STEPS = [("kernel_32", 180), ("kernel_48", 180), ("launch_64", 180), ("torch_32", 400), ("torch_48", 400), ("numpy_32", 900)]


def hand_meshes():
    """24 link meshes: a palm and four more boxes, nineteen capsules (a cylinder and two spheres) of finger-link sizes"""
    from dex_retargeting_amd import collision, meshio

    def at(z):
        T = np.eye(4)
        T[2, 3] = z
        return T

    out = [collision.TriangleMesh(*meshio.box_mesh(s)) for s in ((0.09, 0.03, 0.1), (0.03, 0.02, 0.04), (0.025, 0.02, 0.03), (0.05, 0.03, 0.02),
                                                                 (0.02, 0.018, 0.05))]
    for i in range(19):
        r, length = 0.007 + 0.0005 * (i % 5), 0.02 + 0.004 * (i % 7)
        parts = [("cylinder", (r, length), np.eye(4)), ("sphere", (r,), at(-length / 2)), ("sphere", (r,), at(length / 2))]
        out.append(collision.TriangleMesh(*meshio.link_mesh(parts)))
    return out


def hand_grids(max_dim):
    from dex_retargeting_amd import collision

    return [collision.link_grid(m, max_dim) for m in hand_meshes()]


def _device_call(grids, k):
    """-> (seconds of the median of three calls, index, gain, count)"""
    import torch

    from dex_retargeting_amd import _lib

    dims = np.array([g.shape for g in grids], np.int32)
    sizes = np.array([g.values.size for g in grids], np.int64)
    offset = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    spacing = [g.spacing[0] for g in grids]
    kk = np.full(len(grids), k, np.int32)
    values = torch.from_numpy(np.concatenate([g.values.reshape(-1) for g in grids])).cuda()
    index, gain = (torch.empty((len(grids), k), dtype=torch.int32, device="cuda") for _ in range(2))
    count = torch.empty((len(grids), 3), dtype=torch.int32, device="cuda")
    nb = _lib.sphere_fit_workspace_bytes(dims)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.sphere_fit_dev(dims, spacing, offset, kk, 0.0, 0.0, 1.0, values.numel(), values.data_ptr(), index.data_ptr(), gain.data_ptr(),
                            count.data_ptr(), ws.data_ptr(), nb, stream=st)

    call()  # warm-up of these shapes
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(times)), times, index.cpu().numpy(), gain.cpu().numpy(), count.cpu().numpy()


def step_kernel(max_dim):
    grids = hand_grids(max_dim)
    t, times, index, gain, count = _device_call(grids, K)
    cover = (count[:, 1] / np.maximum(count[:, 0], 1)).round(3).tolist()
    return dict(links=len(grids), k=K, max_dim=max_dim, samples=int(sum(g.values.size for g in grids)), interior=int(count[:, 0].sum()),
                seconds=t, all_seconds=times, coverage_per_link=cover, coverage_min=min(cover), coverage_mean=float(np.mean(cover)),
                spheres=int(count[:, 2].sum()), checksum=int(index.astype(np.int64).sum()))


def step_launch_64():
    from dex_retargeting_amd import collision

    n, h = 64, 0.001
    i = np.arange(n)
    d = np.minimum(i, n - 1 - i) + 0.5  # cells to the nearest face of a box half a cell outside the grid
    v = -(np.minimum(np.minimum(d[:, None, None], d[None, :, None]), d[None, None, :]) * h).astype(np.float32)
    grid = collision.SdfGrid(v, 0.0, h)
    one, times1, _, _, _ = _device_call([grid], 1)
    full, times, index, gain, count = _device_call([grid], 128)
    return dict(samples=n ** 3, interior=int(count[0, 0]), first_round_seconds=one, first_round_all=times1, rounds=int(count[0, 2]), all_rounds_seconds=full,
                all_rounds_all=times, mean_round_seconds=full / max(1, int(count[0, 2])), covered=int(count[0, 1]), checksum=int(index.astype(np.int64).sum()))


def _torch_fit(values, h, k, chunk=1 << 25):
    """the greedy rounds of include/dexr_sphere_fit.h in torch: membership by a chunked cdist of index triples, argmax of a packed key"""
    import torch

    v = torch.from_numpy(values).cuda()
    interior = v < 0
    ijk = torch.nonzero(interior).double()  # every interior sample is a candidate (min_radius = 0)
    flat = torch.nonzero(interior.reshape(-1)).reshape(-1)
    t = (-v[interior].double()) / h
    m = torch.floor(t * t).clamp(max=float(2 ** 20 - 1))
    uncovered = torch.ones(len(ijk), dtype=torch.bool, device="cuda")
    index, gains = [], []
    for _ in range(k):
        if not bool(uncovered.any()):
            break
        unc = ijk[uncovered]
        gain = torch.empty(len(ijk), dtype=torch.int64, device="cuda")
        step = max(1, chunk // max(1, len(unc)))
        for s in range(0, len(ijk), step):
            d2 = torch.cdist(ijk[s:s + step], unc).square().round()
            gain[s:s + step] = (d2 <= m[s:s + step, None]).sum(1)
        key = (gain << 40) | (m.long() << 20) | ((1 << 20) - 1 - flat)
        w = int(torch.argmax(key))
        if int(gain[w]) == 0:
            break
        index.append(int(flat[w]))
        gains.append(int(gain[w]))
        uncovered &= ~((ijk - ijk[w]).square().sum(1) <= m[w])
    return index, gains


def step_torch(max_dim):
    import torch

    grids = hand_grids(max_dim)
    _, _, index, gain, count = _device_call(grids, K)
    _torch_fit(grids[0].values, grids[0].spacing[0], 1)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fits = [_torch_fit(g.values, g.spacing[0], K) for g in grids]
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    same = all(i == index[b, :len(i)].tolist() and gn == gain[b, :len(gn)].tolist() and len(i) == count[b, 2] for b, (i, gn) in enumerate(fits))
    return dict(links=len(grids), k=K, max_dim=max_dim, seconds=t, equal_to_the_kernel=bool(same))


def step_numpy(max_dim):
    import sphere_fit_reference as sr

    grids = hand_grids(max_dim)
    _, _, index, gain, count = _device_call(grids, K)
    t0 = time.perf_counter()
    fits = [sr.fit(g.values, g.spacing[0], K) for g in grids]
    t = time.perf_counter() - t0
    same = all(np.array_equal(f[0], index[b]) and np.array_equal(f[1], gain[b]) and np.array_equal(f[2], count[b]) for b, f in enumerate(fits))
    return dict(links=len(grids), k=K, max_dim=max_dim, seconds=t, equal_to_the_kernel=bool(same))


def run_step(name):
    kind, n = name.split("_")
    if kind == "kernel":
        return step_kernel(int(n))
    if kind == "launch":
        return step_launch_64()
    if kind == "torch":
        return step_torch(int(n))
    if kind == "numpy":
        return step_numpy(int(n))
    raise SystemExit(f"unknown step {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--only", default="", help="comma-separated steps of the driver (default: all)")
    ap.add_argument("--out", default=None, help="directory that also gets the lines as sphere_fit_probe.jsonl (default: print only)")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(dict(step=args.step, **run_step(args.step))), flush=True)
        return 0
    log = None
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        log = open(os.path.join(args.out, "sphere_fit_probe.jsonl"), "a")
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
