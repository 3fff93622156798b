"""The yardstick of the distance transform (include/dexr_distance_transform.h): numpy and brute force.  The voxelisation in float64
exactly as the header defines it, d2 as the minimum over ALL occupied voxels of the integer squared offset -- no separable pass, no
envelope: it shares no algorithm with the kernels it judges -- and both output forms in float64, rounded once to float32."""
import numpy as np

NONE = 1 << 30  # DEXR_EDT_NONE
PAIRS_AT_ONCE = 1 << 22  # sample-voxel pairs of one chunk of the brute force


def voxel_indices(points, n, origin, h):
    """points (N, 3) -> (idx (N, 3) float64 = floor(u + 0.5), keep (N,) bool, u (N, 3)): the rule of the header, float64, the division a
    multiplication by the reciprocal"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    inv = 1.0 / float(h)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (p - np.asarray(origin, dtype=np.float64)) * inv
        f = np.floor(u + 0.5)
        keep = np.isfinite(p).all(1) & (f >= 0).all(1) & (f < np.asarray(n, dtype=np.float64)).all(1)
    return f, keep, u


def voxelise(points, n, origin, h):
    """-> count (nx, ny, nz) int32, saturated at 2^31 - 1"""
    f, keep, _ = voxel_indices(points, n, origin, h)
    idx = f[keep].astype(np.int64)
    count = np.zeros(tuple(n), dtype=np.int64)
    np.add.at(count, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
    return np.minimum(count, 2 ** 31 - 1).astype(np.int32)


def d2_brute(occupied):
    """occupied (nx, ny, nz) bool -> d2 (nx, ny, nz) int32: every sample against every occupied voxel"""
    occupied = np.asarray(occupied, dtype=bool)
    n = occupied.shape
    vox = np.argwhere(occupied).astype(np.int32)
    if len(vox) == 0:
        return np.full(n, NONE, dtype=np.int32)
    samples = np.stack(np.meshgrid(*[np.arange(k, dtype=np.int32) for k in n], indexing="ij"), -1).reshape(-1, 3)
    out = np.empty(len(samples), dtype=np.int32)
    step = max(1, PAIRS_AT_ONCE // len(vox))
    for a in range(0, len(samples), step):
        d = samples[a:a + step, None, :] - vox[None, :, :]
        out[a:a + step] = (d * d).sum(-1).min(1)
    return out.reshape(n)


def clamped_distance(d2, h, max_distance):
    """float64: max_distance where d2 is NONE, min(h sqrt(d2), max_distance) otherwise"""
    d2 = np.asarray(d2)
    t = float(h) * np.sqrt(np.where(d2 == NONE, 0, d2).astype(np.float64))
    return np.where(d2 == NONE, float(max_distance), np.minimum(t, float(max_distance)))


def unsigned_values(d2, h, radius, max_distance):
    return (clamped_distance(d2, h, max_distance) - float(radius)).astype(np.float32)


def signed_values(occupied, h, max_distance):
    """-> (values float32, d2 to the occupied voxels, d2 to the free ones)"""
    occupied = np.asarray(occupied, dtype=bool)
    to_occ, to_free = d2_brute(occupied), d2_brute(~occupied)
    half = float(h) * 0.5
    v = np.where(occupied, -clamped_distance(to_free, h, max_distance) + half, clamped_distance(to_occ, h, max_distance) - half)
    return v.astype(np.float32), to_occ, to_free


def from_points(points, n, origin, h, min_points=1, radius=0.0, max_distance=None):
    """-> (values float32, d2 int32, count int32)"""
    if max_distance is None:
        max_distance = default_max_distance(n, h)
    count = voxelise(points, n, origin, h)
    d2 = d2_brute(count >= min_points)
    return unsigned_values(d2, h, radius, max_distance), d2, count


def default_max_distance(n, h):
    """the diagonal of the grid's box, as collision.py forms it"""
    import math

    return float(h) * math.sqrt(sum((int(k) - 1) ** 2 for k in n))


def ulp_distance(a, b):
    """float32 arrays of finite values -> int64 array: how many float32 values apart"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
