"""Host reference for the --regrid_interp cubic tests (numpy only, fp64): what mud_volume_bspline_coeffs and mud_volume_regrid_cubic must
compute (include/mudiff_hip.h), operation by operation - numpy rounds every product and sum separately, as the
kernels do.  Volumes are [X,Y,Z] arrays as everywhere in the tests; the device's [Z][Y][X] buffers are their transposes."""
import numpy as np

import volume_bias_ref as B
import volume_regrid_ref as G

POLE = np.sqrt(np.float64(3.0)) - np.float64(2.0)


def filter_axis(c, axis):
    """The recursion along one axis of an fp64 array, every line at once (each line sees exactly the per-line operations, in order)."""
    c = np.moveaxis(np.asarray(c, np.float64), axis, 0)
    N, z = c.shape[0], POLE
    if N == 1:
        return np.moveaxis(c.copy(), 0, axis)
    g = 6.0 * c
    a, zk = np.zeros(c.shape[1:], np.float64), np.float64(1.0)
    for k in range(2 * N - 2):
        a = a + zk * g[k if k <= N - 1 else 2 * N - 2 - k]
        zk = zk * z
    cp = np.empty_like(g)
    cp[0] = a / (1.0 - zk)
    for i in range(1, N):
        cp[i] = g[i] + z * cp[i - 1]
    out = np.empty_like(g)
    out[N - 1] = (z / (z * z - 1.0)) * (cp[N - 1] + z * cp[N - 2])
    for i in range(N - 2, -1, -1):
        out[i] = z * (out[i + 1] - cp[i])
    return np.moveaxis(out, 0, axis)


def coefficients(values):
    """fp32 values [X,Y,Z] (what the pipeline sees of a file) -> (fp64 coefficients [X,Y,Z], the number of non-finite voxels): a
    non-finite value is read as 0; the recursion runs along x, then y, then z."""
    v = np.asarray(values, np.float32)
    ok = np.isfinite(v)
    c = np.where(ok, v, np.float32(0)).astype(np.float64)
    for axis in (0, 1, 2):
        c = filter_axis(c, axis)
    return c, int((~ok).sum())


def value_range(values):
    """(lo, hi): the range of the finite values, widened to contain 0 (what mud_volume_fg_range yields, widened)."""
    v = np.asarray(values, np.float32)
    v = v[np.isfinite(v)]
    return (min(float(v.min()), 0.0), max(float(v.max()), 0.0)) if v.size else (0.0, 0.0)


def mirror(i, S):
    """Index arrays in [-1, S + 1] of an axis of S under mirror boundaries."""
    if S == 1:
        return np.zeros_like(i)
    i = np.where(i < 0, -i, i)
    i = np.where(i > S - 1, 2 * (S - 1) - i, i)
    return np.where(i < 0, -i, i)


def in_range(M, src_shape, out_shape):
    """Where 0 <= p_a <= S_a - 1 on every axis -> (bool [X,Y,Z], the coordinates)."""
    p = G.coordinates(M, out_shape)
    inside = np.ones(tuple(out_shape), bool)
    for a in range(3):
        inside &= (p[a] >= 0.0) & (p[a] <= np.float64(src_shape[a] - 1))
    return inside, p


def tissue(values, f, t):
    """The background guard at the points (f, t): is any in-volume trilinear neighbour of non-zero weight a voxel that is not 0?"""
    v = np.asarray(values, np.float32)
    found = np.zeros(f[0].shape, bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = ((t[0] if dx else 1.0 - t[0]) * (t[1] if dy else 1.0 - t[1])) * (t[2] if dz else 1.0 - t[2])
                idx = [f[a] + d for a, d in enumerate((dx, dy, dz))]
                use = w != 0
                for a in range(3):
                    use &= idx[a] < v.shape[a]
                ii = [np.minimum(idx[a], v.shape[a] - 1) for a in range(3)]
                found |= use & (v[ii[0], ii[1], ii[2]] != 0)
    return found


def interpolate(coeffs, values, M, out_shape, lo, hi, guard=True, clamp=True, rounded=True):
    """mud_volume_regrid_cubic: coeffs fp64 [SX,SY,SZ] of the fp32 `values` -> fp32 [X,Y,Z].  Without `guard` / `clamp` the background
    guard / the clamp to [lo, hi] is left out, without `rounded` the fp64 sum is returned as it is (the comparison with scipy)."""
    c = np.asarray(coeffs, np.float64)
    S = c.shape
    inside, p = in_range(M, S, out_shape)
    fl = [np.where(inside, np.floor(v), 0.0) for v in p]
    t = [np.where(inside, v - fv, 0.0) for v, fv in zip(p, fl)]
    f = [fv.astype(np.int64) for fv in fl]
    b = [B.bspline(tv) for tv in t]
    acc = np.zeros(tuple(out_shape), np.float64)
    for dz in range(4):
        for dy in range(4):
            for dx in range(4):
                w = (b[0][dx] * b[1][dy]) * b[2][dz]
                acc = acc + w * c[mirror(f[0] - 1 + dx, S[0]), mirror(f[1] - 1 + dy, S[1]), mirror(f[2] - 1 + dz, S[2])]
    if clamp:
        acc = np.where(acc < lo, np.float64(lo), acc)
        acc = np.where(acc > hi, np.float64(hi), acc)
    keep = inside & tissue(values, f, t) if guard else inside
    return np.where(keep, acc.astype(np.float32), np.float32(0)) if rounded else np.where(keep, acc, 0.0)


def regrid(values, M, out_shape):
    """range -> coefficients -> interpolation of fp32 values [SX,SY,SZ]: what volume_regrid.regrid(mode='cubic') computes."""
    c, _ = coefficients(values)
    return interpolate(c, values, M, out_shape, *value_range(values))
