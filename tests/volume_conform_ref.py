"""The numpy restatement of --conform / --antialias (mudiff_hip.volume_conform, csrc/volume_lowpass.hip): the conform
grid, the anti-aliasing rule, the three-pass low-pass exactly as defined (fp64 products and sums with t ascending, one rounding to fp32
per pass) and its composition with volume_regrid_ref's trilinear.  Written from the definitions, not from the package's code."""
import numpy as np

import volume_regrid_ref as G

WORLD_AXIS = {'R': (0, 1.0), 'L': (0, -1.0), 'A': (1, 1.0), 'P': (1, -1.0), 'S': (2, 1.0), 'I': (2, -1.0)}


def conform_grid(first_shape, first_world, shape=(240, 240, 155), spacing=(1.0, 1.0, 1.0), target='LPS'):
    """-> (shape, affine): axis v runs towards target[v] in steps of spacing[v]; the grid centre lies on the first input's grid centre."""
    a = np.zeros((4, 4))
    for v, letter in enumerate(target):
        w, sign = WORLD_AXIS[letter]
        a[w, v] = sign * spacing[v]
    first_world = np.asarray(first_world, np.float64)
    centre = first_world @ np.append((np.asarray(first_shape, np.float64) - 1) / 2, 1.0)
    a[:3, 3] = centre[:3] - a[:3, :3] @ ((np.asarray(shape, np.float64) - 1) / 2)
    a[3, 3] = 1.0
    return tuple(shape), a


def factors(M):
    return np.sqrt((np.asarray(M, np.float64)[:3, :3] ** 2).sum(1))


def sigma(f, tol=1e-6):
    return float(np.sqrt(f * f - 1.0) / (2.0 * np.sqrt(2.0 * np.log(2.0)))) if f > 1.0 + tol else 0.0


def radius(s):
    return int(np.ceil(3.0 * s))


def weights(s):
    """exp(-t^2 / (2 s^2)) for t = -R..R, or None for s = 0."""
    if s == 0:
        return None
    t = np.arange(-radius(s), radius(s) + 1, dtype=np.float64)
    return np.exp(-t * t / (2.0 * s * s))


def one_pass(v, w, axis, keep=np.float32):
    """v: [X,Y,Z] -> (sum_t w[t] v[i+t]) / (sum_t w[t]) along `axis`, both sums over the t with 0 <= i + t < S, t ascending, in fp64;
    rounded to `keep` once."""
    R = (len(w) - 1) // 2
    v = np.moveaxis(np.asarray(v, np.float64), axis, 0)
    S = v.shape[0]
    acc, den = np.zeros(v.shape), np.zeros(v.shape)
    for t in range(-R, R + 1):
        lo, hi = max(0, -t), min(S, S - t)                   # the i with 0 <= i + t < S
        if lo >= hi:
            continue
        acc[lo:hi] += w[t + R] * v[lo + t:hi + t]
        den[lo:hi] += w[t + R]
    return np.moveaxis((acc / den).astype(keep), 0, axis)


def lowpass(values, weights_xyz, keep=np.float32):
    """values: fp32 [X,Y,Z] (the values the pipeline sees) -> (the volume after the passes in x, y, z order, the non-finite voxels read
    as 0).  Without any weights: the values themselves."""
    v = np.asarray(values, np.float32)
    if all(w is None for w in weights_xyz):
        return v, 0
    bad = ~np.isfinite(v)
    v = np.where(bad, np.float32(0), v)
    for axis, w in enumerate(weights_xyz):
        if w is not None:
            v = one_pass(v, w, axis, keep)
    return v, int(bad.sum())


def antialiased_trilinear(values, M, out_shape, keep=np.float32):
    """The low-pass the rule asks for under the sampling matrix M, then volume_regrid_ref.trilinear.  keep=np.float64 carries the
    intermediates in fp64 (what the fp32 pipeline is measured against)."""
    low, _ = lowpass(values, [weights(sigma(f)) for f in factors(M)], keep)
    if keep is np.float32:
        return G.trilinear(low, M, out_shape)
    return trilinear64(low, M, out_shape)


def trilinear64(src, M, out_shape):
    """volume_regrid_ref.trilinear on an fp64 source, returned in fp64: the reference the fp32 chain's own error is measured against."""
    src = np.asarray(src, np.float64)
    px, py, pz = G.coordinates(M, out_shape)
    out = np.zeros(out_shape, np.float64)
    fx, fy, fz = np.floor(px), np.floor(py), np.floor(pz)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                xx, yy, zz = fx + dx, fy + dy, fz + dz
                w = (1 - np.abs(px - xx)) * (1 - np.abs(py - yy)) * (1 - np.abs(pz - zz))
                ok = (xx >= 0) & (xx < src.shape[0]) & (yy >= 0) & (yy < src.shape[1]) & (zz >= 0) & (zz < src.shape[2]) & (w != 0)
                xi, yi, zi = (np.clip(c, 0, s - 1).astype(np.int64) for c, s in zip((xx, yy, zz), src.shape))
                out += np.where(ok, src[xi, yi, zi] * w, 0.0)
    return out


def stripes(shape, period=2, lo=0.0, hi=200.0):
    """Stripes along x: lo at even multiples of period / 2, hi at odd ones."""
    x = np.arange(shape[0])
    v = np.where((x // (period // 2)) % 2 == 0, lo, hi).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(v[:, None, None], shape))


def blobs(affine, shape, centres_mm, widths_mm, amplitudes):
    """One analytic field, a sum of Gaussian blobs in world millimetres, sampled on the grid (shape, affine) -> fp64 [X,Y,Z]."""
    i, j, k = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing='ij')
    a = np.asarray(affine, np.float64)
    w = [a[r, 0] * i + a[r, 1] * j + a[r, 2] * k + a[r, 3] for r in range(3)]
    out = np.zeros(shape)
    for c, s, amp in zip(centres_mm, widths_mm, amplitudes):
        out += amp * np.exp(-sum((w[r] - c[r]) ** 2 for r in range(3)) / (2.0 * s * s))
    return out
