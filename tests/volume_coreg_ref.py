"""Host reference for the --coregister tests (numpy only, fp64): what mud_volume_joint_hist must compute (include/mudiff_hip.h), and the
synthetic "head" the recovery tests register.  Coordinates and the trilinear rule are volume_regrid_ref's."""
import numpy as np

import volume_regrid_ref as G

HEAD_SHAPE = (44, 40, 36)
TRUE_PARAMS = (2.3, -1.7, 1.1, 3.0, -2.0, 4.0)            # mm, mm, mm, deg, deg, deg
BAR_MEAN, BAR_MAX = 0.25, 0.5                             # voxels: the recovery bar


def sample_coordinates(M, shape, stride):
    """p = M (i, j, k, 1) in fp64 at the sample points (all indices multiples of stride) -> three [nx,ny,nz] arrays (the arithmetic of
    volume_regrid_ref.coordinates)."""
    M = np.asarray(M, np.float64)
    i, j, k = np.meshgrid(*[np.arange(0, n, stride, dtype=np.float64) for n in shape], indexing='ij')
    return [((M[a, 0] * i + M[a, 1] * j) + M[a, 2] * k) + M[a, 3] for a in range(3)]


def bin_of(v, lo, scale, bins):
    """clamp((int)floor((double(v) - lo) * scale), 0, bins - 1), two roundings."""
    d = np.asarray(v, np.float32).astype(np.float64) - np.float64(lo)
    d = np.floor(d * np.float64(scale))
    return np.clip(d, 0, bins - 1).astype(np.int64)


def joint_hist(fix, mov, M, stride, ranges, bins, details=False):
    """fix: fp32 [X,Y,Z], mov: fp32 [SX,SY,SZ] (the values the pipeline sees) -> int64 [bins, bins].  With `details` also a dict: counted
    (number of counted samples), points (number of sample points), inside (bool per sample point: p in the overlap), p, fix_values /
    mov64 / mov_values (at the samples inside the overlap: fp32, the fp64 sum, its fp32 rounding), finite (which of those are counted)."""
    fix, mov = np.asarray(fix, np.float32), np.asarray(mov, np.float32)
    p = sample_coordinates(M, fix.shape, stride)
    with np.errstate(invalid='ignore'):
        inside = np.ones(p[0].shape, bool)
        for a in range(3):
            inside &= (p[a] >= 0) & (p[a] <= mov.shape[a] - 1)
    q = [v[inside] for v in p]
    f = [np.floor(v) for v in q]
    w = [v - fv for v, fv in zip(q, f)]
    acc = np.zeros(q[0].shape, np.float64)
    with np.errstate(invalid='ignore'):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    wgt = ((w[0] if dx else 1.0 - w[0]) * (w[1] if dy else 1.0 - w[1])) * (w[2] if dz else 1.0 - w[2])
                    ii = [np.minimum(fv + d, mov.shape[a] - 1).astype(np.int64) for a, (fv, d) in enumerate(zip(f, (dx, dy, dz)))]
                    use = wgt != 0                        # (inside the overlap a neighbour past the edge has weight 0)
                    v = mov[ii[0], ii[1], ii[2]].astype(np.float64)
                    acc = acc + np.where(use, np.where(use, v, 0.0) * wgt, 0.0)
    mv = acc.astype(np.float32)
    fv = fix[::stride, ::stride, ::stride][inside]
    ok = np.isfinite(fv) & np.isfinite(mv)
    flo, fscale, mlo, mscale = ranges
    idx = bin_of(fv[ok], flo, fscale, bins) * bins + bin_of(mv[ok], mlo, mscale, bins)
    hist = np.bincount(idx, minlength=bins * bins).reshape(bins, bins).astype(np.int64)
    if not details:
        return hist
    return hist, dict(counted=int(ok.sum()), points=int(inside.size), inside=inside, p=p, fix_values=fv, mov64=acc, mov_values=mv, finite=ok)


def n_edge(info, ranges, bins, src_max, mov_shape):
    """The counted samples whose bin the device may place differently: the fp64 moving value within 2^-22 |v| + 1e-9 max|src| of a bin
    edge, or p within 1e-9 of the overlap's border (all sample points for the latter, counted or not)."""
    _, _, mlo, mscale = ranges
    v = info['mov64'][info['finite']]
    tol = 2.0 ** -22 * np.abs(v) + 1e-9 * src_max
    t = (v - mlo) * mscale
    dist = np.abs(t - np.round(t)) / mscale if mscale > 0 else np.full(v.shape, np.inf)
    inner = (np.round(t) >= 1) & (np.round(t) <= bins - 1)           # (edges 0 and bins are clamped away)
    near = int((inner & (dist <= tol)).sum())
    border = np.zeros(info['inside'].shape, bool)
    with np.errstate(invalid='ignore'):
        for a in range(3):
            border |= (np.abs(info['p'][a]) <= 1e-9) | (np.abs(info['p'][a] - (mov_shape[a] - 1)) <= 1e-9)
    return near + int(border.sum())


def ranges_of(fix, mov, bins):
    """mudiff_hip.volume_coreg.bin_ranges for value arrays: finite min / max of each."""
    out = []
    for a in (fix, mov):
        a = np.asarray(a, np.float32)
        a = a[np.isfinite(a)].astype(np.float64)
        lo, hi = (float(a.min()), float(a.max())) if a.size else (0.0, 0.0)
        out += [lo, float(bins) / (hi - lo) if hi > lo else 0.0]
    return tuple(out)


# ---------------------------------------------------------------------------------------------------
# the synthetic head
# ---------------------------------------------------------------------------------------------------
def _smooth(a, sigma):
    r = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in range(3):
        a = np.apply_along_axis(lambda v: np.convolve(np.pad(v, r, mode='reflect'), k, mode='valid'), axis, a)
    return a


def head(shape=HEAD_SHAPE, seed=11):
    """-> (t in [0, 1] [X,Y,Z] float64: gaussian noise smoothed with sigma = 2.5 voxels, mask: the ellipsoid of radii 0.40 shape)."""
    rng = np.random.default_rng(seed)
    t = _smooth(rng.standard_normal(shape), 2.5)
    t = (t - t.min()) / (t.max() - t.min())
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2.0) / (0.40 * n) for n in shape], indexing='ij')
    return t, (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 1.0


def fixed_contrast(t, mask):
    return np.asfortranarray(((200.0 + 800.0 * t) * mask).astype(np.float32))


def moving_contrast(t, mask):
    return np.asfortranarray(((900.0 - 600.0 * t ** 2 + 150.0 * np.sin(9.0 * t)) * mask).astype(np.float32))


def moved(vol, M_true, seed=12, sigma=8.0, mask=None):
    """The volume a patient who moved leaves: moved[q] = vol[inv(M_true) q] (trilinear), so that M_true is the sampling matrix that
    undoes it; plus gaussian noise of `sigma` where the moved `mask` is."""
    inv = np.linalg.inv(np.asarray(M_true, np.float64))
    out = G.trilinear(vol, inv, vol.shape).astype(np.float64)
    if mask is not None and sigma > 0:
        inside = G.trilinear(mask.astype(np.float32), inv, vol.shape) > 0.5
        out = out + np.random.default_rng(seed).standard_normal(vol.shape) * sigma * inside
    return np.asfortranarray(out.astype(np.float32))


def displacement_error(M, M_true, mask):
    """|M x - M_true x| over the mask's voxels, in moving voxels -> (mean, max)."""
    idx = np.argwhere(mask).astype(np.float64)
    h = np.concatenate([idx, np.ones((idx.shape[0], 1))], 1).T
    d = (np.asarray(M, np.float64)[:3] - np.asarray(M_true, np.float64)[:3]) @ h
    e = np.sqrt((d ** 2).sum(0))
    return float(e.mean()), float(e.max())
