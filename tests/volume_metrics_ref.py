"""fp64 numpy / scipy restatement of the volume scores (mudiff_hip.volume_metrics): the reference that
csrc/volume_metrics.hip is tested against, itself checked against a brute-force loop over the windows."""
import math

import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2
COV_NORM = 343.0 / 342.0


def _ssim_from_moments(ux, uy, uxx, uyy, uxy):
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def interior(shape):
    """Voxels whose 7x7x7 window lies inside the volume."""
    m = np.zeros(shape, bool)
    m[3:-3, 3:-3, 3:-3] = True
    return m


def ssim_map(pred, gt):
    """skimage's structural_similarity map carried to three axes (uniform 7x7x7 window, data_range 1); only the interior is meaningful."""
    from scipy.ndimage import uniform_filter
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    f = lambda a: uniform_filter(a, size=7, mode='reflect')       # noqa: E731  (the border is cropped: the mode does not matter)
    return _ssim_from_moments(f(p), f(g), f(p * p), f(g * g), f(p * g))


def ssim_map_brute(pred, gt):
    """The same map by a loop over the interior windows (NaN outside the interior)."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    out = np.full(p.shape, np.nan)
    Z, X, Y = p.shape
    for z in range(3, Z - 3):
        for x in range(3, X - 3):
            for y in range(3, Y - 3):
                a, b = p[z - 3:z + 4, x - 3:x + 4, y - 3:y + 4], g[z - 3:z + 4, x - 3:x + 4, y - 3:y + 4]
                out[z, x, y] = _ssim_from_moments(a.mean(), b.mean(), (a * a).mean(), (b * b).mean(), (a * b).mean())
    return out


def _scores(d, S, inner, sel):
    n, ni = int(sel.sum()), int((sel & inner).sum())
    if n == 0:
        return dict(voxels=0, interior_voxels=ni, psnr=None, mae=None, ssim3d=None)
    mse = float(np.mean(d[sel] ** 2))
    return dict(voxels=n, interior_voxels=ni, psnr=math.inf if mse == 0 else 10 * math.log10(1 / mse), mae=float(np.mean(np.abs(d[sel]))),
                ssim3d=float(np.mean(S[sel & inner])) if ni else None)


def pearson(a, b):
    """Two-pass Pearson correlation; None when either variance is 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a - a.mean(), b - b.mean()
    va, vb = float(np.sum(a * a)), float(np.sum(b * b))
    return None if va == 0 or vb == 0 else float(np.sum(a * b)) / math.sqrt(va * vb)


def score(pred, gt, region, names, std=None, ssim=None):
    """Scores of [Z, X, Y] pred / gt with region bits (bit k = names[k]) and an optional std volume ->
    {name: voxels, interior_voxels, psnr, mae, ssim3d, per_plane {psnr, mae, ssim3d} [, mean_std, pearson_r]}.
    `ssim`: a precomputed SSIM map (default: ssim_map)."""
    p, g = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    d = p - g
    S = ssim_map(p, g) if ssim is None else ssim
    inner = interior(p.shape)
    region = np.asarray(region)
    out = {}
    for k, name in enumerate(names):
        sel = (region >> k) & 1 == 1
        r = _scores(d, S, inner, sel)
        r['per_plane'] = {key: [] for key in ('psnr', 'mae', 'ssim3d')}
        for z in range(p.shape[0]):
            pz = np.zeros_like(sel)
            pz[z] = sel[z]
            v = _scores(d, S, inner, pz)
            for key in ('psnr', 'mae', 'ssim3d'):
                r['per_plane'][key].append(v[key])
        if std is not None:
            s = np.asarray(std, np.float64)
            r['mean_std'] = float(np.mean(s[sel])) if sel.any() else None
            r['pearson_r'] = pearson(s[sel], np.abs(d[sel])) if sel.any() else None
        out[name] = r
    return out
