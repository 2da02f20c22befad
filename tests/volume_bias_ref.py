"""Host reference for the --bias_correct tests (numpy only, fp64): the definition of DESIGN.md section 5.14 that the kernels of
csrc/volume_bias.hip mirror operation by operation, an engine that drives mudiff_hip.volume_bias.loop from it, and the synthetic head
of the recovery tests.  Volumes are [X,Y,Z] arrays as everywhere in the tests; a lattice of level l is a C-ordered fp64 array
[m][m][m], m = 2^l + 3, indexed [cz][cy][cx] (the device's flat order)."""
import numpy as np

import volume_coreg_ref as K

HEAD_SHAPE = K.HEAD_SHAPE
RECOVERY = dict(shrink=2, levels=4, iters=50, tol=1e-3, bins=200, fwhm=0.15, wiener=0.01)
# the ratio the restatement alone reaches on the recovery volume; the bar of both recovery tests is 1.5 x it
RECORDED_RATIO = 0.02304
BAR = 1.5 * RECORDED_RATIO


def bspline(t):
    """The four uniform cubic B-spline weights at t in [0, 1), in the order of evaluation the device uses -> [4, ...]."""
    t = np.asarray(t, np.float64)
    omt = 1.0 - t
    t2 = t * t
    t3 = t2 * t
    b0 = ((omt * omt) * omt) / 6.0
    b1 = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0
    b2 = (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0
    b3 = t3 / 6.0
    return np.stack([b0, b1, b2, b3])


def axis_weights(idx, S, n):
    """Voxel indices on an axis of size S, n spans -> (span int64 [len], weights fp64 [4, len])."""
    x = (np.asarray(idx).astype(np.float64) + 0.5) * np.float64(n)
    x = x / np.float64(S)
    span = np.minimum(np.floor(x), np.float64(n - 1))
    return span.astype(np.int64), bspline(x - span)


def _axes(shape, stride, n):
    return [axis_weights(np.arange(0, S, stride), S, n) for S in shape]


def field(lattices, shape, stride=1):
    """F at the voxels whose indices are multiples of `stride` -> fp64 [nx,ny,nz]: levels in order, then the 4 x 4 x 4 support with x
    fastest, each term (bx*by)*bz * L added to the running sum (no fused multiply-add)."""
    acc = None
    for l, L in enumerate(lattices):
        L = np.asarray(L, np.float64)
        n = 1 << l
        assert L.shape == (n + 3,) * 3
        (sx, bx), (sy, by), (sz, bz) = _axes(shape, stride, n)
        if acc is None:
            acc = np.zeros((sx.size, sy.size, sz.size), np.float64)
        for dz in range(4):
            for dy in range(4):
                for dx in range(4):
                    w = (bx[dx][:, None, None] * by[dy][None, :, None]) * bz[dz][None, None, :]
                    acc = acc + w * L[(sz + dz)[None, None, :], (sy + dy)[None, :, None], (sx + dx)[:, None, None]]
    return acc


def log_image(values, shrink):
    """fp32 values [X,Y,Z] -> u fp32 [nx,ny,nz]: log of the samples that are finite and > 0, NaN elsewhere."""
    v = np.asarray(values, np.float32)[::shrink, ::shrink, ::shrink]
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(v) & (v > 0)
    return np.where(ok, np.log(np.where(ok, v, np.float32(1))), np.float32(np.nan)).astype(np.float32)


def corrected(u, lattices, shape, shrink, c_old=None):
    """-> (c fp32, lo, hi, dmax): c = float32(double(u) - F); lo / hi its finite extremes (None without any); dmax the largest
    |double(c) - double(c_old)| over the samples where that is a number (c_old defaults to u)."""
    u = np.asarray(u, np.float32)
    c = (u.astype(np.float64) - field(lattices, shape, shrink)).astype(np.float32)
    fin = c[np.isfinite(c)]
    lo, hi = (float(fin.min()), float(fin.max())) if fin.size else (None, None)
    d = np.abs(c.astype(np.float64) - np.asarray(u if c_old is None else c_old, np.float32).astype(np.float64))
    d = d[~np.isnan(d)]
    return c, lo, hi, float(d.max()) if d.size else 0.0


def hist(c, lo, scale, bins):
    c = np.asarray(c, np.float32)
    return np.bincount(K.bin_of(c[np.isfinite(c)], lo, scale, bins), minlength=bins).astype(np.int64)


def table_at(c, table, lo, scale):
    """Linear interpolation between bin centres, clamped at the ends, in fp64."""
    table = np.asarray(table, np.float64)
    bins = table.size
    p = np.asarray(c, np.float32).astype(np.float64) - np.float64(lo)
    p = p * np.float64(scale)
    p = p - 0.5
    p = np.minimum(np.maximum(p, 0.0), np.float64(bins - 1))
    i = np.minimum(np.floor(p), np.float64(bins - 2)).astype(np.int64)
    f = p - i
    return table[i] + f * (table[i + 1] - table[i])


def fit(c, table, lo, scale, level, shape, shrink, k):
    """-> (delta, omega): int64 [m][m][m] sums of one level's multilevel-B-spline fit of r = c - table(c) over the finite samples."""
    c = np.asarray(c, np.float32)
    n = 1 << level
    m = n + 3
    (sx, bx), (sy, by), (sz, bz) = _axes(shape, shrink, n)
    ok = np.isfinite(c)
    ix, iy, iz = np.nonzero(ok)
    r = c[ok].astype(np.float64) - table_at(c[ok], table, lo, scale)
    sq = [((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + b[3] * b[3] for b in (bx, by, bz)]
    S2 = (sq[0][ix] * sq[1][iy]) * sq[2][iz]
    delta, omega = np.zeros(m * m * m, np.int64), np.zeros(m * m * m, np.int64)
    two_k = np.float64(2.0) ** int(k)
    for dz in range(4):
        for dy in range(4):
            for dx in range(4):
                w = (bx[dx][ix] * by[dy][iy]) * bz[dz][iz]
                cp = ((sz[iz] + dz) * m + (sy[iy] + dy)) * m + (sx[ix] + dx)
                np.add.at(delta, cp, np.rint(((((w * w) * w) * r) / S2) * two_k).astype(np.int64))
                np.add.at(omega, cp, np.rint((w * w) * two_k).astype(np.int64))
    return delta.reshape(m, m, m), omega.reshape(m, m, m)


def apply(values, lattices):
    """Every voxel: float32(double(v) / exp(F)); a zero stays zero, a non-finite voxel is passed through."""
    v = np.asarray(values, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        out = (v.astype(np.float64) / np.exp(field(lattices, v.shape, 1))).astype(np.float32)
    return np.where(np.isfinite(v) & (v != 0), out, v)


class Engine:
    """What mudiff_hip.volume_bias.loop drives, restated: the log image `u` (from log_image, or the device's own) of a volume `shape`."""

    def __init__(self, u, shape, shrink):
        self.u, self.shape, self.shrink = np.asarray(u, np.float32), tuple(shape), int(shrink)
        self.c = self.u.copy()
        self.n_samples = int(self.u.size)

    def corrected(self, lattices):
        self.c, lo, hi, dmax = corrected(self.u, lattices, self.shape, self.shrink, self.c)
        return lo, hi, dmax

    def hist(self, lo, scale, bins):
        return hist(self.c, lo, scale, bins)

    def fit(self, level, table, lo, scale, k):
        return fit(self.c, table, lo, scale, level, self.shape, self.shrink, k)


# ---------------------------------------------------------------------------------------------------
# the recovery volume
# ---------------------------------------------------------------------------------------------------
def shaded_head(shape=HEAD_SHAPE, seed=11, noise_seed=21):
    """-> (volume fp32 [X,Y,Z] F-ordered, true log field fp64, mask): volume_coreg_ref.head's ellipsoid, three piecewise-constant
    tissue classes (the terciles of its smooth texture: 400 / 700 / 1000), gaussian noise of 2 % of the class spacing, times exp of
    a quadratic field scaled to [-0.3, 0.3] over the mask; zero outside the mask."""
    t, mask = K.head(shape, seed)
    q = np.quantile(t[mask], [1 / 3, 2 / 3])
    tissue = np.select([t < q[0], t < q[1]], [400.0, 700.0], 1000.0)
    tissue = tissue + np.random.default_rng(noise_seed).standard_normal(shape) * (0.02 * 300.0)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    f = 0.5 * g[0] + 0.3 * g[1] - 0.4 * g[2] + 0.6 * g[0] ** 2 - 0.5 * g[1] * g[2] + 0.3 * g[2] ** 2 - 0.4 * g[0] * g[1]
    f = (f - f[mask].min()) / (f[mask].max() - f[mask].min()) * 0.6 - 0.3
    return np.asfortranarray((tissue * np.exp(f) * mask).astype(np.float32)), f, mask


def recovery_ratio(lattices, true_field, mask):
    """RMS over the mask of (estimated - true) log field, each with its masked mean removed, over the RMS of the true field treated
    the same way."""
    est = field(lattices, true_field.shape, 1)[mask]
    tru = true_field[mask]
    est, tru = est - est.mean(), tru - tru.mean()
    return float(np.sqrt(np.mean((est - tru) ** 2)) / np.sqrt(np.mean(tru ** 2)))
