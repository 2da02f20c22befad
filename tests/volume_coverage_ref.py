"""numpy restatement of mud_volume_interval_coverage (csrc/volume_coverage.hip)."""
import numpy as np

N, BELOW, ABOVE, INSIDE, NONFINITE = range(5)
WIDTH, WIDTH_INSIDE = range(2)


def coverage(lo, hi, gt, region=None, nreg=1, z0=0, z1=None):
    """lo, hi, gt float32 [Z, X, Y], region uint8 bits or None (every voxel in every region) -> (int64 counts [planes, nreg, 5], float64
    sums [planes, nreg, 2], z0, z1) for the planes z0..z1 clipped to the volume.  A voxel with a NaN in lo, hi or gt counts as NONFINITE
    only; of the others, BELOW is gt < lo, ABOVE gt > hi, INSIDE neither; the widths are float64(hi) - float64(lo), summed with
    math-exact order left to numpy (the test's tolerance is relative 1e-10)."""
    lo, hi, gt = (np.asarray(a, np.float32) for a in (lo, hi, gt))
    Z = lo.shape[0]
    z0, z1 = max(0, int(z0)), Z - 1 if z1 is None else min(Z - 1, int(z1))
    counts = np.zeros((z1 - z0 + 1, nreg, 5), np.int64)
    sums = np.zeros((z1 - z0 + 1, nreg, 2), np.float64)
    for z in range(z0, z1 + 1):
        l, h, g = lo[z], hi[z], gt[z]
        nan = np.isnan(l) | np.isnan(h) | np.isnan(g)
        with np.errstate(invalid='ignore'):
            below, above = ~nan & (g < l), ~nan & (g > h)
        inside = ~nan & ~below & ~above
        w = np.where(nan, 0.0, h.astype(np.float64) - l.astype(np.float64))
        for k in range(nreg):
            m = np.ones(l.shape, bool) if region is None else ((region[z] >> k) & 1).astype(bool)
            counts[z - z0, k] = [(m & ~nan).sum(), (m & below).sum(), (m & above).sum(), (m & inside).sum(), (m & nan).sum()]
            sums[z - z0, k] = [w[m].sum(), w[m & inside].sum()]
    return counts, sums, z0, z1
