"""Host reference for the --denoise tests (numpy only): the definition of DESIGN.md section 5.15 that the kernels of
csrc/volume_denoise.hip mirror operation by operation - the pseudo-residual keys, the radix-select histograms, the non-local-means
estimate - and the noisy slab of the recovery tests.  Volumes are [X,Y,Z] arrays as everywhere in the tests."""
import numpy as np

SKIP = np.uint32(0xFFFFFFFF)
K = np.float32(np.sqrt(6.0 / 7.0))
SLAB_SHAPE, SLAB_SIGMA = (24, 20, 18), 30.0
# what the restatement alone reaches on the slab at the true sigma, and the sigma it estimates there; the bar
# of both recovery tests is 1.5 x the ratio, the estimate must sit within 20 % of the true 30
RECORDED_RATIO = 0.12777
RECORDED_SIGMA = 32.237
BAR = 1.5 * RECORDED_RATIO


def residual_keys(values):
    """fp32 values [X,Y,Z] -> uint32 keys [X,Y,Z]: the bits of |eps|, eps = sqrtf(6/7) * (v - (sum of the six face neighbours, fp32, in
    the order -x +x -y +y -z +z) / 6), over the voxels that are > 0 and have six face neighbours inside, finite and > 0; SKIP elsewhere."""
    v = np.asarray(values, np.float32)
    keys = np.full(v.shape, SKIP, np.uint32)
    if min(v.shape) < 3:
        return keys
    c = v[1:-1, 1:-1, 1:-1]
    six = [v[:-2, 1:-1, 1:-1], v[2:, 1:-1, 1:-1], v[1:-1, :-2, 1:-1], v[1:-1, 2:, 1:-1], v[1:-1, 1:-1, :-2], v[1:-1, 1:-1, 2:]]
    with np.errstate(invalid='ignore', over='ignore'):
        ok = np.isfinite(c) & (c > 0)
        for a in six:
            ok &= np.isfinite(a) & (a > 0)
        s = six[0] + six[1]
        for a in six[2:]:
            s = s + a
        eps = K * (c - s / np.float32(6))
    keys[1:-1, 1:-1, 1:-1] = np.where(ok, np.abs(eps).astype(np.float32).view(np.uint32), SKIP)
    return keys


def select_hist(keys, prefix, which):
    """One pass of the radix select -> int64 [256]: the counts of byte 3 - which over the keys that are not SKIP and whose `which`
    higher bytes equal prefix."""
    k = np.asarray(keys, np.uint32).reshape(-1)
    k = k[k != SKIP]
    shift = 24 - 8 * int(which)
    if which:
        k = k[(k >> np.uint32(shift + 8)) == np.uint32(prefix)]
    return np.bincount(((k >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256).astype(np.int64)


def sigma_by_sorting(values):
    """-> (sigma, samples): 1.4826 x the lower median of |eps| found by sorting (what the radix select must equal); (0.0, 0) without a
    sample."""
    keys = residual_keys(values).reshape(-1)
    keys = np.sort(keys[keys != SKIP])
    if not keys.size:
        return 0.0, 0
    return 1.4826 * float(keys[(keys.size - 1) // 2: (keys.size - 1) // 2 + 1].view(np.float32)[0]), int(keys.size)


def nlm(values, sigma, search=2, patch=1, beta=1.0, rician=False, details=False):
    """The estimate of every voxel -> fp32 [X,Y,Z].  Candidates in z-outermost / x-fastest order; per candidate d2 = the fp32 sum of
    D_t over the patch offsets that count (z outermost, x fastest) / their number, w = exp(-(d2 / h)) in fp32; sw, sa in fp64.  With
    `details` -> (the estimate, m fp64: the weighted mean, in rician mode less 2 sigma^2, before the clamp and the square root)."""
    out = nlm_modes(values, sigma, search, patch, beta, (bool(rician),))[bool(rician)]
    return out if details else out[0]


def nlm_modes(values, sigma, search=2, patch=1, beta=1.0, modes=(False, True)):
    """nlm(..., details=True) for several `rician` modes at once (the weights do not depend on the mode) -> {mode: (estimate, m)}."""
    v = np.asarray(values, np.float32)
    X, Y, Z = v.shape
    s, r = int(search), int(patch)
    H = s + r
    P = np.full((X + 2 * H, Y + 2 * H, Z + 2 * H), np.nan, np.float32)
    P[H:H + X, H:H + Y, H:H + Z] = v
    ok = np.isfinite(P)
    h = np.float32(2.0 * float(beta) * float(sigma) * float(sigma))
    a_all = {False: P.astype(np.float64)}
    a_all[True] = a_all[False] * a_all[False]

    def window(a, o, grow):                        # the volume grown by `grow` voxels per side, seen through the offset o
        lo = H - grow
        return a[lo + o[0]:lo + o[0] + X + 2 * grow, lo + o[1]:lo + o[1] + Y + 2 * grow, lo + o[2]:lo + o[2] + Z + 2 * grow]

    sw, wmax = np.zeros(v.shape, np.float64), np.zeros(v.shape, np.float32)
    sa = {mode: np.zeros(v.shape, np.float64) for mode in modes}
    zero = (0, 0, 0)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore', under='ignore'):
        for oz in range(-s, s + 1):
            for oy in range(-s, s + 1):
                for ox in range(-s, s + 1):
                    o = (ox, oy, oz)
                    if o == zero:
                        continue
                    counts = window(ok, zero, r) & window(ok, o, r)
                    d = window(P, zero, r) - window(P, o, r)
                    D = np.where(counts, d * d, np.float32(0))       # (an entry that does not count adds +0: the sum's bits are those
                    number = counts.astype(np.int32)                 # of the sum that skips it, every term being >= 0)
                    total, n = np.zeros(v.shape, np.float32), np.zeros(v.shape, np.int32)
                    for pz in range(2 * r + 1):
                        for py in range(2 * r + 1):
                            for px in range(2 * r + 1):
                                total = total + D[px:px + X, py:py + Y, pz:pz + Z]
                                n = n + number[px:px + X, py:py + Y, pz:pz + Z]
                    cand = counts[r:r + X, r:r + Y, r:r + Z]
                    d2 = total / np.maximum(n, 1).astype(np.float32)
                    w = np.exp(-(d2 / h)).astype(np.float32)
                    w64 = w.astype(np.float64)
                    sw = np.where(cand, sw + w64, sw)
                    for mode in modes:
                        sa[mode] = np.where(cand, sa[mode] + w64 * window(a_all[mode], o, 0), sa[mode])
                    wmax = np.where(cand, np.maximum(wmax, w), wmax)
        centre = np.where(wmax > 0, wmax.astype(np.float64), 1.0)      # no candidate (or every weight 0): the voxel itself
        result = {}
        for mode in modes:
            m = (sa[mode] + centre * window(a_all[mode], zero, 0)) / (sw + centre)
            if mode:
                m = m - (2.0 * float(sigma)) * float(sigma)
            out = (np.sqrt(np.maximum(m, 0.0)) if mode else m).astype(np.float32)
            result[mode] = (np.where(np.isfinite(v) & (v != 0), out, v), m)
    return result


def phantom(shape, seed, head=True, sigma=30.0):
    """-> fp64 [X,Y,Z]: three tissue classes (400 / 700 / 1000, the terciles of a smooth function) plus Gaussian noise inside an
    ellipsoid (the whole volume without `head`), exact zeros outside it, and in the planes x < 3 a Rayleigh-like background |noise|
    (where the Rician correction takes voxels to 0)."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    smooth = np.sin(2.1 * g[0] + 0.3) + np.cos(1.7 * g[1] - 0.2) * np.sin(1.3 * g[2]) + 0.5 * g[0] * g[1]
    q = np.quantile(smooth, [1 / 3, 2 / 3])
    tissue = np.select([smooth < q[0], smooth < q[1]], [400.0, 700.0], 1000.0) + rng.standard_normal(shape) * sigma
    inside = (g[0] / 0.9) ** 2 + (g[1] / 0.85) ** 2 + (g[2] / 0.9) ** 2 < 1 if head else np.ones(shape, bool)
    vol = np.where(inside, np.maximum(tissue, 1.0), 0.0)
    if head:
        vol[:3] = np.maximum(np.abs(rng.standard_normal((3,) + tuple(shape[1:])) * sigma), 0.5)
    return vol


def slab(shape=SLAB_SHAPE, sigma=SLAB_SIGMA, seed=1):
    """-> (noisy fp32 [X,Y,Z] F-ordered, clean): 400 for x < 12 and 700 elsewhere, plus Gaussian noise."""
    clean = np.where(np.arange(shape[0])[:, None, None] < 12, 400.0, 700.0) * np.ones(shape)
    noisy = clean + np.random.default_rng(seed).standard_normal(shape) * sigma
    return np.asfortranarray(noisy.astype(np.float32)), clean


def recovery_ratio(denoised, noisy, clean):
    rmse = lambda a: float(np.sqrt(np.mean((np.asarray(a, np.float64) - clean) ** 2)))      # noqa: E731
    return rmse(denoised) / rmse(noisy)
