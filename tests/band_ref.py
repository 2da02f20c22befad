"""numpy restatement of the thick-volume path (csrc/band.hip, mudiff_hip.thick_volume): the geometry of a thick
volume against the thin grid, the rows of the measurement matrix A, the projection x - A^T (A A^T)^-1 (A (x - s eta) - a y) in fp64 by
a dense solve, an fp32 emulation of the kernel's exact chain, and the rounding bounds the tests hold the kernel to.  Nothing here
imports the package; `constrain_fp32` takes the tables of ops.band_tables as an object with their attributes."""
import math

import numpy as np

EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------
# geometry and weights
# ---------------------------------------------------------------------------------------------------
def geometry(thin_affine, thick_affine):
    """Two 4 x 4 voxel-to-world affines that share the in-plane geometry -> (c0, step, thin_dz): thick slice j has its centre at thin
    index c0 + j * step; thin_dz: the thin grid's slice spacing in mm."""
    a, b = np.asarray(thin_affine, np.float64), np.asarray(thick_affine, np.float64)
    dz = float(np.linalg.norm(a[:3, 2]))
    axis = a[:3, 2] / dz
    c0 = float(np.dot(b[:3, 3] - a[:3, 3], axis)) / dz
    step = float(np.dot(b[:3, 2], axis)) / dz
    return c0, step, dz


def row(n, c, width, profile='box'):
    """fp64 [n]: the weights of the thick slice centred at thin index c, `width` thin slices thick; thin slice i covers
    [i - 1/2, i + 1/2].  box: the overlap length with [c - width / 2, c + width / 2]; gauss: FWHM = width, cut at c +- width, the
    density integrated over each thin slice.  Normalised to sum 1 (all 0 when nothing overlaps)."""
    out = np.zeros(n)
    if profile == 'box':
        lo, hi = c - width / 2.0, c + width / 2.0
        for i in range(n):
            out[i] = max(0.0, min(hi, i + 0.5) - max(lo, i - 0.5))
    else:
        sigma = width / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        lo, hi = c - width, c + width
        for i in range(n):
            p, q = max(lo, i - 0.5), min(hi, i + 0.5)
            if q > p:
                out[i] = 0.5 * (math.erf((q - c) / (sigma * math.sqrt(2.0))) - math.erf((p - c) / (sigma * math.sqrt(2.0))))
    s = out.sum()
    return out / s if s > 0 else out


def support(c, width, profile='box'):
    return (c - width / 2.0, c + width / 2.0) if profile == 'box' else (c - width, c + width)


def weights(n, c0, step, width, profile='box', count=None):
    """The thick slices at c0 + j * step, j = 0..count-1 (None: as many as start inside the stack), against thin slices 0..n-1 ->
    (A fp64 [m, n] over the slices whose support lies inside [-1/2, n - 1/2], their centres [m], their indices j)."""
    rows, centres, idx = [], [], []
    j = 0
    while (j < count) if count is not None else (c0 + j * step <= n - 0.5):
        c = c0 + j * step
        lo, hi = support(c, width, profile)
        if lo >= -0.5 - 1e-9 and hi <= n - 0.5 + 1e-9:
            rows.append(row(n, c, width, profile))
            centres.append(c)
            idx.append(j)
        j += 1
    return np.asarray(rows, np.float64).reshape(len(rows), n), np.asarray(centres), idx


def as_kernel(A):
    """A as the kernel sees it: the weights rounded once to fp32, in fp64."""
    return np.asarray(A, np.float64).astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------
# the projection
# ---------------------------------------------------------------------------------------------------
def measure(x, A):
    """A x in fp64 from the fp32 operands: x [n, P] -> [m, P]."""
    return as_kernel(A) @ np.asarray(x, np.float64)


def constrain(x, y, A, eta=None, a=1.0, s=0.0, clean=True):
    """x - A^T (A A^T)^-1 (A (x - s eta) - a y) in fp64 from the fp32 operands, by a dense solve.  x, eta [n, P]; y [m, P]."""
    A, x, y = as_kernel(A), np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x if clean else x - float(s) * np.asarray(eta, np.float64)
    r = A @ d - (1.0 if clean else float(a)) * y
    return x - A.T @ np.linalg.solve(A @ A.T, r)


def constrain_fp32(x, y, tab, eta=None, a=1.0, s=0.0, clean=True):
    """The kernel's chain in numpy fp32, every product and sum rounded once, in the tables' order: forward substitution while
    accumulating, backward substitution, scatter.  tab: ops.band_tables' object (start, member, w, tstart, tmember, tw, lc, m, n, bw)."""
    f = np.float32
    x, y = np.asarray(x, f), np.asarray(y, f)
    m, n, bw = tab.m, tab.n, tab.bw
    lc = np.asarray(tab.lc, f).reshape(m, bw + 1)
    P = x.shape[1:]
    v = np.zeros((m,) + P, f)
    for j in range(m):
        acc = np.zeros(P, f)
        for q in range(tab.start[j], tab.start[j + 1]):
            i = int(tab.member[q])
            d = x[i] if clean else x[i] - f(s) * np.asarray(eta[i], f)
            acc = acc + f(tab.w[q]) * d
        r = acc - (y[j] if clean else f(a) * y[j])
        t = np.zeros(P, f)
        for k in range(1, min(bw, j) + 1):
            t = t + lc[j, k] * v[j - k]
        v[j] = (r - t) * lc[j, 0]
    u = np.zeros_like(v)
    for j in range(m - 1, -1, -1):
        t = np.zeros(P, f)
        for k in range(1, bw + 1):
            if j + k < m:
                t = t + lc[j + k, k] * u[j + k]
        u[j] = (v[j] - t) * lc[j, 0]
    out = x.copy()
    for i in range(n):
        if tab.tstart[i] == tab.tstart[i + 1]:
            continue
        c = np.zeros(P, f)
        for q in range(tab.tstart[i], tab.tstart[i + 1]):
            c = c + f(tab.tw[q]) * u[int(tab.tmember[q])]
        out[i] = np.where(c == 0, x[i], x[i] - c)
    return out


# ---------------------------------------------------------------------------------------------------
# rounding bounds: first order in EPS = 2^-24, counting the roundings of the chain
# ---------------------------------------------------------------------------------------------------
def bandwidth(A):
    j, k = np.nonzero(as_kernel(A) @ as_kernel(A).T)
    return int(np.abs(j - k).max())


def cond(A):
    ev = np.linalg.eigvalsh(as_kernel(A) @ as_kernel(A).T)
    return float(ev[-1] / ev[0])


def bound_out(x, y, A, eta=None, a=1.0, s=0.0, clean=True):
    """Per element of `out` [n, P]; +inf on a thin slice under no thick slice (compared bit for bit elsewhere).  With |.| elementwise,
    K_j the members of thick slice j, T_i the thick slices over thin slice i, D = |x| + s |eta|, u = G^-1 r, c = A^T u:
      residual   dr_j = (K_j + 4) EPS (sum_s w_js D_s + a |y_j|): s * eta and the difference (2), K products and K - 1 sums, a * y, acc - ay;
      solve      du = |G^-1| (dr + (2 bw + 8) EPS |L| |L^T| |u|): the two substitutions are backward stable, each row of a
                 substitution rounding bw products, bw sums, one difference and the product with 1 / L_jj (Higham, Accuracy and
                 Stability, Thm 8.5: (T + dT) v = b, |dT| <= gamma_{bw+2} |T|), and the factor's entries and reciprocal diagonal are
                 themselves rounded once (2 EPS |L| per factor); || |G^-1| |L| |L^T| || <= (bw + 1) cond(G), which is where the
                 condition number of G enters;
      scatter    |A^T| du + T_i EPS |A^T| |u| + EPS (|x_i| + |c_i|): T products and T - 1 sums, and the last difference."""
    A, x, y = as_kernel(A), np.asarray(x, np.float64), np.asarray(y, np.float64)
    aa = np.abs(A)
    a_, s_ = (1.0, 0.0) if clean else (float(a), float(s))
    e = 0.0 if clean else np.asarray(eta, np.float64)
    D = np.abs(x) + s_ * np.abs(e)
    K = (A != 0).sum(1).reshape((-1,) + (1,) * (x.ndim - 1))
    T = (A != 0).sum(0).reshape((-1,) + (1,) * (x.ndim - 1))
    G = A @ A.T
    L = np.linalg.cholesky(G)
    bw = bandwidth(A)
    r = A @ (x - s_ * e) - a_ * y
    u = np.linalg.solve(G, r)
    dr = (K + 4) * EPS * (_mat(aa, D) + a_ * np.abs(y))
    du = _mat(np.abs(np.linalg.inv(G)), dr + (2 * bw + 8) * EPS * _mat(np.abs(L) @ np.abs(L.T), np.abs(u)))
    c = _mat(A.T, u)
    out = _mat(aa.T, du) + T * EPS * _mat(aa.T, np.abs(u)) + EPS * (np.abs(x) + np.abs(c))
    out[(A != 0).sum(0) == 0] = np.inf
    return out


def _mat(M, v):
    return np.tensordot(M, v, axes=(1, 0))


def bound_measure(x, A):
    """Per element of A x [m, P] computed in fp32 (mud_band_measure) against fp64: K_j EPS sum_s w_js |x_s| (K products, K - 1 sums)."""
    A, x = np.abs(as_kernel(A)), np.abs(np.asarray(x, np.float64))
    K = (A != 0).sum(1).reshape((-1,) + (1,) * (x.ndim - 1))
    return K * EPS * _mat(A, x)


def bound_residual_norms(x_norm, y_norm, A):
    """The relative form's numerator: per thick slice, a bound on the L2 norm over the pixels of A out - y after the clean step, from the
    L2 norms x_norm [n] of x's thin slices and y_norm [m] of y's thick slices alone.  bound_residual is dominated by a non-negative
    linear map of (|x|, |y|) - |u| <= |G^-1| (|A| |x| + |y|), |c| <= |A^T| |u| - and the L2 norm of a non-negative combination of
    images is at most that combination of their norms.  One more EPS (|A out| + |y|) covers a difference A out - y formed in fp32."""
    A = as_kernel(A)
    aa, xn, yn = np.abs(A), np.asarray(x_norm, np.float64), np.asarray(y_norm, np.float64)
    K, T = (A != 0).sum(1), (A != 0).sum(0)
    G = A @ A.T
    L = np.linalg.cholesky(G)
    gi = np.abs(np.linalg.inv(G))
    r = aa @ xn + yn
    u = gi @ r
    du = gi @ ((K + 4) * EPS * r + (2 * bandwidth(A) + 8) * EPS * (np.abs(L) @ np.abs(L.T) @ u))
    c = aa.T @ u
    out = np.where(T > 0, aa.T @ du + T * EPS * (aa.T @ u) + EPS * (xn + c), 0.0)
    return aa @ out + K * EPS * (aa @ (xn + c)) + EPS * (aa @ (xn + c) + yn)


def bound_residual(x, y, A):
    """Per element of |A out - y| [m, P] after the clean step on x: exactly, A out = y, so what is left is A applied to the error of
    out, |A| bound_out over the covered thin slices, plus the rounding of forming A out in fp32 (bound_measure of |x| + |c|, which
    dominates |out|); a residual formed in fp64 is inside it a fortiori."""
    A_ = as_kernel(A)
    b = bound_out(x, y, A, clean=True)
    b = np.where(np.isfinite(b), b, 0.0)
    x64 = np.asarray(x, np.float64)
    c = x64 - constrain(x, y, A)
    return _mat(np.abs(A_), b) + bound_measure(np.abs(x64) + np.abs(c), A)
