"""fp64 numpy restatement of the multi-coil path (csrc/sense.hip, mudiff_hip.sense): the default coil maps, the
measurement A x = (M F(C_c x))_c, its adjoint, N = A^H A, and the data-consistency step of mud_sense_constrain with the same
conjugate-gradient recurrence and the same guards.  Nothing here imports the package."""
import numpy as np

from kspace_ref import fft2


def coil_maps(S, Nc):
    """The smooth synthetic sensitivities of the issue: complex128 [Nc, S, S] with unit root-sum-of-squares."""
    g = (np.arange(S) - S // 2) / S
    u, v = np.meshgrid(g, g, indexing='ij')
    theta = 2 * np.pi * (np.arange(Nc) + 0.5) / Nc
    ct, st = np.cos(theta)[:, None, None], np.sin(theta)[:, None, None]
    m = np.exp(-((u - 0.75 * ct) ** 2 + (v - 0.75 * st) ** 2) / (2 * 0.6 ** 2))
    phi = theta[:, None, None] + np.pi * (u * ct + v * st)
    return m * np.exp(1j * phi) / np.sqrt((m ** 2).sum(0))


def _maps_of(maps, rows):
    maps = np.asarray(maps).astype(np.complex128)
    return np.broadcast_to(maps[None] if maps.ndim == 3 else maps, (rows,) + maps.shape[-3:])


def _mask_of(mask, rows):
    mask = np.asarray(mask) != 0
    return np.broadcast_to(mask, (rows,) + mask.shape[-2:])[:, None]


def measure(x, maps, mask):
    """y = M F(C_c x): x real [rows, S, S], maps [Nc, S, S] or [1 or rows, Nc, S, S], mask [1 or rows, S, S] -> complex128 [rows, Nc, S, S]."""
    x = np.asarray(x, np.float64)
    return np.where(_mask_of(mask, x.shape[0]), fft2(_maps_of(maps, x.shape[0]) * x[:, None]), 0.0)


def adjoint(y, maps):
    """Re sum_c conj(C_c) F^H y_c: [rows, Nc, S, S] -> real [rows, S, S]."""
    y = np.asarray(y).astype(np.complex128)
    return (np.conj(_maps_of(maps, y.shape[0])) * fft2(y, inverse=True)).sum(1).real


def normal(x, maps, mask):
    """N x = A^H A x."""
    return adjoint(measure(x, maps, mask), maps)


def dense_normal(maps, mask):
    """N of one slice as a real [S^2, S^2] matrix, column by column."""
    S = np.asarray(maps).shape[-1]
    eye = np.eye(S * S).reshape(S * S, S, S)
    return normal(eye, maps, mask).reshape(S * S, S * S).T


def levels(rows, t, toff, a_tab, s_tab, clean):
    """(a, s) per row: the tables at clamp(t + toff); clean: (1, 0)."""
    if clean:
        return np.ones(rows), np.zeros(rows)
    c = np.clip(np.asarray(t, np.int64) + int(toff), 0, len(a_tab) - 1)
    return np.asarray(a_tab, np.float64)[c], np.asarray(s_tab, np.float64)[c]


def rhs(x_new, ahy, maps, mask, eta, a, s):
    """b = N (x_new - s eta) - a A^H y."""
    x_new = np.asarray(x_new, np.float64)
    d = x_new if eta is None else x_new - s[:, None, None] * np.asarray(eta, np.float64)
    return normal(d, maps, mask) - a[:, None, None] * np.asarray(ahy, np.float64)


def cg(b, maps, mask, lam, iters):
    """(I + lam N) e = b by `iters` conjugate-gradient steps from e = 0, every scalar per row.  A row whose r.r is exactly 0 (b = 0
    included) or whose p.q is 0 is frozen from then on.  -> (e, |r_iters| / |b| per row, 0 for a frozen row)."""
    dot = lambda u, v: (u * v).sum((1, 2))                                               # noqa: E731
    rows = b.shape[0]
    e, r, p = np.zeros_like(b), b.copy(), b.copy()
    rr, bb = dot(r, r), dot(b, b)
    frozen = np.zeros(rows, bool)
    for _ in range(int(iters)):
        q = p + lam * normal(p, maps, mask)
        pq = dot(p, q)
        frozen |= (rr == 0) | (pq == 0)
        alpha = np.where(frozen, 0.0, rr / np.where(frozen, 1.0, pq))
        e = e + alpha[:, None, None] * p
        r = r - alpha[:, None, None] * q
        rr_new = np.where(frozen, 0.0, dot(r, r))
        beta = np.where(rr_new == 0, 0.0, rr_new / np.where(rr == 0, 1.0, rr))
        p = r + beta[:, None, None] * p
        rr = rr_new
    res = np.where((rr == 0) | (bb == 0), 0.0, np.sqrt(rr / np.where(bb == 0, 1.0, bb)))
    return e, res


def constrain(x_new, ahy, maps, mask, lam, iters, eta, t, toff, a_tab, s_tab, clean, with_res=False):
    """x = x_new - lam e, the step of mud_sense_constrain, in fp64 from the fp32 operands."""
    x_new = np.asarray(x_new, np.float64)
    a, s = levels(x_new.shape[0], t, toff, a_tab, s_tab, clean)
    b = rhs(x_new, ahy, maps, mask, None if clean else eta, a, s)
    e, res = cg(b, maps, mask, float(lam), iters)
    out = x_new - float(lam) * e
    return (out, res) if with_res else out


def constrain_dense(x_new, ahy, maps, mask, lam, eta, a, s):
    """The same step of ONE slice with a dense solve of (I + lam N): x_new, ahy, eta [S, S]; maps [Nc, S, S]; mask [S, S]."""
    S = x_new.shape[-1]
    N = dense_normal(maps, mask[None])
    d = np.asarray(x_new, np.float64) - s * np.asarray(eta, np.float64)
    b = N @ d.reshape(-1) - a * np.asarray(ahy, np.float64).reshape(-1)
    e = np.linalg.solve(np.eye(S * S) + lam * N, b)
    return np.asarray(x_new, np.float64) - lam * e.reshape(S, S)


def optimality(x, x_new, ahy, maps, mask, lam, eta, a, s):
    """|(x - x_new) + lam (N (x - s eta) - a A^H y)| / |lam b| per row: 0 at the exact minimiser."""
    x, x_new = np.asarray(x, np.float64), np.asarray(x_new, np.float64)
    n = lambda v: np.sqrt((v * v).sum((1, 2)))                                           # noqa: E731
    b = rhs(x_new, ahy, maps, mask, eta, a, s)
    g = (x - x_new) + lam * rhs(x, ahy, maps, mask, eta, a, s)
    return n(g) / np.maximum(lam * n(b), 1e-300)
