"""numpy restatements of the low-resolution-volume path (csrc/lowres.hip, mudiff_hip.lowres_volume): the
projection x - A^T (A A^T)^-1 (A (x - s eta) - a y) for A = A_z (x) A_y (x) A_x
 (a) `constrain_dense`: fp64, A built explicitly by np.kron, one dense solve;
 (b) `constrain_separable`: fp64, one solve per axis (what the factorisation A A^T = G_z (x) G_y (x) G_x promises);
 (c) `constrain_fp32`: the kernels' four passes in numpy fp32, every product and sum rounded once, in the tables' order.
The per-axis weights are band_ref's (`row`, `weights`).  Nothing here imports the package; (c) takes the tables of ops.lowres_tables as
an object with attributes z, y, x, each with ops.band_tables' attributes."""
import numpy as np

from band_ref import as_kernel

EPS32 = 2.0 ** -23


def kron3(A_z, A_y, A_x):
    """A = A_z (x) A_y (x) A_x [m_z m_y m_x, n H W] from the weights as the kernel sees them (rounded once to fp32)."""
    return np.kron(np.kron(as_kernel(A_z), as_kernel(A_y)), as_kernel(A_x))


def measure_dense(x, A_z, A_y, A_x):
    """A x in fp64: x [n, H, W] -> [m_z, m_y, m_x]."""
    return (kron3(A_z, A_y, A_x) @ np.asarray(x, np.float64).reshape(-1)).reshape(A_z.shape[0], A_y.shape[0], A_x.shape[0])


def _residual_operands(x, y, eta, a, s, clean):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x if clean else x - float(s) * np.asarray(eta, np.float64)
    return x, d, (1.0 if clean else float(a)) * y


def constrain_dense(x, y, A_z, A_y, A_x, eta=None, a=1.0, s=0.0, clean=True):
    """(a): x, eta [n, H, W]; y [m_z, m_y, m_x] -> fp64 [n, H, W]."""
    x, d, ay = _residual_operands(x, y, eta, a, s, clean)
    A = kron3(A_z, A_y, A_x)
    r = A @ d.reshape(-1) - ay.reshape(-1)
    return x - (A.T @ np.linalg.solve(A @ A.T, r)).reshape(x.shape)


def _along(M, v, axis):
    """M applied along `axis` of v."""
    return np.moveaxis(np.tensordot(M, v, axes=(1, axis)), 0, axis)


def constrain_separable(x, y, A_z, A_y, A_x, eta=None, a=1.0, s=0.0, clean=True):
    """(b): measure axis by axis, solve G_z, G_y, G_x one after the other, scatter axis by axis."""
    x, d, ay = _residual_operands(x, y, eta, a, s, clean)
    mats = [as_kernel(M) for M in (A_z, A_y, A_x)]
    r = d
    for axis, M in enumerate(mats):
        r = _along(M, r, axis)
    u = r - ay
    for axis, M in enumerate(mats):
        u = _along(np.linalg.inv(M @ M.T), u, axis)
    for axis, M in enumerate(mats):
        u = _along(M.T, u, axis)
    return x - u


def null_basis(A_z, A_y, A_x):
    """An orthonormal fp64 basis [n H W, k] of the null space of A."""
    A = kron3(A_z, A_y, A_x)
    _, sv, vt = np.linalg.svd(A, full_matrices=True)
    rank = int((sv > sv[0] * 1e-12).sum())
    return vt[rank:].T


# ---------------------------------------------------------------------------------------------------
# (c) the kernels' chain in fp32
# ---------------------------------------------------------------------------------------------------
f32 = np.float32


def _gather_fp32(v, tab, axis):
    """sum_s w_js v[member_js] along `axis`, from 0 in table order (passes 1 and 2)."""
    v = np.moveaxis(v, axis, 0)
    out = np.zeros((tab.m,) + v.shape[1:], f32)
    for j in range(tab.m):
        acc = np.zeros(v.shape[1:], f32)
        for q in range(tab.start[j], tab.start[j + 1]):
            acc = acc + f32(tab.w[q]) * v[int(tab.member[q])]
        out[j] = acc
    return np.moveaxis(out, 0, axis)


def _scatter_fp32(u, tab, axis):
    """sum_j tw_ji u[j] along `axis`, from 0 with j ascending (pass 4); 0 where nothing covers."""
    u = np.moveaxis(u, axis, 0)
    out = np.zeros((tab.n,) + u.shape[1:], f32)
    for i in range(tab.n):
        c = np.zeros(u.shape[1:], f32)
        for q in range(tab.tstart[i], tab.tstart[i + 1]):
            c = c + f32(tab.tw[q]) * u[int(tab.tmember[q])]
        out[i] = c
    return np.moveaxis(out, 0, axis)


def _solve_fp32(r, tab, axis):
    """The banded forward and backward substitution with tab.lc along `axis` (passes 2 and 3)."""
    r = np.moveaxis(r, axis, 0)
    m, bw = tab.m, tab.bw
    lc = np.asarray(tab.lc, f32).reshape(m, bw + 1)
    v = np.zeros_like(r)
    for j in range(m):
        t = np.zeros(r.shape[1:], f32)
        for k in range(1, min(bw, j) + 1):
            t = t + lc[j, k] * v[j - k]
        v[j] = (r[j] - t) * lc[j, 0]
    u = np.zeros_like(r)
    for j in range(m - 1, -1, -1):
        t = np.zeros(r.shape[1:], f32)
        for k in range(1, bw + 1):
            if j + k < m:
                t = t + lc[j + k, k] * u[j + k]
        u[j] = (v[j] - t) * lc[j, 0]
    return np.moveaxis(u, 0, axis)


def measure_fp32(x, tabs):
    """mud_lowres_measure's chain: along y, then x, then z."""
    return _gather_fp32(_gather_fp32(_gather_fp32(np.asarray(x, f32), tabs.y, 1), tabs.x, 2), tabs.z, 0)


def constrain_fp32(x, y, tabs, eta=None, a=1.0, s=0.0, clean=True):
    """(c): x, eta [n, H, W] fp32; y [m_z, m_y, m_x] fp32 -> fp32 [n, H, W]."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    d = x if clean else x - f32(s) * np.asarray(eta, f32)
    P = _gather_fp32(_gather_fp32(d, tabs.y, 1), tabs.x, 2)                       # 1. in-plane measure
    r = _gather_fp32(P, tabs.z, 0) - (y if clean else f32(a) * y)                # 2. z measure ...
    u = _solve_fp32(r, tabs.z, 0)                                                #    ... and solve
    u = _solve_fp32(_solve_fp32(u, tabs.y, 1), tabs.x, 2)                        # 3. in-plane solves
    c = _scatter_fp32(_scatter_fp32(_scatter_fp32(u, tabs.x, 2), tabs.y, 1), tabs.z, 0)      # 4. scatter: x innermost, z outermost
    return np.where(c == 0, x, x - c)
