"""numpy restatement of the known-region kernels (csrc/known_region.hip): mud_known_constrain's select of the
forward-diffused known values (fp32 mul, mul, add, each rounded once, and np.where), mud_known_coverage's in-bounds test of a resampling
matrix in fp64, and the composition of the known region on the prediction grid that mudiff_hip.known_region performs."""
import numpy as np

import ensemble_ref as E

KIND_KNOWN, KIND_RENOISE = 3, 4


def constrain(x_new, known, mask, eta, t, toff, a_tab, s_tab, clean=False):
    """[rows, row_len] arrays -> float32 [rows, row_len].  mask None: known everywhere (x_new unused)."""
    known = np.asarray(known, np.float32)
    rows = known.shape[0]
    if clean:
        q = known
    else:
        a_tab, s_tab = np.asarray(a_tab, np.float32), np.asarray(s_tab, np.float32)
        c = np.clip(np.asarray(t, np.int64) + int(toff), 0, len(a_tab) - 1)
        a, s = a_tab[c].reshape(rows, 1), s_tab[c].reshape(rows, 1)
        with np.errstate(invalid='ignore', over='ignore'):
            p0 = (a * known).astype(np.float32)
            p1 = (s * np.asarray(eta, np.float32)).astype(np.float32)
            q = (p0 + p1).astype(np.float32)
    if mask is None:
        return q.copy()
    return np.where(np.asarray(mask) != 0, q, np.asarray(x_new, np.float32))


def keyed_eta(keys, row_len, seed, step, kind):
    return E.randn_keyed(keys, row_len, seed, step, kind)


def source_coordinates(M, out_shape):
    """p[a][i, j, k] = ((m[a,0] * i + m[a,1] * j) + m[a,2] * k) + m[a,3] in fp64, every product and sum rounded once."""
    m = np.asarray(M, np.float64)[:3, :4]
    X, Y, Z = out_shape
    i, j, k = np.meshgrid(np.arange(X, dtype=np.float64), np.arange(Y, dtype=np.float64), np.arange(Z, dtype=np.float64), indexing='ij')
    return [((m[a, 0] * i + m[a, 1] * j) + m[a, 2] * k) + m[a, 3] for a in range(3)]


def coverage(M, src_shape, out_shape):
    """uint8 [X, Y, Z]: 1 where 0 <= p_a <= S_a - 1 on every axis."""
    p = source_coordinates(M, out_shape)
    ok = np.ones(tuple(out_shape), bool)
    for a in range(3):
        ok &= (p[a] >= 0.0) & (p[a] <= float(src_shape[a] - 1))
    return ok.astype(np.uint8)


def near_a_bound(M, src_shape, out_shape, eps=1e-9):
    """bool [X, Y, Z]: some p_a lies within eps of 0 or S_a - 1 (where a last-bit difference of p could flip the test)."""
    p = source_coordinates(M, out_shape)
    near = np.zeros(tuple(out_shape), bool)
    for a in range(3):
        near |= (np.abs(p[a]) <= eps) | (np.abs(p[a] - float(src_shape[a] - 1)) <= eps)
    return near


def compose(coverage_xyz, known_xyz, trust_xyz, drop, s0, s1):
    """The known region on the prediction grid, [X, Y, Z] bool: coverage AND K finite AND (trust != 0 when given) AND the slice is not in
    one of the inclusive (a, b) ranges of `drop` AND s0 <= slice <= s1."""
    ok = (np.asarray(coverage_xyz) != 0) & np.isfinite(known_xyz)
    if trust_xyz is not None:
        ok &= np.asarray(trust_xyz) != 0
    for z in range(ok.shape[2]):
        if z < s0 or z > s1 or any(a <= z <= b for a, b in drop):
            ok[:, :, z] = False
    return ok
