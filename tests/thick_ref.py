"""fp64 numpy restatement of the thick-slice path (csrc/slab.hip, mudiff_hip.thick): the layout, the profile, the
measurement y_j = sum_l w_l k_{z_j + l}, the projection of mud_slab_constrain, the interpolated baseline, and the two rounding bounds
the GPU tests hold the kernel to.  Nothing here imports the package."""
import math

import numpy as np

EPS = 2.0 ** -24


def layout(Z, L, gap=0, offset=0):
    """[(first, last, complete)]: slab j starts at offset + j (L + gap); the volume may cut the last one short."""
    out, z = [], offset
    while z < Z:
        out.append((z, min(z + L - 1, Z - 1), z + L - 1 <= Z - 1))
        z += L + gap
    return out


def profile(L, kind='box'):
    """fp64 [L], positive, sum 1.  gauss: FWHM = L slices."""
    if kind == 'box':
        w = np.full(L, 1.0)
    else:
        c = (L - 1) / 2.0
        w = np.array([math.exp(-4.0 * math.log(2.0) * (min(l, L - 1 - l) - c) ** 2 / (L * L)) for l in range(L)])
    return w / w.sum()


def gains(w):
    """g_l = w_l / sum_m w_m^2 in fp64 from the fp32 weights, rounded once to fp32 (what the caller hands the kernel)."""
    w = np.asarray(w, np.float32).astype(np.float64)
    return (w / (w * w).sum()).astype(np.float32)


def average(x, members, w):
    """avg[j] = sum_l w_l x[members[j][l]] over the members >= 0, fp64 from the fp32 operands.  w: [L] or [groups, L]."""
    x, members = np.asarray(x, np.float64), np.asarray(members)
    w = np.broadcast_to(np.asarray(w, np.float64), members.shape)
    out = np.zeros((members.shape[0],) + x.shape[1:])
    for j, row in enumerate(members):
        for l, m in enumerate(row):
            if m >= 0:
                out[j] += w[j, l] * x[m]
    return out


def constrain(x_new, y, members, w, g, eta, t, toff, a_tab, s_tab, clean):
    """r = sum_l w_l (x_new_l - s eta_l) - a y_j, x_l <- x_new_l - g_l r for the members of every group (the level of a, s: the first
    member's); a row of no group is returned as it is.  fp64 from the fp32 operands."""
    x_new, members = np.asarray(x_new, np.float64), np.asarray(members)
    w = np.broadcast_to(np.asarray(w, np.float64), members.shape)
    g = np.broadcast_to(np.asarray(g, np.float64), members.shape)
    out = x_new.copy()
    for j, row in enumerate(members):
        rows = [(l, m) for l, m in enumerate(row) if m >= 0]
        a, s = 1.0, 0.0
        if not clean:
            c = int(np.clip(int(np.asarray(t)[rows[0][1]]) + int(toff), 0, len(a_tab) - 1))
            a, s = float(np.asarray(a_tab, np.float64)[c]), float(np.asarray(s_tab, np.float64)[c])
        r = -a * np.asarray(y, np.float64)[j]
        for l, m in rows:
            r = r + w[j, l] * (x_new[m] - (0.0 if clean else s * np.asarray(eta, np.float64)[m]))
        for l, m in rows:
            out[m] = x_new[m] - g[j, l] * r
    return out


def bound_out(x_new, y, members, w, g, eta, t, toff, a_tab, s_tab, clean):
    """Per element of every member row: (L + 4) 2^-24 (|x_new_l| + g_l (sum_m w_m (|x_new_m| + s |eta_m|) + a |y|)); +inf on a free row
    (compared bit for bit elsewhere).  It counts the roundings of the chain: L products and L - 1 sums of the accumulation, s * eta and
    the difference, a * y, the residual, g * r and the last difference."""
    x_new, members = np.abs(np.asarray(x_new, np.float64)), np.asarray(members)
    w = np.broadcast_to(np.asarray(w, np.float64), members.shape)
    g = np.broadcast_to(np.asarray(g, np.float64), members.shape)
    out = np.full(x_new.shape, np.inf)
    for j, row in enumerate(members):
        rows = [(l, m) for l, m in enumerate(row) if m >= 0]
        a, s = 1.0, 0.0
        if not clean:
            c = int(np.clip(int(np.asarray(t)[rows[0][1]]) + int(toff), 0, len(a_tab) - 1))
            a, s = float(np.asarray(a_tab, np.float64)[c]), float(np.asarray(s_tab, np.float64)[c])
        tot = a * np.abs(np.asarray(y, np.float64)[j])
        for l, m in rows:
            tot = tot + w[j, l] * (x_new[m] + (0.0 if clean else s * np.abs(np.asarray(eta, np.float64)[m])))
        for l, m in rows:
            out[m] = (len(rows) + 4) * EPS * (x_new[m] + g[j, l] * tot)
    return out


def bound_residual(x_new, y, members, w):
    """Per element of every group, after the clean step: (L + 4) 2^-24 (sum_l w_l |x_new_l| + |y|)."""
    n = (np.asarray(members) >= 0).sum(1).reshape((-1,) + (1,) * (np.asarray(x_new).ndim - 1))
    return (n + 4) * EPS * (average(np.abs(np.asarray(x_new, np.float64)), members, w) + np.abs(np.asarray(y, np.float64)))


def emulate_fp32(x_new, y, w, g, eta, a, s, clean):
    """The kernel's chain for one group whose members are rows 0..L-1 of x_new, in numpy fp32, every product and sum rounded once."""
    f = np.float32
    x_new, y, eta = np.asarray(x_new, f), np.asarray(y, f), None if eta is None else np.asarray(eta, f)
    acc = np.zeros_like(y)
    for l in range(x_new.shape[0]):
        d = x_new[l] if clean else x_new[l] - f(s) * eta[l]
        acc = acc + f(w[l]) * d
    r = acc - (y if clean else f(a) * y)
    return np.stack([x_new[l] - f(g[l]) * r for l in range(x_new.shape[0])])


def interpolate(y, starts, L, n):
    """[n, ...]: piecewise linear along z through (starts[j] + (L - 1) / 2, y[j]), constant beyond the first and the last centre."""
    y = np.asarray(y, np.float64)
    c = np.asarray(starts, np.float64) + (L - 1) / 2.0
    out = np.empty((n,) + y.shape[1:])
    for z in range(n):
        if z <= c[0]:
            out[z] = y[0]
        elif z >= c[-1]:
            out[z] = y[-1]
        else:
            j = int(np.searchsorted(c, z, side='right')) - 1
            f = (z - c[j]) / (c[j + 1] - c[j])
            out[z] = (1.0 - f) * y[j] + f * y[j + 1]
    return out
