"""fp64 numpy restatement of the accelerated thick-slice path (csrc/slab_kspace.hip, mudiff_hip.multislice), built
on kspace_ref and thick_ref: the measurement y_j = M_eff * F(sum_l w_l k_l), the projection of mud_slab_kspace_constrain, the zero-filled
interpolated baseline, the rounding bound the tests hold the kernel to, and an fp32 / complex64 emulation of the kernel's chain in its
operation order.  Nothing here imports the package."""
import numpy as np

import kspace_ref as KR
import thick_ref as TR

EPS = 2.0 ** -24


def _tables(members, w, g=None):
    members = np.asarray(members)
    members = members.reshape(1, -1) if members.ndim == 1 else members
    w = np.broadcast_to(np.asarray(w, np.float64), members.shape)
    g = None if g is None else np.broadcast_to(np.asarray(g, np.float64), members.shape)
    return members, w, g


def measure(k, members, w, mask):
    """y[j] = mask * F(sum_l w_l k[members[j][l]]): complex128 [groups, S, S].  mask: [1 or groups, S, S]."""
    return KR.measure(TR.average(k, *_tables(members, w)[:2]), mask)


def _level(rows, t, toff, a_tab, s_tab, clean):
    """(a, s) of a group: the level of its first member; clean: (1, 0)."""
    if clean:
        return 1.0, 0.0
    c = int(np.clip(int(np.asarray(t)[rows[0][1]]) + int(toff), 0, len(a_tab) - 1))
    return float(np.asarray(a_tab, np.float64)[c]), float(np.asarray(s_tab, np.float64)[c])


def constrain(x_new, y, mask, members, w, g, eta, t, toff, a_tab, s_tab, clean):
    """d = sum_l w_l (x_l - s eta_l), R = mask ? F(d) - a y_j : 0, x_l <- x_l - g_l Re F^H R for the members of every group (the level
    of a, s: the first member's); a row of no group is returned as it is.  fp64 from the fp32 operands; x_new: [rows, S, S]."""
    x_new = np.asarray(x_new, np.float64)
    members, w, g = _tables(members, w, g)
    mask = np.asarray(mask) != 0
    out = x_new.copy()
    for j, row in enumerate(members):
        rows = [(l, m) for l, m in enumerate(row) if m >= 0]
        a, s = _level(rows, t, toff, a_tab, s_tab, clean)
        d = np.zeros(x_new.shape[1:])
        for l, m in rows:
            d = d + w[j, l] * (x_new[m] - (0.0 if clean else s * np.asarray(eta, np.float64)[m]))
        r = np.where(mask[0 if mask.shape[0] == 1 else j], KR.fft2(d) - a * np.asarray(y, np.complex128)[j], 0.0)
        c = KR.fft2(r, inverse=True).real
        for l, m in rows:
            out[m] = x_new[m] - g[j, l] * c
    return out


def _l2(a):
    return np.sqrt((np.abs(np.asarray(a)).astype(np.float64) ** 2).sum((-2, -1)))


def bound(x_new, y, members, w, g, eta, t, toff, a_tab, s_tab, clean):
    """Per member row, in L2 over the image:
        g_l (3 rule(S) + (L + 4) 2^-24) (sum_m w_m (|x_m| + s |eta_m|) + a |y|) + 2^-24 |x_l|,
    +inf on a free row (compared bit for bit elsewhere).  3 rule(S): the two transforms and the residual between them, kspace's bound;
    (L + 4) 2^-24: the roundings of the accumulation, s * eta, a * y and g * c, thick's count; 2^-24 |x_l|: the last difference."""
    S = np.asarray(x_new).shape[-1]
    members, w, g = _tables(members, w, g)
    nx, ne, ny = _l2(x_new), (None if eta is None else _l2(eta)), _l2(y)
    out = np.full(np.asarray(x_new).shape[0], np.inf)
    for j, row in enumerate(members):
        rows = [(l, m) for l, m in enumerate(row) if m >= 0]
        a, s = _level(rows, t, toff, a_tab, s_tab, clean)
        tot = a * ny[j]
        for l, m in rows:
            tot = tot + w[j, l] * (nx[m] + (0.0 if clean else s * ne[m]))
        for l, m in rows:
            out[m] = g[j, l] * (3 * KR.rule(S) + (len(rows) + 4) * EPS) * tot + EPS * nx[m]
    return out


def baseline(y, starts, L, n):
    """The zero-filled baseline: Re F^H y_j per slab, interpolated linearly along z as thick_ref.interpolate does: fp64 [n, S, S]."""
    return TR.interpolate(KR.fft2(np.asarray(y, np.complex128), inverse=True).real, starts, L, n)


# ---- the kernel's chain in fp32 --------------------------------------------------------------------------------------------------------
def _cmul(ar, ai, br, bi):
    """(ar + i ai)(br + i bi), the four products and the two sums each rounded once to fp32 (kspace_fft.h: ks_mul)."""
    return ar * br - ai * bi, ar * bi + ai * br


def _lines_f32(re, im, inverse):
    """Unscaled DFT of the last axis in fp32: radix-2 decimation in frequency with twiddles correctly rounded from fp64 (log2 S layers,
    the layer count of the kernel's radix-4 passes), then the bit reversal undone."""
    S = re.shape[-1]
    logS = S.bit_length() - 1
    ang = -2.0 * np.pi * np.arange(S // 2) / S
    twr, twi = np.cos(ang).astype(np.float32), (np.sin(ang) * (-1.0 if inverse else 1.0)).astype(np.float32)
    re, im = re.astype(np.float32).copy(), im.astype(np.float32).copy()
    lead = re.shape[:-1]
    for layer in range(logS):
        h = S >> (layer + 1)                                                           # half the span
        vr, vi = re.reshape(lead + (-1, 2, h)), im.reshape(lead + (-1, 2, h))
        ar, ai, br, bi = vr[..., 0, :], vi[..., 0, :], vr[..., 1, :], vi[..., 1, :]
        sr, si, dr, di = ar + br, ai + bi, ar - br, ai - bi
        wr, wi = twr[:: 1 << layer][:h], twi[:: 1 << layer][:h]
        pr, pi = _cmul(dr, di, wr, wi)
        re, im = np.stack([sr, pr], -2).reshape(lead + (S,)), np.stack([si, pi], -2).reshape(lead + (S,))
    rev = np.array([int(format(v, f'0{logS}b')[::-1], 2) for v in range(S)])
    return re[..., rev], im[..., rev]


def fft2_f32(re, im, inverse=False):
    """Unitary 2D DFT of [S, S] in fp32: rows, columns, then the exact scale 1/S once."""
    re, im = _lines_f32(re, im, inverse)
    re, im = _lines_f32(re.T, im.T, inverse)
    s = np.float32(1.0 / re.shape[-1])
    return (re.T * s).astype(np.float32), (im.T * s).astype(np.float32)


def emulate_fp32(x_new, y, mask, w, g, eta, a, s, clean):
    """The kernel's chain for one group whose members are rows 0..L-1 of x_new [L, S, S], in numpy fp32, every product and sum rounded
    once, in the kernel's order: acc = acc + w * (x - s * eta) from 0, F, mask ? D - a * y : 0, F^H, out = x - g * Re(.)."""
    f = np.float32
    x_new, eta = np.asarray(x_new, f), None if eta is None else np.asarray(eta, f)
    y = np.asarray(y, np.complex64)
    acc = np.zeros(x_new.shape[1:], f)
    for l in range(x_new.shape[0]):
        d = x_new[l] if clean else x_new[l] - f(s) * eta[l]
        acc = acc + f(w[l]) * d
    Dr, Di = fft2_f32(acc, np.zeros_like(acc))
    ar, ai = (y.real, y.imag) if clean else (f(a) * y.real, f(a) * y.imag)
    m = np.asarray(mask).reshape(acc.shape) != 0
    rr, ri = np.where(m, Dr - ar, f(0)), np.where(m, Di - ai, f(0))
    c = fft2_f32(rr, ri, inverse=True)[0]
    return np.stack([x_new[l] - f(g[l]) * c for l in range(x_new.shape[0])]).astype(f)
