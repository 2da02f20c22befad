"""numpy restatement of the slice-coupled keyed draws (csrc/ensemble.hip: mud_randn_keyed_coupled) on top of tests/ensemble_ref.py, and of
the through-plane sums (csrc/volume_through_plane.hip: mud_volume_through_plane).  DESIGN.md section 5.23."""
import math

import numpy as np

import ensemble_ref as E


def taps(sigma):
    """(half taps w_0..w_R, R): R = ceil(3 sigma), w_j ~ exp(-j^2 / (2 sigma^2)), the square sum over j = -R..R equal to 1."""
    R = int(math.ceil(3.0 * sigma))
    w = [math.exp(-(j * j) / (2.0 * sigma * sigma)) for j in range(R + 1)]
    norm = math.sqrt(w[0] * w[0] + 2.0 * math.fsum(v * v for v in w[1:]))
    return np.array([v / norm for v in w], np.float64), R


def correlation(half, lag):
    """sum_j w_j w_{j+lag} over the full taps j = -R..R."""
    full = np.concatenate([half[:0:-1], half])
    lag = abs(int(lag))
    return 0.0 if lag >= full.size else float(np.sum(full[:full.size - lag] * full[lag:]))


class WhiteNoise:
    """eta(slice, sample) rows of E.randn_keyed under one (row_len, seed, step, kind), each computed once; the slice wraps modulo 2^64."""

    def __init__(self, row_len, seed, step, kind):
        self.args, self.rows = (row_len, seed, step, kind), {}

    def row(self, slice_, sample):
        key = (slice_ & E.M64, sample)
        if key not in self.rows:
            row_len, seed, step, kind = self.args
            out = np.empty(row_len, np.float64)
            k = E.key(seed)
            for b in range((row_len + 3) // 4):
                v = E.block_normals(E.philox4x64(E.counter(b, key[0], sample, step, kind), k))
                n = min(4, row_len - 4 * b)
                out[4 * b:4 * b + n] = v[:n]
            self.rows[key] = out.astype(np.float32)
        return self.rows[key]


def randn_keyed_coupled(keys, row_len, seed, step, kind, half, R, noise=None):
    """keys [rows][2] = (slice, sample) -> float32 [rows, row_len]: fp32(sum_{j=-R..R} half[|j|] * eta(slice + j)), the products and the
    sum in fp64 in tap order, eta the fp32 rows of E.randn_keyed."""
    noise = noise or WhiteNoise(row_len, seed, step, kind)
    keys = np.asarray(keys, np.int64).reshape(-1, 2)
    out = np.empty((len(keys), row_len), np.float32)
    for r, (s, m) in enumerate(keys.tolist()):
        acc = np.zeros(row_len, np.float64)
        for j in range(-R, R + 1):
            acc = acc + np.float64(half[abs(j)]) * noise.row(s + j, m).astype(np.float64)
        out[r] = acc.astype(np.float32)
    return out


def through_plane_sums(vol, mask=None, z0=0, z1=None):
    """[Z, X, Y] fp32 volume, optional mask (non-zero: inside) -> float64 [z1 - z0 + 1, 8]: per plane (N_DZ, S_DZ, N_DZZ, S_DZZ, N_DX, S_DX,
    N_DY, S_DY), the fp64 differences of the fp32 values; planes outside z0..z1 do not take part."""
    v = np.asarray(vol, np.float32).astype(np.float64)
    Z = v.shape[0]
    z0, z1 = max(0, z0), Z - 1 if z1 is None else min(Z - 1, z1)
    v = v[z0:z1 + 1]
    m = np.ones(v.shape, bool) if mask is None else np.asarray(mask)[z0:z1 + 1] != 0
    P = v.shape[0]
    out = np.zeros((P, 8), np.float64)
    for z in range(P):
        if z + 1 < P:
            both = m[z] & m[z + 1]
            out[z, 0], out[z, 1] = both.sum(), np.abs(v[z + 1] - v[z])[both].sum()
        if 0 < z < P - 1:
            three = m[z - 1] & m[z] & m[z + 1]
            out[z, 2], out[z, 3] = three.sum(), np.abs((v[z + 1] - 2.0 * v[z]) + v[z - 1])[three].sum()
        bx = m[z, :-1, :] & m[z, 1:, :]
        out[z, 4], out[z, 5] = bx.sum(), np.abs(v[z, 1:, :] - v[z, :-1, :])[bx].sum()
        by = m[z, :, :-1] & m[z, :, 1:]
        out[z, 6], out[z, 7] = by.sum(), np.abs(v[z, :, 1:] - v[z, :, :-1])[by].sum()
    return out


def through_plane(vol, mask=None, z0=0, z1=None):
    """The report's numbers from through_plane_sums: dict(mean_dz, mean_dzz, mean_dx, mean_dy, anisotropy, dz)."""
    s = through_plane_sums(vol, mask, z0, z1)
    tot = np.zeros(8)
    for row in s:
        tot = tot + row
    mean = lambda a, n: a / n if n else None      # noqa: E731
    r = dict(mean_dz=mean(tot[1], tot[0]), mean_dzz=mean(tot[3], tot[2]), mean_dx=mean(tot[5], tot[4]), mean_dy=mean(tot[7], tot[6]))
    inplane = None if r['mean_dx'] is None or r['mean_dy'] is None else (r['mean_dx'] + r['mean_dy']) / 2
    r['anisotropy'] = r['mean_dz'] / inplane if r['mean_dz'] is not None and inplane else None
    r['dz'] = [mean(row[1], row[0]) for row in s[:-1]]
    return r
