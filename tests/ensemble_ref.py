"""numpy restatement of the ensemble kernels (csrc/ensemble.hip): the keyed Philox4x64-10 Gaussian draws of mud_randn_keyed and the
fp64 per-pixel mean / spread of mud_ensemble_stats.  Plain python integers for the 64-bit words, so the
restatement is independent of numpy's generator; tests check its raw words against numpy.random.Philox."""
import math

import numpy as np

M64 = (1 << 64) - 1
PHILOX_M0, PHILOX_M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
PHILOX_W0, PHILOX_W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
KEY_HI = 0x4D55444946460001
KIND_X, KIND_Z, KIND_NOISE = 0, 1, 2


def philox4x64(ctr, key, rounds=10):
    """Random123 philox4x64_R: counter (4 words), key (2 words) -> 4 words."""
    c0, c1, c2, c3 = (int(v) & M64 for v in ctr)
    k0, k1 = (int(v) & M64 for v in key)
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + PHILOX_W0) & M64, (k1 + PHILOX_W1) & M64
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> 64, p0 & M64, p1 >> 64, p1 & M64
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def counter(block, slice_, sample, step, kind):
    return block, slice_, ((sample << 32) | (step << 8) | kind) & M64, 0


def key(seed):
    return int(seed) & M64, KEY_HI


def block_normals(words):
    """4 words -> the block's 4 normals (fp64, before the one rounding to fp32): (w0, w1) -> lanes 0, 1; (w2, w3) -> lanes 2, 3."""
    out = []
    for wa, wb in ((words[0], words[1]), (words[2], words[3])):
        u1 = ((wa >> 11) + 1) * 2.0 ** -53
        u2 = (wb >> 11) * 2.0 ** -53
        r = math.sqrt(-2.0 * math.log(u1))
        th = 6.283185307179586 * u2
        out += [r * math.cos(th), r * math.sin(th)]
    return out


def randn_keyed(keys, row_len, seed, step, kind):
    """keys [rows][2] = (slice, sample) -> float32 [rows, row_len] (each value computed in fp64, rounded once)."""
    keys = np.asarray(keys, np.int64).reshape(-1, 2)
    out = np.empty((len(keys), row_len), np.float64)
    k = key(seed)
    for r, (s, j) in enumerate(keys.tolist()):
        for b in range((row_len + 3) // 4):
            v = block_normals(philox4x64(counter(b, s, j, step, kind), k))
            n = min(4, row_len - 4 * b)
            out[r, 4 * b:4 * b + n] = v[:n]
    return out.astype(np.float32)


def premap(x, scale=1.0, shift=0.0, lo=-np.inf, hi=np.inf):
    """clamp(x*scale + shift, lo, hi): the multiply and the add each rounded once in fp32 (no fused multiply-add); NaN stays NaN."""
    x = np.asarray(x, np.float32)
    y = x * np.float32(scale)
    y = y + np.float32(shift)
    return np.clip(y, np.float32(lo), np.float32(hi))


def ensemble_stats(samples, scale=1.0, shift=0.0, lo=-np.inf, hi=np.inf):
    """samples [n, N, ...] -> (mean, std) float32 [n, ...]: fp64 sums in sample order j = 0..N-1 (a sequential loop, not np.sum, whose
    pairwise order differs), the unbiased variance (N - 1), each output rounded once."""
    y = premap(samples, scale, shift, lo, hi).astype(np.float64)
    N = y.shape[1]
    s = np.zeros(y[:, 0].shape, np.float64)
    for j in range(N):
        s = s + y[:, j]
    m = s / N
    v = np.zeros_like(m)
    for j in range(N):
        d = y[:, j] - m
        v = v + d * d
    return m.astype(np.float32), np.sqrt(v / (N - 1)).astype(np.float32)
