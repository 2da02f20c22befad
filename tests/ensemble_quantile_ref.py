"""numpy restatement of mud_ensemble_quantiles (csrc/ensemble.hip): the definition the kernel is held to bit for
bit.  np.quantile on float32 data uses another lerp and is not the definition; tests compare against it only loosely."""
import numpy as np

from ensemble_ref import premap


def quantiles(samples, qs, scale=1.0, shift=0.0, lo=-np.inf, hi=np.inf):
    """samples [n, N, ...] and K fractions in [0, 1] -> float32 [K, n, ...].  With y the pre-mapped fp32 samples (ensemble_ref.premap)
    sorted ascending along N:  h = (N - 1) q,  i = min(floor(h), N - 2),  g = h - i,  out = fp32(y[i] + g * (y[i+1] - y[i])),  every
    step from h on in fp64 and rounded once.  A pixel with a NaN sample gives NaN for every q."""
    y = premap(samples, scale, shift, lo, hi)
    N = y.shape[1]
    bad = np.isnan(y).any(axis=1)
    ys = np.sort(y, axis=1).astype(np.float64)               # (np.sort puts a NaN last; those pixels are overwritten below)
    out = np.empty((len(qs),) + y.shape[:1] + y.shape[2:], np.float32)
    with np.errstate(invalid='ignore'):
        for k, q in enumerate(qs):
            h = np.float64(N - 1) * np.float64(q)
            i = min(int(np.floor(h)), N - 2)
            g = h - np.float64(i)
            d = ys[:, i + 1] - ys[:, i]
            e = g * d
            out[k] = (ys[:, i] + e).astype(np.float32)
            out[k][bad] = np.nan
    return out
