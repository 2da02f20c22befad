"""Measurements of DESIGN.md section 5.15 (--denoise): the three kernels of csrc/volume_denoise.hip at 240 x 240 x 155 int16 for the
windows (search, patch) = (2, 1) and (3, 1) - HIP events, 5 warm-up launches, median of 30 -, the wall time of one whole denoise() at
the defaults, and the numpy restatement of the same on this host at a size it can finish (60 x 60 x 39, stated in the output).

    python scripts/bench_denoise.py [--out profiles/denoise_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)

SHAPE = (240, 240, 155)
HOST_SHAPE = (60, 60, 39)
WINDOWS = ((2, 1), (3, 1))


def timed(fn, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def head(shape, seed=1):
    """The ellipsoid head of scripts/bench_bias.py: three tissue classes plus noise times a smooth shading, zero outside."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2.0) / (0.40 * n) for n in shape], indexing='ij')
    inside = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 1.0
    tissue = np.select([rng.random(shape) < 0.33, rng.random(shape) < 0.5], [400.0, 700.0], 1000.0) + rng.standard_normal(shape) * 6.0
    return np.asfortranarray((tissue * np.exp(0.3 * g[0] - 0.2 * g[1] * g[2]) * inside).astype('<i2'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--no_host', action='store_true', help='skip the numpy restatement')
    args = ap.parse_args()
    from mudiff_hip import ops, volume_denoise as VD, volume_intake as VI
    import volume_denoise_ref as D
    dev = 'cuda:0'
    vol = head(SHAPE)
    raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), 4, '<', 1.0, 0.0, SHAPE, np.eye(4), None)
    d = VI.upload(raw, dev)
    meta = (4, SHAPE, 1.0, 0.0)
    out = dict(shape=SHAPE, dtype='int16', launches=args.launches, kernel={})
    keys = ops.volume_denoise_residual(d, *meta)
    sigma, samples = VD.estimate_sigma(raw, dev)
    out['sigma'], out['samples'] = sigma, samples
    out['kernel']['residual'] = timed(lambda: ops.volume_denoise_residual(d, *meta), args.launches)
    out['kernel']['select_hist'] = timed(lambda: ops.volume_denoise_select_hist(keys, 0, 0), args.launches)
    print(f"sigma {sigma:.3f} from {samples} samples; residual {out['kernel']['residual']['median_ms']:.4f} ms, select_hist "
          f"{out['kernel']['select_hist']['median_ms']:.4f} ms", flush=True)
    n = float(np.prod(SHAPE))
    for s, r in WINDOWS:
        t = out['kernel'][f'nlm_s{s}_r{r}'] = timed(lambda: ops.volume_denoise_nlm(d, *meta, s, r, sigma, 1.0), args.launches)
        pairs = n * ((2 * s + 1) ** 3 - 1) * (2 * r + 1) ** 3
        t['squared_differences_per_s'] = pairs / (t['median_ms'] * 1e-3)
        print(f"nlm ({s}, {r}): {t['median_ms']:.3f} ms, {t['squared_differences_per_s'] / 1e12:.2f} T patch terms / s", flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, rep = VD.denoise(raw, dev)
    torch.cuda.synchronize()
    out['denoise'] = dict(wall_s=time.perf_counter() - t0, report=rep)
    print(f"denoise() at the defaults: {out['denoise']['wall_s']:.3f} s, sigma {rep['sigma']:.3f}", flush=True)
    if not args.no_host:
        small = head(HOST_SHAPE).astype(np.float32)
        t0 = time.perf_counter()
        s_host, _ = D.sigma_by_sorting(small)
        D.nlm(small, s_host)
        out['host_numpy'] = dict(shape=HOST_SHAPE, wall_s=time.perf_counter() - t0)
        print(f"numpy restatement at {HOST_SHAPE}: {out['host_numpy']['wall_s']:.2f} s", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
