"""Cost of the ensemble's quantile pass: the device time (HIP events) of ops.ensemble_quantiles with K = 3
fractions next to ops.ensemble_stats on the same [32, N, 256, 256] sample buffer, for N = 8 and N = 64, and what the pass adds to the
sampling of a --num_samples 8 chunk: those 32 slices x 8 samples are 8 batches of 32 through GraphSampler.sample_keyed at BASELINE
config 3, so the share is quantiles_ms(N = 8) / (8 x one batch's sampling).  Legs alternated in one process, best of three.  Prints one JSON
line (profiles/ensemble_quantiles_bench.json).

    python scripts/bench_ensemble_quantiles.py [--slices 32] [--reps 20]"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench import bench_config, build_models, synthetic_batch  # noqa: E402
from mudiff_hip import ensemble, ops  # noqa: E402
from mudiff_hip import sampling as S  # noqa: E402

QS = (0.05, 0.5, 0.95)


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--slices', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    H, B, T = cfg.image_size, 32, cfg.num_timesteps
    pre = ensemble.premap(True)
    g = torch.Generator(device=dev).manual_seed(5)
    bufs = {N: torch.randn(a.slices, N, H, H, device=dev, generator=g).mul_(0.6) for N in (8, 64)}      # a share of the samples clamps
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, B, dev, seed=100)
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, dev), g1, g2, cfg, B, H, H, dev)
    keys = torch.stack([torch.arange(B) // 8 + 40, torch.arange(B) % 8], 1)

    res = {f'{k}_{N}': [] for N in bufs for k in ('stats', 'quantiles')}
    res['sample'] = []
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        for N, x in bufs.items():
            res[f'stats_{N}'].append(event_ms(lambda: ops.ensemble_stats(x, *pre), a.reps))
            res[f'quantiles_{N}'].append(event_ms(lambda: ops.ensemble_quantiles(x, QS, *pre), a.reps))
        res['sample'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3))
    best = {k: min(v) for k, v in res.items()}
    out = {}
    for N, x in bufs.items():
        nbytes = 4.0 * x.numel()
        q = ops.ensemble_quantiles(x, QS, *pre)
        out[f'N{N}'] = dict(stats_ms=round(best[f'stats_{N}'], 4), quantiles_ms=round(best[f'quantiles_{N}'], 4),
                            quantiles_over_stats=round(best[f'quantiles_{N}'] / best[f'stats_{N}'], 3),
                            stats_read_GBps=round(nbytes / best[f'stats_{N}'] / 1e6, 1),
                            quantiles_read_GBps=round(nbytes / best[f'quantiles_{N}'] / 1e6, 1),
                            ordered=bool((q[0] <= q[1]).all() and (q[1] <= q[2]).all()), finite=bool(torch.isfinite(q).all()))
    batches = a.slices * 8 // B
    print(json.dumps(dict(
        slices=a.slices, image_size=H, steps=T, quantiles=list(QS), **out, batch_sampling_ms=round(best['sample'], 3),
        chunk_batches=batches, chunk_sampling_ms=round(batches * best['sample'], 3),
        quantiles_share_of_chunk_sampling=round(best['quantiles_8'] / (batches * best['sample']), 6),
        stats_share_of_chunk_sampling=round(best['stats_8'] / (batches * best['sample']), 6),
        all_ms={k: [round(t, 4) for t in v] for k, v in res.items()})))


if __name__ == '__main__':
    main()
