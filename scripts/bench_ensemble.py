"""N-sample ensembles at BASELINE config 3 (256x256, nf=64, batches of 32): samples/s of mudiff_hip.ensemble.sample_ensemble (N = 8 per
slice, keyed draws) next to slices/s of the plain captured sampler (GraphSampler.sample, one normal_ draw per slice) on the same
slices, alternated in one process; plus the device time (HIP events) of one step's keyed draws and of the statistics of a
161-slice x 8-sample volume.  Prints one JSON line.

    python scripts/bench_ensemble.py [--slices 64] [--samples 8] [--batch 32] [--iters 3]
    rocprofv3 --kernel-trace --stats -d <dir> -o ens -- python scripts/bench_ensemble.py --iters 1     # k_randn_keyed, k_ensemble_stats*"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench import bench_config, build_models, synthetic_batch  # noqa: E402
from mudiff_hip import ensemble, ops  # noqa: E402
from mudiff_hip.driver import pad_batch  # noqa: E402
from mudiff_hip import sampling as S  # noqa: E402


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
    ap.add_argument('--slices', type=int, default=64)
    ap.add_argument('--samples', type=int, default=8)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=3)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    H, B, n, N = cfg.image_size, a.batch, a.slices, a.samples
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, n, dev, seed=100)
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, dev), g1, g2, cfg, B, H, H, dev)
    gen = torch.Generator(device=dev).manual_seed(0)

    def plain():
        outs = []
        for b0 in range(0, n, B):
            cs = [pad_batch(c[b0:b0 + B], min(B, n - b0), B) for c in conds]
            x0 = torch.randn(B, 1, H, H, device=dev, generator=gen)
            outs.append(sampler.sample(*cs, x0, cfg.num_timesteps, generator=gen))
        return outs

    def ens():
        return ensemble.sample_ensemble(cfg, g1, g2, conds, N, 1024, sampler=sampler)

    plain()
    ens()                                                                   # warm-up of both paths
    torch.cuda.synchronize()
    t_plain, t_ens = [], []
    for _ in range(a.iters):                                                # alternated: both see the same box state
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plain()
        torch.cuda.synchronize()
        t_plain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        mean, std = ens()
        torch.cuda.synchronize()
        t_ens.append(time.perf_counter() - t0)
    plain_rate = n / min(t_plain)
    ens_rate = n * N / min(t_ens)

    keys = torch.stack([torch.arange(B) // N, torch.arange(B) % N], 1).to(dev)
    z, noise = torch.empty(B, cfg.nz, device=dev), torch.empty(B, 1, H, H, device=dev)
    draws_ms = event_ms(lambda: (ops.randn_keyed_into(z, keys, 1024, 1, ops.KIND_Z), ops.randn_keyed_into(noise, keys, 1024, 1, ops.KIND_NOISE)), 20)
    vol = torch.rand(161, N, H, H, device=dev) * 2 - 1
    stats_ms = event_ms(lambda: ops.ensemble_stats(vol, 0.5, 0.5, 0.0, 1.0), 20)
    stats_bytes = 4.0 * 161 * H * H * (N + 2)
    print(json.dumps(dict(
        slices=n, samples_per_slice=N, batch=B, plain_slices_per_s=round(plain_rate, 3), ensemble_samples_per_s=round(ens_rate, 3),
        ensemble_over_plain=round(ens_rate / plain_rate, 4), plain_s=[round(t, 4) for t in t_plain], ensemble_s=[round(t, 4) for t in t_ens],
        keyed_draws_per_step_ms=round(draws_ms, 4), stats_161x8_ms=round(stats_ms, 4), stats_161x8_tb_per_s=round(stats_bytes / stats_ms / 1e9, 3),
        mean_std=float(std.double().mean()), finite=bool(torch.isfinite(mean).all() and torch.isfinite(std).all()))))


if __name__ == '__main__':
    main()
