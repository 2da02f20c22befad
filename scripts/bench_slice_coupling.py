"""Cost of --slice_coupling at BASELINE config 3 (one batch of 32 x 1 x 256 x 256, four reverse steps): the device time (HIP events) of
the image-sized Gaussian draws of one batch - x_init and the four steps' posterior noise - drawn coupled (sigma = 4, R = 12: 25 Philox
blocks per output block) and uncoupled, next to the whole keyed sampling of that batch (GraphSampler.sample_keyed: its draws and the four
captured reverse steps), alternated in one process.  Prints one JSON line (profiles/slice_coupling_bench.json).

    python scripts/bench_slice_coupling.py [--sigma 4] [--batch 32] [--reps 20]"""
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
from mudiff_hip import ops, slice_coupling  # noqa: E402
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
    ap.add_argument('--sigma', type=float, default=4.0)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    H, B, T = cfg.image_size, a.batch, cfg.num_timesteps
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, B, dev, seed=100)
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, dev), g1, g2, cfg, B, H, H, dev)
    coupling = slice_coupling.coupling_taps(a.sigma)
    taps, radius = ops.coupling_taps_arg(*coupling)
    keys = torch.stack([torch.arange(B) + 40, torch.zeros(B, dtype=torch.int64)], 1)
    kd = keys.to(dev)
    x = torch.empty(B, 1, H, H, device=dev)
    image_draws = [(0, ops.KIND_X_INIT)] + [(k, ops.KIND_NOISE) for k in range(T)]

    def plain():
        for step, kind in image_draws:
            ops.randn_keyed_into(x, kd, 1024, step, kind)

    def coupled():
        for step, kind in image_draws:
            ops.randn_keyed_coupled_into(x, kd, 1024, step, kind, taps, radius)

    res = dict(plain=[], coupled=[], sample=[], sample_coupled=[])
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        res['plain'].append(event_ms(plain, a.reps))
        res['coupled'].append(event_ms(coupled, a.reps))
        res['sample'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3))
        res['sample_coupled'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T, coupling=coupling), 3))
    best = {k: min(v) for k, v in res.items()}
    out = sampler.sample_keyed(*conds, keys, 1024, T, coupling=coupling)
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, sigma=a.sigma, radius=radius, image_draws=len(image_draws),
        plain_draws_ms=round(best['plain'], 4), coupled_draws_ms=round(best['coupled'], 4),
        coupled_over_plain=round(best['coupled'] / best['plain'], 3),
        batch_sampling_ms=round(best['sample'], 3), batch_sampling_coupled_ms=round(best['sample_coupled'], 3),
        coupled_draws_share_of_sampling=round(best['coupled'] / best['sample'], 5),
        plain_draws_share_of_sampling=round(best['plain'] / best['sample'], 5),
        all_ms={k: [round(t, 4) for t in v] for k, v in res.items()}, finite=bool(torch.isfinite(out).all()))))


if __name__ == '__main__':
    main()
