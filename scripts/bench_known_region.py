"""Cost of --known_volume at BASELINE config 3 (one batch of 32 x 1 x 256 x 256, four reverse steps, a half-known mask, R = 1): the
device time (HIP events) of the four constraint launches of one batch (mud_known_constrain: three at a noise level, drawing in the kernel,
and the clean one) next to the whole keyed sampling of that batch with and without the constraint (GraphSampler.sample_keyed),
alternated in one process.  Prints one JSON line (profiles/known_region_bench.json).

    python scripts/bench_known_region.py [--batch 32] [--reps 20]"""
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
from mudiff_hip import ops  # noqa: E402
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
    keys = torch.stack([torch.arange(B) + 40, torch.zeros(B, dtype=torch.int64)], 1)
    kd = keys.to(dev)
    known = torch.tanh(torch.randn(B, 1, H, H, device=dev))
    mask = torch.zeros(B, 1, H, H, dtype=torch.uint8, device=dev)
    mask[:, :, :, : H // 2] = 1                                             # half of every slice is known
    x, x_new = torch.empty(B, 1, H, H, device=dev), torch.randn(B, 1, H, H, device=dev)
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    t = torch.zeros(B, dtype=torch.int64, device=dev)

    def constrain():                                                         # what one batch adds: a launch after each of the T steps
        for k, i in enumerate(reversed(range(T))):
            t.fill_(i)
            ops.known_constrain_into(x, x_new, known, mask, kd, 1024, k, ops.KIND_KNOWN, t, 0, a_cum, s_cum, clean=i == 0)

    def copies():                                                            # what it replaces: the copy of x_new into x
        for _ in range(T):
            x.copy_(x_new)

    res = dict(constrain=[], copies=[], sample=[], sample_known=[])
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        res['constrain'].append(event_ms(constrain, a.reps))
        res['copies'].append(event_ms(copies, a.reps))
        res['sample'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3))
        res['sample_known'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T, known=known, known_mask=mask), 3))
    best = {k: min(v) for k, v in res.items()}
    out = sampler.sample_keyed(*conds, keys, 1024, T, known=known, known_mask=mask)
    m = mask.bool()
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, known_fraction=0.5, resample=1,
        constrain_ms_per_batch=round(best['constrain'], 4), copies_ms_per_batch=round(best['copies'], 4),
        batch_sampling_ms=round(best['sample'], 3), batch_sampling_known_ms=round(best['sample_known'], 3),
        slices_per_s=round(1000.0 * B / best['sample'], 2), slices_per_s_known=round(1000.0 * B / best['sample_known'], 2),
        constrain_share_of_sampling=round(best['constrain'] / best['sample'], 6),
        all_ms={k: [round(v, 4) for v in vs] for k, vs in res.items()},
        known_exact=bool(torch.equal(out[m], known[m])), finite=bool(torch.isfinite(out).all()))))


if __name__ == '__main__':
    main()
