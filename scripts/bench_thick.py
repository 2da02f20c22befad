"""Cost of --known_thick at BASELINE config 3 (one batch of 32 x 1 x 256 x 256, four reverse steps, slabs of L = 5 thin slices under a
Gaussian profile: 6 measured slabs and 2 free rows, R = 1): the device time (HIP events) of mud_slab_constrain (at a noise level, drawing
in the kernel, and clean) against its algorithmic bytes, mud_slab_average, and the whole keyed sampling of the batch with and without
the constraint (GraphSampler.sample_keyed), alternated in one process.  Prints one JSON line (profiles/thick_bench.json).

    python scripts/bench_thick.py [--batch 32] [--slab 5] [--reps 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench import bench_config, build_models, synthetic_batch  # noqa: E402
from mudiff_hip import ops  # noqa: E402
from mudiff_hip import sampling as S  # noqa: E402
from mudiff_hip import thick as TK  # noqa: E402


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
    ap.add_argument('--slab', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    H, B, T, L = cfg.image_size, a.batch, cfg.num_timesteps, a.slab
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, B, dev, seed=100)
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, dev), g1, g2, cfg, B, H, H, dev)
    keys = torch.stack([torch.arange(B) + 40, torch.zeros(B, dtype=torch.int64)], 1)
    kd = keys.to(dev)
    k = torch.tanh(torch.randn(B, H, H, device=dev))
    groups = B // L
    members = np.arange(groups * L, dtype=np.int32).reshape(groups, L)
    w = TK.profile_weights(L, 'gauss').astype(np.float32)
    tables = ops.slab_tables(members, w)
    y = ops.slab_average(k, members, w)
    x, x_new = torch.empty(B, 1, H, H, device=dev), torch.randn(B, 1, H, H, device=dev)
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    t = torch.ones(B, dtype=torch.int64, device=dev)
    free = B - groups * L
    # per pixel of a row: a member is read and written (4 + 4; its second read hits the cache), a free row is copied (4 + 4); y: 4 a group
    bytes_per_call = (8 * B + 4 * groups) * H * H

    def constrain_all():                                                     # what one batch adds: one call after each of the T steps
        for j, i in enumerate(reversed(range(T))):
            t.fill_(i)
            ops.slab_constrain_into(x, x_new, y, tables, kd, 1024, j, ops.KIND_THICK, t, 0, a_cum, s_cum, clean=i == 0)

    noisy = lambda: ops.slab_constrain_into(x, x_new, y, tables, kd, 1024, 1, ops.KIND_THICK, t, 0, a_cum, s_cum)      # noqa: E731
    clean = lambda: ops.slab_constrain_into(x, x_new, y, tables, kd, 1024, 1, ops.KIND_THICK, t, 0, a_cum, s_cum, clean=True)      # noqa: E731
    thick = (y, members, w, None)
    res = dict(constrain_batch=[], constrain_noisy=[], constrain_clean=[], average=[], sample=[], sample_thick=[])
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        res['constrain_batch'].append(event_ms(constrain_all, a.reps))
        res['constrain_noisy'].append(event_ms(noisy, a.reps))
        res['constrain_clean'].append(event_ms(clean, a.reps))
        res['average'].append(event_ms(lambda: ops.slab_average(k, members, w, out=y), a.reps))
        res['sample'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3))
        res['sample_thick'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T, thick=thick), 3))
    best = {k_: min(v) for k_, v in res.items()}
    spread = {k_: round((max(v) - min(v)) / min(v), 5) for k_, v in res.items() if k_.startswith('sample')}
    out = sampler.sample_keyed(*conds, keys, 1024, T, thick=thick)
    d = ops.slab_average(out[:, 0].contiguous(), members, w) - y
    residual = float((torch.linalg.vector_norm(d.flatten(1), dim=1) / torch.linalg.vector_norm(y.flatten(1), dim=1)).max())
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, L=L, profile='gauss', groups=groups, free_rows=free, resample=1, bytes_per_call=int(bytes_per_call),
        constrain_noisy_us=round(1e3 * best['constrain_noisy'], 2), constrain_clean_us=round(1e3 * best['constrain_clean'], 2),
        constrain_noisy_gb_per_s=round(bytes_per_call / best['constrain_noisy'] / 1e6, 1),
        constrain_clean_gb_per_s=round(bytes_per_call / best['constrain_clean'] / 1e6, 1),
        average_us=round(1e3 * best['average'], 2), constrain_ms_per_batch=round(best['constrain_batch'], 4),
        batch_sampling_ms=round(best['sample'], 3), batch_sampling_thick_ms=round(best['sample_thick'], 3),
        slices_per_s=round(1000.0 * B / best['sample'], 2), slices_per_s_thick=round(1000.0 * B / best['sample_thick'], 2),
        ratio=round(best['sample'] / best['sample_thick'], 5), condition_met=bool(best['sample'] / best['sample_thick'] >= 0.99),
        legs_spread=spread, constrain_share_of_sampling=round(best['constrain_batch'] / best['sample'], 6),
        all_ms={k_: [round(v, 4) for v in vs] for k_, vs in res.items()},
        max_residual=residual, finite=bool(torch.isfinite(out).all()))))


if __name__ == '__main__':
    main()
