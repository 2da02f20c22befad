"""Cost of --known_kspace at BASELINE config 3 (one batch of 32 x 1 x 256 x 256, four reverse steps, an equispaced x4 mask, R = 1): the
device time (HIP events) of the three launches of mud_kspace_constrain (at a noise level, drawing in the kernel, and clean) against their
algorithmic bytes, the two launches of ops.fft2, and the whole keyed sampling of the batch with and without the constraint
(GraphSampler.sample_keyed), alternated in one process.  Prints one JSON line (profiles/kspace_bench.json).

    python scripts/bench_kspace.py [--batch 32] [--reps 20]"""
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
from mudiff_hip import kspace as KS  # noqa: E402
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
    k = torch.tanh(torch.randn(B, H, H, device=dev))
    M = KS.symmetrise(KS.build_mask(H, 'equispaced', 4, 0.08, 0, seed=1024))
    mask = torch.from_numpy(M).to(dev)[None].contiguous()
    y = torch.where(mask != 0, ops.fft2(k), torch.zeros((), device=dev, dtype=torch.complex64)).contiguous()
    x, x_new = torch.empty(B, 1, H, H, device=dev), torch.randn(B, 1, H, H, device=dev)
    work = torch.empty(B, H, H, device=dev, dtype=torch.complex64)
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    t = torch.ones(B, dtype=torch.int64, device=dev)
    fraction = float(M.mean())
    # per pixel: (a) x_new 4 + work 8; (b) work 8 + 8, mask 1, y 8 where measured; (c) work 8 + x_new 4 + out 4
    bytes_per_pixel = 12 + 17 + 8 * fraction + 16

    def constrain_all():                                                     # what one batch adds: three launches after each of the T steps
        for j, i in enumerate(reversed(range(T))):
            t.fill_(i)
            ops.kspace_constrain_into(x, x_new, y, mask, work, kd, 1024, j, ops.KIND_KSPACE, t, 0, a_cum, s_cum, clean=i == 0)

    noisy = lambda: ops.kspace_constrain_into(x, x_new, y, mask, work, kd, 1024, 1, ops.KIND_KSPACE, t, 0, a_cum, s_cum)      # noqa: E731
    clean = lambda: ops.kspace_constrain_into(x, x_new, y, mask, work, kd, 1024, 1, ops.KIND_KSPACE, t, 0, a_cum, s_cum, clean=True)      # noqa: E731
    kc = work.clone()
    res = dict(constrain_batch=[], constrain_noisy=[], constrain_clean=[], fft2=[], sample=[], sample_kspace=[])
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        res['constrain_batch'].append(event_ms(constrain_all, a.reps))
        res['constrain_noisy'].append(event_ms(noisy, a.reps))
        res['constrain_clean'].append(event_ms(clean, a.reps))
        res['fft2'].append(event_ms(lambda: ops.fft2(kc, out=kc), a.reps))
        res['sample'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3))
        res['sample_kspace'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T, kspace=(y, mask)), 3))
    best = {k_: min(v) for k_, v in res.items()}
    out = sampler.sample_keyed(*conds, keys, 1024, T, kspace=(y, mask))
    d = torch.where(mask != 0, ops.fft2(out[:, 0].contiguous()) - y, torch.zeros((), device=dev, dtype=torch.complex64))
    residual = float((torch.linalg.vector_norm(d.flatten(1), dim=1) / torch.linalg.vector_norm(y.flatten(1), dim=1)).max())
    pixels = B * H * H
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, pattern='equispaced', accel=4, effective_fraction=round(fraction, 4), resample=1,
        bytes_per_pixel=round(bytes_per_pixel, 2), bytes_per_launch_triple=int(bytes_per_pixel * pixels),
        constrain_noisy_us=round(1e3 * best['constrain_noisy'], 2), constrain_clean_us=round(1e3 * best['constrain_clean'], 2),
        constrain_noisy_gb_per_s=round(bytes_per_pixel * pixels / best['constrain_noisy'] / 1e6, 1),
        constrain_clean_gb_per_s=round(bytes_per_pixel * pixels / best['constrain_clean'] / 1e6, 1),
        fft2_us=round(1e3 * best['fft2'], 2), fft2_gb_per_s=round(32.0 * pixels / best['fft2'] / 1e6, 1),
        constrain_ms_per_batch=round(best['constrain_batch'], 4),
        batch_sampling_ms=round(best['sample'], 3), batch_sampling_kspace_ms=round(best['sample_kspace'], 3),
        slices_per_s=round(1000.0 * B / best['sample'], 2), slices_per_s_kspace=round(1000.0 * B / best['sample_kspace'], 2),
        ratio=round(best['sample'] / best['sample_kspace'], 5), condition_met=bool(best['sample'] / best['sample_kspace'] >= 0.99),
        constrain_share_of_sampling=round(best['constrain_batch'] / best['sample'], 6),
        all_ms={k_: [round(v, 4) for v in vs] for k_, vs in res.items()},
        max_residual=residual, finite=bool(torch.isfinite(out).all()))))


if __name__ == '__main__':
    main()
