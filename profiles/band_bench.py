"""Cost of --known_thick_volume at BASELINE config 3 (256 x 256, four reverse steps, batch 32) on a 155-slice volume (DESIGN.md section
5.29; prints one JSON line: profiles/band_bench.json).

(a) The price of lockstep: the 155 slices through GraphSampler.sample_lockstep with constraint=None (the first-step graph replayed for
    every batch of every step) against the same slices through GraphSampler.sample_keyed batch by batch (first-step graph once per
    batch, then the later-step graph), alternated in one process; slices/s of each and their ratio.
(b) mud_band_constrain per call (HIP events) at n = 155, S = 256, sets = 1 and 8, for 5 mm slices on a 1 mm grid from a fractional
    origin: contiguous (m = 30, bandwidth 1) and every 2.5 mm (m = 60, bandwidth 2); drawing in the kernel, and clean; and the four calls
    of one prediction as a share of its sampling time under lockstep.

    python profiles/band_bench.py [--batch 32] [--slices 155] [--reps 20]"""
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
from mudiff_hip import thick_volume as TV  # noqa: E402


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
    ap.add_argument('--slices', type=int, default=155)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    H, B, T, n = cfg.image_size, a.batch, cfg.num_timesteps, a.slices
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, n, dev, seed=100)
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, dev), g1, g2, cfg, B, H, H, dev)
    keys = torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.int64)], 1)

    def keyed():                                                             # batch by batch, the last one padded
        out = []
        for lo in range(0, n, B):
            m = min(B, n - lo)
            idx = torch.tensor(list(range(lo, lo + m)) + [lo + m - 1] * (B - m))
            out.append(sampler.sample_keyed(*(c[idx.to(dev)] for c in conds), keys[idx], 1024, T)[:m])
        return torch.cat(out)

    lock = lambda: sampler.sample_lockstep(conds, keys, 1024, T)             # noqa: E731
    res = dict(keyed=[], lockstep=[])
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        res['keyed'].append(event_ms(keyed, 2))
        res['lockstep'].append(event_ms(lock, 2))
    best = {k: min(v) for k, v in res.items()}
    diff = float((keyed() - lock()).abs().max())
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    kernel = {}
    for name, step, m in (('contiguous', 5.0, 30), ('overlap', 2.5, 60)):
        A = TV.weight_rows(n, 2.3 + step * np.arange(m), 5.0, 'box')
        tab = ops.band_tables(A)
        y = ops.band_measure(torch.tanh(torch.randn(1, n, H * H, device=dev)), tab)[0]
        for sets in (1, 8):
            x_new, x = torch.randn(sets * n, 1, H, H, device=dev), torch.empty(sets * n, 1, H, H, device=dev)
            work = torch.empty(sets * tab.m, H * H, device=dev)
            kd = torch.stack([torch.arange(n).repeat(sets), torch.arange(sets).repeat_interleave(n)], 1).to(dev)
            t = torch.ones(sets * n, dtype=torch.int64, device=dev)
            call = lambda clean: ops.band_constrain_into(x, x_new, y, tab, work, kd, 1024, 1, ops.KIND_BAND, t, 0, a_cum, s_cum, clean=clean)      # noqa: E731
            noisy, clean = event_ms(lambda: call(False), a.reps), event_ms(lambda: call(True), a.reps)
            # per pixel: x read per member and once more in the scatter, out written, y read, v written, read, u written and read per member
            nbytes = 4 * H * H * (sets * (2 * tab.nnz + 2 * n + 3 * tab.m) + tab.m)
            per_prediction = (T - 1) * noisy + clean
            kernel[f'{name}_sets{sets}'] = dict(m=tab.m, bandwidth=tab.bw, cond=round(tab.cond, 3), sets=sets, noisy_us=round(1e3 * noisy, 1),
                                                clean_us=round(1e3 * clean, 1), bytes_per_call=int(nbytes),
                                                clean_gb_per_s=round(nbytes / clean / 1e6, 1), ms_per_prediction=round(per_prediction, 3),
                                                share_of_lockstep_sampling=round(per_prediction / (sets * best['lockstep']), 6))
            del x_new, x, work
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, slices=n, volume_keyed_ms=round(best['keyed'], 2), volume_lockstep_ms=round(best['lockstep'], 2),
        slices_per_s_keyed=round(1000.0 * n / best['keyed'], 2), slices_per_s_lockstep=round(1000.0 * n / best['lockstep'], 2),
        lockstep_over_keyed=round(best['keyed'] / best['lockstep'], 5),
        legs_spread={k: round((max(v) - min(v)) / min(v), 5) for k, v in res.items()},
        all_ms={k: [round(v, 3) for v in vs] for k, vs in res.items()}, max_abs_difference=diff, band_constrain=kernel)))


if __name__ == '__main__':
    main()
