"""Cost of --known_lowres_volume at BASELINE config 3 (256 x 256, four reverse steps, batch 32) on a 155-slice volume (DESIGN.md section
5.31; prints one JSON line: profiles/lowres_bench.json).

(a) GraphSampler.sample_lockstep over the 155 slices, three legs alternated in one process, best of three each: unconstrained, with
    --known_thick_volume's constraint for a 1 x 1 x 5 mm Y (30 thick slices from a fractional origin, bandwidth 1) and with
    --known_lowres_volume's for a 2 x 2 x 5 mm Y (30 x 127 x 127 coarse voxels from a fractional origin, bandwidth 1 on every axis);
    slices/s of each and the constraint's share of the sampling time.
(b) One apply_volume of the new constraint per call (HIP events; the four passes of mud_lowres_constrain together): drawing in the
    kernel, and clean; mud_lowres_measure (passes 1 and 2 without the solves) next to them; the four calls of one prediction as a
    share of its lockstep sampling time.

    python profiles/lowres_bench.py [--batch 32] [--slices 155] [--reps 20]"""
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
from mudiff_hip import lowres_volume as LV  # noqa: E402
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
    k = torch.tanh(torch.randn(1, n, H, H, device=dev))
    m_z = (n - 5) // 5
    A_z = TV.weight_rows(n, 2.3 + 5.0 * np.arange(m_z), 5.0, 'box')                  # 5 mm slices on 1 mm, a fractional origin
    A_p = TV.weight_rows(H, 0.8 + 2.0 * np.arange((H - 2) // 2), 2.0, 'box')         # 2 mm voxels on 1 mm, a fractional origin
    band_tab = ops.band_tables(A_z)
    thick = TV.BandMeasurement(ops.band_measure(k.reshape(1, n, H * H), band_tab)[0].view(m_z, H, H), A_z)
    low_tab = ops.lowres_tables(A_z, A_p, A_p)
    lowres = LV.LowresMeasurement(ops.lowres_measure(k, low_tab)[0], (A_z, A_p, A_p))
    legs = dict(free=None, thick_volume=thick, lowres_volume=lowres)
    run = lambda c: sampler.sample_lockstep(conds, keys, 1024, T, constraint=c)      # noqa: E731
    res = {name: [] for name in legs}
    for _ in range(3):                                                               # alternated: every leg sees the same box state
        for name, c in legs.items():
            res[name].append(event_ms(lambda: run(c), 2))
    best = {name: min(v) for name, v in res.items()}
    residual = {}
    for name in ('thick_volume', 'lowres_volume'):
        legs[name].record_volume(run(legs[name]), sampler.lockstep_x_new)
        residual[name] = legs[name].finish()['max_residual']
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    x_new, x = torch.randn(n, 1, H, H, device=dev), torch.empty(n, 1, H, H, device=dev)
    work = torch.empty(ops.lowres_ws_floats(1, low_tab), device=dev)
    ax = torch.empty((1,) + low_tab.shape, device=dev)
    kd = torch.stack([torch.arange(n), torch.zeros(n, dtype=torch.int64)], 1).to(dev)
    t = torch.ones(n, dtype=torch.int64, device=dev)
    call = lambda clean: ops.lowres_constrain_into(x, x_new, lowres.y, low_tab, work, kd, 1024, 1, ops.KIND_LOWRES, t, 0, a_cum, s_cum, clean=clean)      # noqa: E731
    noisy, clean = event_ms(lambda: call(False), a.reps), event_ms(lambda: call(True), a.reps)
    measure = event_ms(lambda: ops.lowres_measure(x_new.view(1, n, H, H), low_tab, out=ax, work=work), a.reps)
    per_prediction = (T - 1) * noisy + clean
    # x read by pass 1 and by pass 4, out written; P written and read; U written, solved in place three times, read by pass 4
    nbytes = 4 * (3 * n * H * H + 2 * n * low_tab.y.m * low_tab.x.m + 8 * low_tab.z.m * low_tab.y.m * low_tab.x.m)
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, slices=n, coarse=list(low_tab.shape), bandwidth=[low_tab.z.bw, low_tab.y.bw, low_tab.x.bw],
        cond=round(low_tab.cond, 3), volume_ms={name: round(v, 2) for name, v in best.items()},
        slices_per_s={name: round(1000.0 * n / v, 2) for name, v in best.items()},
        share_of_sampling={name: round((best[name] - best['free']) / best[name], 5) for name in ('thick_volume', 'lowres_volume')},
        legs_spread={name: round((max(v) - min(v)) / min(v), 5) for name, v in res.items()},
        all_ms={name: [round(v, 3) for v in vs] for name, vs in res.items()}, max_residual=residual,
        lowres_constrain=dict(noisy_us=round(1e3 * noisy, 1), clean_us=round(1e3 * clean, 1), measure_us=round(1e3 * measure, 1),
                              bytes_per_call=int(nbytes), clean_gb_per_s=round(nbytes / clean / 1e6, 1), ms_per_prediction=round(per_prediction, 3),
                              share_of_lockstep_sampling=round(per_prediction / best['lowres_volume'], 6)))))


if __name__ == '__main__':
    main()
