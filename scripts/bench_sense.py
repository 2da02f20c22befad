"""Cost of --known_sense at BASELINE config 3 (one batch of 32 x 1 x 256 x 256, four reverse steps, 8 coils, an equispaced x4 mask,
lambda 8, 12 iterations, R = 1): the device time (HIP events) of mud_sense_constrain at 1, 2 and `iters` iterations, from which one
conjugate-gradient iteration (one application of N = A^H A in three launches plus the vector update: an upper bound on the application)
follows as the slope, against the clean mud_kspace_constrain on the same batch, alternated in one process; the measurement and the
adjoint; and the whole keyed sampling of the batch with and without the constraint (GraphSampler.sample_keyed), alternated, best of
three.  Prints one JSON line (profiles/sense_bench.json).

    python scripts/bench_sense.py [--batch 32] [--coils 8] [--iters 12] [--reps 20]"""
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
from mudiff_hip import constraints as Cn  # noqa: E402
from mudiff_hip import kspace as KS  # noqa: E402
from mudiff_hip import ops  # noqa: E402
from mudiff_hip import sampling as S  # noqa: E402
from mudiff_hip import sense as SN  # noqa: E402


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
    ap.add_argument('--coils', type=int, default=8)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--lam', type=float, default=8.0)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    cfg = bench_config()
    H, B, T, Nc = cfg.image_size, a.batch, cfg.num_timesteps, a.coils
    g1, g2, _ = build_models(cfg, dev, 0, 1)
    conds = synthetic_batch(cfg, B, dev, seed=100)
    sampler = S.GraphSampler(S.Posterior_Coefficients(cfg, dev), g1, g2, cfg, B, H, H, dev)
    keys = torch.stack([torch.arange(B) + 40, torch.zeros(B, dtype=torch.int64)], 1)
    kd = keys.to(dev)
    k = torch.tanh(torch.randn(B, H, H, device=dev))
    M = KS.build_mask(H, 'equispaced', 4, 0.08, 0, seed=1024)
    mask = torch.from_numpy(M).to(dev)[None].contiguous()
    maps = torch.from_numpy(SN.coil_maps(H, Nc)).to(dev)[None].contiguous()
    y = ops.sense_measure(k, maps, mask)
    ahy = ops.sense_adjoint(y, maps)
    x, x_new = torch.empty(B, 1, H, H, device=dev), torch.randn(B, 1, H, H, device=dev)
    work = torch.empty(ops.sense_ws_floats(B, Nc, H), device=dev)
    cg = torch.empty(B, device=dev)
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    t = torch.ones(B, dtype=torch.int64, device=dev)
    # the single-coil clean constraint on the same batch
    ms_eff = torch.from_numpy(KS.symmetrise(M)).to(dev)[None].contiguous()
    y1 = torch.where(ms_eff != 0, ops.fft2(k), torch.zeros((), device=dev, dtype=torch.complex64)).contiguous()
    work1 = torch.empty(B, H, H, device=dev, dtype=torch.complex64)

    def sense(iters, clean=False):
        return lambda: ops.sense_constrain_into(x, x_new, ahy, mask, maps, a.lam, iters, cg, work, kd, 1024, 1, ops.KIND_SENSE, t, 0, a_cum, s_cum,
                                                clean=clean)

    kspace_clean = lambda: ops.kspace_constrain_into(x, x_new, y1, ms_eff, work1, kd, 1024, 1, ops.KIND_KSPACE, t, 0, a_cum, s_cum, clean=True)      # noqa: E731
    yc = y.clone()
    bound = lambda: Cn.SenseRows(ahy, mask, maps, a.lam, a.iters)                                                                                  # noqa: E731
    names = ('sense_1', 'sense_2', 'sense_iters', 'sense_iters_clean', 'kspace_clean', 'measure', 'adjoint', 'sample', 'sample_sense')
    res = {n: [] for n in names}
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        res['sense_1'].append(event_ms(sense(1), a.reps))
        res['kspace_clean'].append(event_ms(kspace_clean, a.reps))
        res['sense_2'].append(event_ms(sense(2), a.reps))
        res['sense_iters'].append(event_ms(sense(a.iters), a.reps))
        res['sense_iters_clean'].append(event_ms(sense(a.iters, True), a.reps))
        res['measure'].append(event_ms(lambda: ops.sense_measure(k, maps, mask, out=yc), a.reps))
        res['adjoint'].append(event_ms(lambda: ops.sense_adjoint(yc, maps, out=ahy), a.reps))
        res['sample'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3))
        res['sample_sense'].append(event_ms(lambda: sampler.sample_keyed(*conds, keys, 1024, T, constraint=bound()), 3))
    best = {n: min(v) for n, v in res.items()}
    iteration = (best['sense_iters'] - best['sense_1']) / max(a.iters - 1, 1)
    out = sampler.sample_keyed(*conds, keys, 1024, T, constraint=bound())
    d = ops.sense_measure(out[:, 0].contiguous(), maps, mask) - y
    residual = float((torch.linalg.vector_norm(d.flatten(1), dim=1) / torch.linalg.vector_norm(y.flatten(1), dim=1)).max())
    print(json.dumps(dict(
        batch=B, image_size=H, steps=T, coils=Nc, pattern='equispaced', accel=4, sampling_fraction=round(float(M.mean()), 4), resample=1,
        **{'lambda': a.lam}, iters=a.iters,
        sense_1_iteration_us=round(1e3 * best['sense_1'], 2), sense_2_iterations_us=round(1e3 * best['sense_2'], 2),
        sense_step_us=round(1e3 * best['sense_iters'], 2), sense_step_clean_us=round(1e3 * best['sense_iters_clean'], 2),
        iteration_us=round(1e3 * iteration, 2), kspace_clean_us=round(1e3 * best['kspace_clean'], 2),
        iteration_over_coils_x_kspace_clean=round(iteration / (Nc * best['kspace_clean']), 4),
        application_target_met=bool(iteration <= 1.25 * Nc * best['kspace_clean']),
        measure_us=round(1e3 * best['measure'], 2), adjoint_us=round(1e3 * best['adjoint'], 2),
        batch_sampling_ms=round(best['sample'], 3), batch_sampling_sense_ms=round(best['sample_sense'], 3),
        slices_per_s=round(1000.0 * B / best['sample'], 2), slices_per_s_sense=round(1000.0 * B / best['sample_sense'], 2),
        ratio=round(best['sample'] / best['sample_sense'], 5),
        sense_ms_per_reverse_step=round((best['sample_sense'] - best['sample']) / T, 3),
        all_ms={n: [round(v, 4) for v in vs] for n, vs in res.items()},
        max_residual=residual, max_cg_residual=float(sampler.sense_cg_res.max()), finite=bool(torch.isfinite(out).all()))))


if __name__ == '__main__':
    main()
