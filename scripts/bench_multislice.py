"""Cost of --known_multislice at BASELINE config 3 (one batch of 32 x 1 x 256 x 256, four reverse steps, slabs of L = 5 thin slices under
a Gaussian profile: 6 measured slabs and 2 free rows, an equispaced x4 mask, R = 1).

    python scripts/bench_multislice.py [--parent DIR] [--out profiles/multislice_bench.json]

The driver opens no GPU itself.  It starts every GPU step as a child under its own `timeout` and stops at the first one that fails:
 1. `--measure`, one process with the legs alternated over three rounds (best of three, the spread reported): the device time (HIP
    events) of mud_slab_kspace_constrain at a noise level (drawing in the kernel) and clean, against its algorithmic bytes; beside it, on
    the same batch, the two older kernels whose work it fuses - mud_kspace_constrain on 6 rows (the transform work) and
    mud_slab_constrain on the 32 rows (the row traffic); and the whole keyed sampling of the batch with and without the constraint
    (GraphSampler.sample_keyed).
 2. with --parent DIR (a built checkout of the commit before this mode): `bench.py --gpus 1 --steps 10 --warmup 3` there and here,
    alternated, two runs each: the default path.
Writes one JSON object to --out and prints it."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def event_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(a):
    import numpy as np
    import torch
    from bench import bench_config, build_models, synthetic_batch
    from mudiff_hip import constraints as Cn, kspace as KS, ops, sampling as S, thick as TK
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
    M = KS.build_mask(H, 'equispaced', a.accel, KS.DEFAULT_CENTER, KS.DEFAULT_AXIS, 1024)
    mask = torch.from_numpy(KS.symmetrise(M)).to(dev)[None].contiguous()
    avg = ops.slab_average(k, members, w)
    y = torch.where(mask != 0, ops.fft2(avg), torch.zeros((), device=dev, dtype=torch.complex64)).contiguous()
    x, x_new = torch.empty(B, 1, H, H, device=dev), torch.randn(B, 1, H, H, device=dev)
    work = torch.empty(B, H, H, device=dev, dtype=torch.complex64)
    a_cum, s_cum, _, _ = sampler._diffusion_tables()
    t = torch.ones(B, dtype=torch.int64, device=dev)
    n_mem, free = groups * L, B - groups * L
    # per pixel: a member is read by the forward row pass and read and written by the inverse one (12), a free row is copied (8); per
    # pixel of a group: work is written, read and written, read (32), y (8) and the mask (1)
    bytes_per_call = (12 * n_mem + 8 * free + 41 * groups) * H * H
    bytes_kspace = 44 * groups * H * H                                   # ops.kspace_constrain_into's count for `groups` rows
    bytes_slab = (8 * B + 4 * groups) * H * H                            # scripts/bench_thick.py's count

    def fused(clean):
        return lambda: ops.slab_kspace_constrain_into(x, x_new, y, mask, tables, work, kd, 1024, 1, ops.KIND_MULTISLICE, t, 0, a_cum, s_cum, clean=clean)

    def constrain_all():                                                     # what one batch adds: one call after each of the T steps
        for j, i in enumerate(reversed(range(T))):
            t.fill_(i)
            ops.slab_kspace_constrain_into(x, x_new, y, mask, tables, work, kd, 1024, j, ops.KIND_MULTISLICE, t, 0, a_cum, s_cum, clean=i == 0)

    # the parent's kernels on the same batch: the transforms of `groups` rows, and the slab projection of all B rows
    xg, xg_new = x[:groups], x_new[:groups].contiguous()
    kspace = lambda clean: (lambda: ops.kspace_constrain_into(xg, xg_new, y, mask, work[:groups], kd[:groups], 1024, 1, ops.KIND_KSPACE,      # noqa: E731
                                                              t[:groups], 0, a_cum, s_cum, clean=clean))
    slab = lambda clean: (lambda: ops.slab_constrain_into(x, x_new, avg, tables, kd, 1024, 1, ops.KIND_THICK, t, 0, a_cum, s_cum, clean=clean))      # noqa: E731
    con = Cn.SlabKSpaceRows((y, mask, members, w, None))
    legs = dict(constrain_batch=(constrain_all, a.reps), fused_noisy=(fused(False), a.reps), fused_clean=(fused(True), a.reps),
                kspace_noisy=(kspace(False), a.reps), kspace_clean=(kspace(True), a.reps), slab_noisy=(slab(False), a.reps),
                slab_clean=(slab(True), a.reps), sample=(lambda: sampler.sample_keyed(*conds, keys, 1024, T), 3),
                sample_multislice=(lambda: sampler.sample_keyed(*conds, keys, 1024, T, constraint=con), 3))
    res = {name: [] for name in legs}
    for _ in range(3):                                                       # alternated: every leg sees the same box state
        for name, (fn, reps) in legs.items():
            res[name].append(event_ms(fn, reps))
    best = {k_: min(v) for k_, v in res.items()}
    spread = {k_: round((max(v) - min(v)) / min(v), 5) for k_, v in res.items()}
    out = sampler.sample_keyed(*conds, keys, 1024, T, constraint=con)
    d = torch.where(mask != 0, ops.fft2(ops.slab_average(out[:, 0].contiguous(), members, w)) - y, torch.zeros((), device=dev, dtype=torch.complex64))
    residual = float((torch.linalg.vector_norm(d.flatten(1), dim=1) / torch.linalg.vector_norm(y.flatten(1), dim=1)).max())
    us = lambda name: round(1e3 * best[name], 2)                             # noqa: E731
    sums = {c: best[f'kspace_{c}'] + best[f'slab_{c}'] for c in ('noisy', 'clean')}
    slack = {c: max(res[f'fused_{c}']) - min(res[f'fused_{c}']) + max(res[f'kspace_{c}']) - min(res[f'kspace_{c}']) + max(res[f'slab_{c}']) - min(res[f'slab_{c}'])
             for c in ('noisy', 'clean')}
    return dict(
        batch=B, image_size=H, steps=T, L=L, profile='gauss', groups=groups, free_rows=free, pattern='equispaced', accel=a.accel,
        effective_fraction=float(mask.float().mean()), resample=1, bytes_per_call=int(bytes_per_call), bytes_kspace_rows=int(bytes_kspace),
        bytes_slab_batch=int(bytes_slab),
        fused_noisy_us=us('fused_noisy'), fused_clean_us=us('fused_clean'), kspace_noisy_us=us('kspace_noisy'), kspace_clean_us=us('kspace_clean'),
        slab_noisy_us=us('slab_noisy'), slab_clean_us=us('slab_clean'),
        parents_sum_noisy_us=round(1e3 * sums['noisy'], 2), parents_sum_clean_us=round(1e3 * sums['clean'], 2),
        round_to_round_spread_noisy_us=round(1e3 * slack['noisy'], 2), round_to_round_spread_clean_us=round(1e3 * slack['clean'], 2),
        fused_within_parents_sum_noisy=bool(best['fused_noisy'] <= sums['noisy'] + slack['noisy']),
        fused_within_parents_sum_clean=bool(best['fused_clean'] <= sums['clean'] + slack['clean']),
        fused_noisy_gb_per_s=round(bytes_per_call / best['fused_noisy'] / 1e6, 1), fused_clean_gb_per_s=round(bytes_per_call / best['fused_clean'] / 1e6, 1),
        constrain_ms_per_batch=round(best['constrain_batch'], 4), batch_sampling_ms=round(best['sample'], 3),
        batch_sampling_multislice_ms=round(best['sample_multislice'], 3), slices_per_s=round(1000.0 * B / best['sample'], 2),
        slices_per_s_multislice=round(1000.0 * B / best['sample_multislice'], 2), ratio=round(best['sample'] / best['sample_multislice'], 5),
        condition_met=bool(best['sample'] / best['sample_multislice'] >= 0.99), legs_spread=spread,
        constrain_share_of_sampling=round(best['constrain_batch'] / best['sample'], 6),
        all_ms={k_: [round(v, 4) for v in vs] for k_, vs in res.items()}, max_residual=residual, finite=bool(torch.isfinite(out).all()))


def step(argv, cwd, limit):
    """One GPU step: a child under its own `timeout`; -> its last stdout line as JSON.  SystemExit at a failure: nothing more is started."""
    print(f'[bench_multislice] {" ".join(argv[1:])} in {cwd}', file=sys.stderr, flush=True)
    c = subprocess.run(['timeout', '-k', '10', str(limit)] + argv, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if c.returncode != 0:
        sys.stderr.write(c.stdout[-2000:] + c.stderr[-4000:])
        raise SystemExit(f'bench_multislice: {" ".join(argv)} in {cwd} ended with status {c.returncode}; stopping here')
    return json.loads([ln for ln in c.stdout.splitlines() if ln.startswith('{')][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--slab', type=int, default=5)
    ap.add_argument('--accel', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--measure', action='store_true', help='the measuring child itself (prints one JSON line)')
    ap.add_argument('--parent', type=str, default=None, help='a built checkout of the parent commit: bench.py runs there and here, alternated')
    ap.add_argument('--out', type=str, default=os.path.join(REPO, 'profiles', 'multislice_bench.json'))
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a)))
        return
    me = [sys.executable, os.path.abspath(__file__), '--measure', '--batch', str(a.batch), '--slab', str(a.slab), '--accel', str(a.accel), '--reps',
          str(a.reps)]
    out = step(me, REPO, 900)
    out['default_path'] = 'not measured'
    if a.parent is not None:
        bench = [sys.executable, 'bench.py', '--gpus', '1', '--steps', '10', '--warmup', '3']
        runs = dict(parent=[], this=[])
        for _ in range(2):                                                   # alternated: parent, this, parent, this
            runs['parent'].append(step(bench, os.path.abspath(a.parent), 600))
            runs['this'].append(step(bench, REPO, 600))
        out['default_path'] = runs
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
