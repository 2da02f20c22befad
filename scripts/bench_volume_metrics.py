"""Time whole-volume scoring (mudiff_hip.volume_metrics) on a synthetic BraTS-geometry pair (240 x 240, 155
planes, full slab, four regions, with a std volume) against the fp64 scipy restatement on the host (tests/volume_metrics_ref.py).

    python scripts/bench_volume_metrics.py [--reps 20] [--no-host]

Prints one JSON line: ops.volume_metrics device time (HIP events, median / min over --reps), score_volume wall time (slice2d and the
host read-back included) and the host restatement's time (one run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mu-diff_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    from mudiff_hip import ops
    from mudiff_hip import volume_metrics as VM
    shape = (155, 240, 240)
    rng = np.random.default_rng(0)
    g = rng.random(shape, dtype=np.float32)
    p = np.clip(g + 0.05 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    brain, tumor = rng.random(shape) < 0.6, rng.random(shape) < 0.1
    region = (1 | brain.astype(np.uint8) << 1 | tumor.astype(np.uint8) << 2 | (brain & ~tumor).astype(np.uint8) << 3).astype(np.uint8)
    std = (0.02 * rng.random(shape)).astype(np.float32)
    dev = 'cuda:0'
    pd, gd, rd, sd = (torch.from_numpy(x).to(dev) for x in (p, g, region, std))
    for _ in range(3):                                               # warm-up: code objects, allocator
        ops.volume_metrics(pd, gd, rd, sd, nreg=4)
        VM.score_volume(pd, gd, rd, sd)
    torch.cuda.synchronize()
    ks = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.volume_metrics(pd, gd, rd, sd, nreg=4)
        e1.record()
        torch.cuda.synchronize()
        ks.append(e0.elapsed_time(e1))
    walls = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = VM.score_volume(pd, gd, rd, sd)
        walls.append((time.perf_counter() - t0) * 1e3)
    out = dict(shape=list(shape), regions=4, std=True, kernel_ms_median=float(np.median(ks)), kernel_ms_min=float(min(ks)),
               score_volume_ms_median=float(np.median(walls)), score_volume_ms_min=float(min(walls)), reps=a.reps,
               ssim3d_slab=rep['metrics']['slab']['ssim3d'])
    if not a.no_host:
        import volume_metrics_ref as R
        t0 = time.perf_counter()                                     # region totals only (no per-plane curves): the SSIM map and masked means
        S = R.ssim_map(p, g)
        inner = R.interior(shape)
        d = p.astype(np.float64) - g
        tot = {}
        for k, name in enumerate(VM.REGIONS):
            sel = (region >> k) & 1 == 1
            tot[name] = (float(np.mean(S[sel & inner])), float(np.mean(d[sel] ** 2)), float(np.mean(np.abs(d[sel]))),
                         R.pearson(std[sel], np.abs(d[sel])))
        out['host_restatement_s'] = time.perf_counter() - t0
        out['ssim3d_slab_abs_diff'] = abs(tot['slab'][0] - rep['metrics']['slab']['ssim3d'])
        out['pearson_slab_abs_diff'] = abs(tot['slab'][3] - rep['uncertainty']['slab']['pearson_r'])
    print(json.dumps(out))


if __name__ == '__main__':
    main()
