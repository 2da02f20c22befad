"""Measurements of DESIGN.md section 5.18 (--brain_extract): mud_volume_edt (its three passes in one call) for both uses of
brain_mask() - the distance to the complement of the tissue mask and the distance to the core - mud_volume_edt_select, and one whole
brain_mask() at the defaults, on a 240 x 240 x 155 int16 head (a brain ellipsoid, a dark gap and a bright scalp shell around it, zero
air) at 1 x 1 x 1 mm and at 0.94 x 0.94 x 3 mm - HIP events, 5 warm-up launches, median of 30.

    python scripts/bench_brain.py [--out profiles/volume_brain.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd'), os.path.join(REPO, 'tests'), os.path.join(REPO, 'scripts')):
    sys.path.insert(0, p)

SHAPE = (240, 240, 155)
SPACINGS = ((1.0, 1.0, 1.0), (0.94, 0.94, 3.0))


def head_with_scalp(shape, seed=1):
    """Normalised radius r of the ellipsoid with semi-axes 0.40 of each side: brain r <= 0.84 (three tissue classes plus noise), a dark gap
    up to 0.92, a bright scalp shell up to 1, zero air."""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2.0) / (0.40 * n) for n in shape], indexing='ij')
    r = np.sqrt(g[0] ** 2 + g[1] ** 2 + g[2] ** 2)
    tissue = np.select([rng.random(shape) < 0.33, rng.random(shape) < 0.5], [500.0, 700.0], 900.0) + rng.standard_normal(shape) * 6.0
    vol = np.select([r <= 0.84, r <= 0.92, r <= 1.0], [tissue, 30.0 + rng.random(shape) * 10.0, 1000.0 + rng.standard_normal(shape) * 6.0], 0.0)
    return np.asfortranarray(np.rint(vol).astype('<i2'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=30)
    args = ap.parse_args()
    from bench_denoise import timed
    from mudiff_hip import ops, volume_brain as VBR, volume_foreground as VF, volume_intake as VI
    dev = 'cuda:0'
    vol = head_with_scalp(SHAPE)
    n = int(np.prod(SHAPE))
    out = dict(shape=SHAPE, dtype='int16', launches=args.launches, spacing={})
    for spacing in SPACINGS:
        raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), 4, '<', 1.0, 0.0, SHAPE, np.diag(list(spacing) + [1.0]), None)
        d, meta = VI.upload(raw, dev), (4, SHAPE, 1.0, 0.0)
        tissue = VF.threshold_mask(d, meta, 256, dict())
        away = ops.volume_edt(tissue, SHAPE, 0, spacing)
        eroded = ops.volume_edt_select(away, 25.0, True)[0]
        core = VF.largest_component(eroded, SHAPE)[0]
        runs = dict(edt_to_complement=lambda: ops.volume_edt(tissue, SHAPE, 0, spacing), edt_to_core=lambda: ops.volume_edt(core, SHAPE, 1, spacing),
                    edt_select=lambda: ops.volume_edt_select(away, 25.0, True), brain_mask=lambda: VBR.brain_mask(raw, dev))
        here = out['spacing']['x'.join(str(s) for s in spacing)] = dict(kernel={})
        for name, fn in runs.items():
            t = here['kernel'][name] = timed(fn, args.launches)
            t['voxels_per_s'] = n / (t['median_ms'] * 1e-3)
            print(f"{spacing} {name}: {t['median_ms']:.4f} ms ({t['voxels_per_s'] / 1e9:.2f} G voxels / s)", flush=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, rep = VBR.brain_mask(raw, dev)
        torch.cuda.synchronize()
        here['brain_mask'] = dict(wall_s=time.perf_counter() - t0, report=rep)
        print(f"{spacing} brain_mask() at the defaults: {here['brain_mask']['wall_s']:.4f} s, {rep}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
