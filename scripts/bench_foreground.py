"""Measurements of DESIGN.md section 5.16 (--foreground): every kernel of csrc/volume_foreground.hip at 240 x 240 x 155 int16 on the
ellipsoid head of scripts/bench_denoise.py with noisy air around it - HIP events, 5 warm-up launches, median of 30 -, the labelling also
on the serpentine (the longest chains), the wall time of one whole foreground() at the defaults, and scipy.ndimage.label of the same
mask on this host for scale.

    python scripts/bench_foreground.py [--out profiles/foreground_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--no_host', action='store_true', help='skip scipy.ndimage.label')
    args = ap.parse_args()
    from bench_denoise import head, timed
    from mudiff_hip import ops, volume_foreground as VF, volume_intake as VI
    import volume_foreground_ref as F
    dev = 'cuda:0'
    rng = np.random.default_rng(2)
    vol = head(SHAPE).astype(np.float64)
    air = np.hypot(rng.normal(0.0, 20.0, SHAPE), rng.normal(0.0, 20.0, SHAPE))      # Rician air where the head's file holds zeros
    vol = np.asfortranarray(np.rint(np.where(vol == 0, air, vol)).astype('<i2'))
    raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), 4, '<', 1.0, 0.0, SHAPE, np.eye(4), None)
    d = VI.upload(raw, dev)
    meta = (4, SHAPE, 1.0, 0.0)
    n = int(np.prod(SHAPE))
    out = dict(shape=SHAPE, dtype='int16', launches=args.launches, kernel={})
    found = ops.volume_fg_range(d, *meta).cpu().numpy().view(np.uint32)
    lo, hi = VF.unkey(~int(found[0])), VF.unkey(found[1])
    scale = 256 / (hi - lo)
    k = VF.otsu_bin(ops.volume_fg_hist(d, *meta, lo, scale, 256).cpu().numpy().view(np.uint32))
    mask = ops.volume_fg_mask(d, *meta, lo, scale, 256, k)
    labels = ops.volume_fg_label(mask, SHAPE, 1)
    census, summary = ops.volume_fg_census(labels, SHAPE)
    winner, components = (int(v) for v in summary.cpu().numpy().view(np.uint64))
    root = 0xFFFFFFFF - (winner & 0xFFFFFFFF)
    kept = ops.volume_fg_select(labels, None, root, False)[0]
    holes = ops.volume_fg_label(kept, SHAPE, 0)
    hole_census = ops.volume_fg_census(holes, SHAPE)[0]
    out.update(lo=lo, hi=hi, bin=k, components=components, largest=winner >> 32)
    runs = dict(range=lambda: ops.volume_fg_range(d, *meta), hist=lambda: ops.volume_fg_hist(d, *meta, lo, scale, 256),
                mask=lambda: ops.volume_fg_mask(d, *meta, lo, scale, 256, k), erode=lambda: ops.volume_fg_morph(mask, SHAPE, False),
                dilate=lambda: ops.volume_fg_morph(mask, SHAPE, True), label_mask=lambda: ops.volume_fg_label(mask, SHAPE, 1),
                label_complement=lambda: ops.volume_fg_label(kept, SHAPE, 0), census=lambda: ops.volume_fg_census(labels, SHAPE),
                select_root=lambda: ops.volume_fg_select(labels, None, root, False),
                select_holes=lambda: ops.volume_fg_select(holes, hole_census, 0, True, kept), apply=lambda: ops.volume_fg_apply(d, *meta, kept))
    snake = torch.from_numpy(np.ascontiguousarray(F.serpentine(SHAPE).transpose(2, 1, 0))).to(dev)
    runs['label_serpentine'] = lambda: ops.volume_fg_label(snake, SHAPE, 1)
    checker = torch.from_numpy(np.ascontiguousarray((np.indices(SHAPE).sum(0) % 2 == 0).astype(np.uint8).transpose(2, 1, 0))).to(dev)
    checker_labels = ops.volume_fg_label(checker, SHAPE, 1)
    runs['census_checkerboard'] = lambda: ops.volume_fg_census(checker_labels, SHAPE)
    for name, fn in runs.items():
        t = out['kernel'][name] = timed(fn, args.launches)
        t['voxels_per_s'] = n / (t['median_ms'] * 1e-3)
        print(f"{name}: {t['median_ms']:.4f} ms ({t['voxels_per_s'] / 1e9:.2f} G voxels / s)", flush=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, rep = VF.foreground(raw, dev)
    torch.cuda.synchronize()
    out['foreground'] = dict(wall_s=time.perf_counter() - t0, report=rep)
    print(f"foreground() at the defaults: {out['foreground']['wall_s']:.4f} s, {rep}", flush=True)
    if not args.no_host:
        from scipy import ndimage
        host = mask.cpu().numpy()
        t0 = time.perf_counter()
        count = ndimage.label(host)[1]
        out['host_scipy_label'] = dict(wall_s=time.perf_counter() - t0, components=int(count))
        print(f"scipy.ndimage.label of the raw mask: {out['host_scipy_label']['wall_s']:.3f} s, {count} components", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
