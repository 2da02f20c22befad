"""Measurements of DESIGN.md section 5.14 (--bias_correct): the kernels of csrc/volume_bias.hip at 240 x 240 x 155 int16 for shrink
4 / 2 / 1 with the field at level 0 (one level) and at level 3 (four levels) - HIP events, 5 warm-up launches, median of 30 -, the wall
time of one whole correct() at the defaults, and the numpy restatement of one iteration (corrected, histogram, fit) on this host.

    python scripts/bench_bias.py [--out profiles/bias_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)

SHAPE = (240, 240, 155)


def timed(fn, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--no_host', action='store_true', help='skip the numpy restatement of one iteration')
    args = ap.parse_args()
    from mudiff_hip import ops, volume_bias as VB, volume_intake as VI
    import volume_bias_ref as B
    dev = 'cuda:0'
    rng = np.random.default_rng(1)
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2.0) / (0.40 * n) for n in SHAPE], indexing='ij')
    head = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 1.0
    tissue = np.select([rng.random(SHAPE) < 0.33, rng.random(SHAPE) < 0.5], [400.0, 700.0], 1000.0) + rng.standard_normal(SHAPE) * 6.0
    vol = np.asfortranarray((tissue * np.exp(0.3 * g[0] - 0.2 * g[1] * g[2]) * head).astype('<i2'))
    raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), 4, '<', 1.0, 0.0, SHAPE, np.eye(4), None)
    d = VI.upload(raw, dev)
    meta = (4, SHAPE, 1.0, 0.0)
    out = dict(shape=SHAPE, dtype='int16', launches=args.launches, kernel={})
    lat_rng = np.random.default_rng(2)
    for shrink in (4, 2, 1):
        eng = VB.DeviceEngine(d, meta, shrink)
        row = out['kernel'][str(shrink)] = dict(samples=eng.n_samples, log=timed(lambda: ops.volume_bias_log(d, *meta, shrink), args.launches))
        for levels in (1, 4):
            lat = VB.flat_lattices([lat_rng.standard_normal(((1 << l) + 3,) * 3) * 0.05 for l in range(levels)], dev)
            lo, hi, _ = eng.corrected([L for L in VB.new_lattices(levels)])
            scale = 200.0 / (hi - lo)
            table = torch.from_numpy(VB.sharpen(eng.hist(lo, scale, 200), lo, hi)).to(dev)
            k = VB.choose_k(eng.n_samples, lo, hi)
            level = levels - 1
            r = row[f'level{level}'] = dict(
                corrected=timed(lambda: ops.volume_bias_corrected(eng.u, eng.c[0], eng.c[1], lat, levels, SHAPE, shrink), args.launches),
                hist=timed(lambda: ops.volume_bias_hist(eng.c[0], lo, scale, 200), args.launches),
                fit=timed(lambda: ops.volume_bias_fit(eng.c[0], table, lo, scale, level, SHAPE, shrink, k), args.launches))
            if shrink == 4:
                r['apply'] = timed(lambda: ops.volume_bias_apply(d, *meta, lat, levels), args.launches)
            print(f'shrink {shrink} level {level}: ' + ', '.join(f"{name} {v['median_ms']:.4f} ms" for name, v in r.items()), flush=True)
        print(f"shrink {shrink}: log {row['log']['median_ms']:.4f} ms, {eng.n_samples} samples", flush=True)
    t0 = time.perf_counter()
    corrected, rep = VB.correct(raw, dev)
    torch.cuda.synchronize()
    out['correct'] = dict(wall_s=time.perf_counter() - t0, iterations=rep['iterations'], dmax=rep['dmax'], field_min=rep['field_min'],
                          field_max=rep['field_max'])
    print(f"correct() at the defaults: {out['correct']['wall_s']:.3f} s, iterations {rep['iterations']}", flush=True)
    if not args.no_host:
        values = vol.astype(np.float32)
        ref = B.Engine(B.log_image(values, 4), SHAPE, 4)
        lattices = VB.new_lattices(4)
        t0 = time.perf_counter()
        lo, hi, _ = ref.corrected(lattices)
        scale = 200.0 / (hi - lo)
        table = VB.sharpen(ref.hist(lo, scale, 200), lo, hi)
        ref.fit(3, table, lo, scale, VB.choose_k(ref.n_samples, lo, hi))
        out['host_numpy_iteration_shrink4_level3_s'] = time.perf_counter() - t0
        print(f"numpy restatement, one iteration at shrink 4, level 3: {out['host_numpy_iteration_shrink4_level3_s']:.2f} s", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
