"""Measurements of DESIGN.md section 5.13 (--coregister): mud_volume_joint_hist at 240 x 240 x 155 int16 onto the same shape through the
oblique matrix at strides 4 / 2 / 1 (HIP events, warm-up, median of 30 launches), its algorithmic-bytes rate as a share of 8 TB/s, the
numpy restatement of one histogram on this host, and the wall time of one whole coregister() search.

    python scripts/bench_coreg.py [--out profiles/coreg_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)

SHAPE, PEAK = (240, 240, 155), 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--no_host', action='store_true', help='skip the numpy restatement (about a minute at stride 1)')
    args = ap.parse_args()
    import mudiff_hip
    from mudiff_hip import volume_coreg as VC, volume_intake as VI
    import volume_coreg_ref as K
    import volume_regrid_ref as G
    dev = 'cuda:0'
    rng = np.random.default_rng(1)
    g = np.meshgrid(*[(np.arange(n) - (n - 1) / 2.0) / (0.40 * n) for n in SHAPE], indexing='ij')
    head = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2) <= 1.0                      # background: ~73 % of the voxels in one bin
    fix = np.asfortranarray(((200 + 800 * rng.random(SHAPE)) * head).astype('<i2'))
    mov = np.asfortranarray(((900 - 600 * rng.random(SHAPE)) * head).astype('<i2'))
    _, sa, _, ra = G.case('oblique', SHAPE, SHAPE)
    lin = sa[:3, :3] / np.array([1.1, 0.9, 1.3])                            # the oblique case's rotation at 1 mm voxels
    sa = sa.copy()
    sa[:3, :3], sa[:3, 3] = lin, -lin @ ((np.array(SHAPE) - 1) / 2.0)
    M = G.matrix(sa, ra)
    raws = [VI.RawVolume(np.ascontiguousarray(v.reshape(-1, order='F')), 4, '<', 1.0, 0.0, SHAPE, a, None) for v, a in ((fix, ra), (mov, sa))]
    ranges = VC.bin_ranges(*raws, 32)
    devs = [VI.upload(r, dev) for r in raws]
    lib = mudiff_hip.load()
    hist = torch.empty(32 * 32, dtype=torch.int32, device=dev)
    mm = (C.c_double * 12)(*np.ascontiguousarray(M[:3]).reshape(-1).tolist())
    out = dict(shape=SHAPE, dtype='int16', bins=32, launches=args.launches, kernel={})
    for stride in (4, 2, 1):
        def launch():
            rc = lib.mud_volume_joint_hist(devs[0].data_ptr(), 4, *SHAPE, 1.0, 0.0, devs[1].data_ptr(), 4, *SHAPE, 1.0, 0.0, mm, stride, *ranges, 32,
                                           hist.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, lib.mud_last_error()
        for _ in range(5):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        counted = int(hist.cpu().numpy().view(np.uint32).astype(np.int64).sum())
        points = int(np.prod([-(-n // stride) for n in SHAPE]))
        nbytes = 2 * points + 2 * min(8 * counted, mov.size)               # one fixed voxel per point; each moving voxel at most once
        med = float(np.median(ms))
        out['kernel'][str(stride)] = dict(median_ms=med, min_ms=float(min(ms)), max_ms=float(max(ms)), points=points, counted=counted,
                                          algorithmic_bytes=nbytes, share_of_8TBs=nbytes / (med * 1e-3) / PEAK)
        print(f'stride {stride}: median {med:.4f} ms (min {min(ms):.4f}, max {max(ms):.4f}), {counted} of {points} counted, '
              f'{100 * nbytes / (med * 1e-3) / PEAK:.2f} % of 8 TB/s', flush=True)
    if not args.no_host:
        t0 = time.perf_counter()
        want = K.joint_hist(fix.astype(np.float32), mov.astype(np.float32), M, 2, ranges, 32)
        out['host_numpy_stride2_s'] = time.perf_counter() - t0
        got = VC.joint_hist(devs[0], (4, SHAPE, 1.0, 0.0), devs[1], (4, SHAPE, 1.0, 0.0), M, 2, ranges, 32)
        out['host_vs_device_stride2_sum_abs_diff'] = int(np.abs(got - want).sum())
        print(f"numpy restatement, stride 2: {out['host_numpy_stride2_s']:.2f} s; sum|dev - ref| {out['host_vs_device_stride2_sum_abs_diff']}", flush=True)
    t0 = time.perf_counter()
    W, rep = VC.coregister(raws[0], raws[1], dev)
    torch.cuda.synchronize()
    out['search'] = dict(wall_s=time.perf_counter() - t0, evaluations=rep['evaluations'], accepted=rep['accepted'], params=rep['params'])
    print(f"coregister: {out['search']['wall_s']:.2f} s, evaluations {rep['evaluations']}, accepted {rep['accepted']}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
