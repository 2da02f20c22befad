"""Time mud_volume_regrid (--regrid) on a BraTS-sized volume: 240 x 240 x 155 int16 voxels resampled onto a
grid of the same shape through the oblique matrix of the tests (tests/volume_regrid_ref.py), trilinear and nearest.

    python scripts/bench_regrid.py [--reps 30] [--no-host]
    rocprofv3 --pmc <counters> -d OUT -- python scripts/bench_regrid.py --reps 3 --no-host

Prints one JSON line: the kernel's device time (HIP events, median / min over --reps after a warm-up), the algorithmic-bytes rate
(source bytes + 4 bytes per output voxel) / time and its share of 8 TB/s, the time of scipy's affine_transform(order=1) on this host for
the same volume (one run), and the largest difference between the two results relative to max|src|."""
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
HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    import volume_regrid_ref as G
    from mudiff_hip import NIFTI_I2
    from mudiff_hip import volume_regrid as VR
    shape = (240, 240, 155)
    rng = np.random.default_rng(0)
    vol = np.asfortranarray((rng.integers(1, 3000, shape) * (rng.random(shape) > 0.3)).astype(np.int16))
    _, sa, _, ra = G.case('oblique', shape, shape)
    M = VR.grid_matrix(sa, ra)
    src = torch.from_numpy(np.ascontiguousarray(vol.reshape(-1, order='F'))).to('cuda:0')
    nbytes = src.numel() * 2 + 4 * int(np.prod(shape))
    out = dict(shape=list(shape), datatype='int16', matrix='oblique', reps=a.reps, algorithmic_bytes=nbytes)
    for mode in ('linear', 'nearest'):
        for _ in range(5):                                           # warm-up: code object, allocator
            res = VR.regrid(src, NIFTI_I2, shape, 1.0, 0.0, M, shape, mode)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = VR.regrid(src, NIFTI_I2, shape, 1.0, 0.0, M, shape, mode)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = float(np.median(ms))
        out[mode] = dict(ms_median=med, ms_min=float(min(ms)), ms_max=float(max(ms)), bytes_per_s=nbytes / (med * 1e-3),
                         share_of_8TBps=nbytes / (med * 1e-3) / HBM_BYTES_PER_S, nonzero=float((res != 0).float().mean()))
        if mode == 'linear':
            linear = res.cpu().numpy().transpose(2, 1, 0)
    if not a.no_host:
        from scipy import ndimage
        f32 = vol.astype(np.float32)
        t0 = time.perf_counter()
        want = ndimage.affine_transform(f32, M[:3, :3], offset=M[:3, 3], output_shape=shape, order=1, mode='grid-constant', cval=0.0)
        out['scipy_affine_transform_s'] = time.perf_counter() - t0
        out['max_abs_diff_over_max_src'] = float(np.abs(linear.astype(np.float64) - want).max() / np.abs(f32).max())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
