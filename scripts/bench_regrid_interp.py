"""Time volume_regrid.regrid(mode='cubic') against mode='linear' on one synthetic int16 volume: both modes in
one process, alternated, each call ended by a device synchronise; the median and the spread of the repeats.  The three passes of the
prefilter are separate kernels (k_bs_x, then k_bs_line twice: y, z): their times come from a kernel trace of this script.

    python scripts/bench_regrid_interp.py [--shape 240 240 155] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'mu-diff_amd')]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--shape', nargs=3, type=int, default=[240, 240, 155])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    from mudiff_hip import volume_regrid as VR
    assert torch.cuda.is_available(), 'this measurement needs the GPU'
    dev = torch.device('cuda:0')
    shape = tuple(args.shape)
    rng = np.random.default_rng(0)
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
    head = (g[0] ** 2 + g[1] ** 2 + g[2] ** 2 < 0.8)                               # a head in air, as the pipeline sees it
    vol = np.asfortranarray((head * (400 + 300 * rng.random(shape))).astype(np.int16))
    raw = torch.from_numpy(np.ascontiguousarray(vol.reshape(-1, order='F'))).to(dev)
    a = np.deg2rad(3.0)
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    M[:3, 3] = (np.array(shape) - 1) / 2.0 - M[:3, :3] @ ((np.array(shape) - 1) / 2.0) + 0.37

    def run(mode):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = VR.regrid(raw, 4, shape, 1.0, 0.0, M, shape, mode)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    times = {'cubic': [], 'linear': []}
    for i in range(args.warmup + args.reps):
        for mode in times:                                                         # alternated: both see the same machine
            t, out = run(mode)
            if i >= args.warmup:
                times[mode].append(t)
    res = {'shape': list(shape), 'reps': args.reps}
    for mode, ts in times.items():
        ts = np.array(ts) * 1e3
        res[mode + '_ms'] = dict(median=float(np.median(ts)), min=float(ts.min()), max=float(ts.max()))
    res['nonzero_fraction'] = float((out != 0).float().mean())
    print(json.dumps(res))


if __name__ == '__main__':
    main()
