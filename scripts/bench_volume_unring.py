"""Time --unring (mudiff_hip.volume_unring) on one synthetic BraTS-geometry volume: 240 x 240 x 155, int16, the
default options (axes 0 1, 20 shifts per side, window 1 3).

    python scripts/bench_volume_unring.py [--reps 20] [--warmup 3]

Prints one JSON line: HIP-event time (median / min over --reps after --warmup runs) of the directional filter, of each of the two line
passes and of the whole stage as volume_unring.unring runs it (tables, uploads and the report's read-back included), the FMA rate of the
shift bank that the line passes imply (lines x n x n x 2 N fused multiply-adds each), and the share of one subject's sampling time
(155 slices at the README's 105 slices/s).  A measurement, not a gate: nothing exists to compare it against."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'mu-diff_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SLICES_PER_S = 105.0


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    from mudiff_hip import ops, volume_intake as VI, volume_unring as VU
    from volume_support import raw_volume
    shape, dev = (240, 240, 155), 'cuda:0'
    rng = np.random.default_rng(0)
    x, y, z = np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing='ij')
    head = ((x / 0.8) ** 2 + (y / 0.9) ** 2 + (z / 0.95) ** 2 <= 1.0) * 600.0 + ((x / 0.3) ** 2 + (y / 0.2) ** 2 + (z / 0.4) ** 2 <= 1.0) * 300.0
    vol = np.asfortranarray(np.rint(head + 20.0 * rng.standard_normal(shape)).astype('<i2'))
    raw = raw_volume(vol)
    kw = VU.DEFAULTS
    N, (nx, ny) = kw['shifts'], (shape[kw['axes'][0]], shape[kw['axes'][1]])
    stored, meta = VI.upload(raw, dev), raw.kernel_meta('bench')
    tables = [torch.from_numpy(t).to(dev) for t in VU.filter_tables(nx, ny)]
    tx, ty = (torch.from_numpy(VU.shift_table(n, N)).to(dev) for n in (nx, ny))
    ix, iy, _ = ops.volume_unring_filter(stored, *meta, kw['axes'], *tables)
    out = torch.empty_like(ix)
    filt = timed(lambda: ops.volume_unring_filter(stored, *meta, kw['axes'], *tables), a.reps, a.warmup)
    line_x = timed(lambda: ops.volume_unring_lines(ix, shape, kw['axes'][0], 2, N, kw['window'], tx, out=out), a.reps, a.warmup)
    line_y = timed(lambda: ops.volume_unring_lines(iy, shape, kw['axes'][1], 2, N, kw['window'], ty, out=out, accumulate=True), a.reps, a.warmup)
    whole = timed(lambda: VU.unring(raw, dev, **kw), a.reps, a.warmup)
    voxels = float(np.prod(shape))
    fma = [voxels * n * 2 * N for n in (nx, ny)]
    sampling_ms = 1e3 * shape[2] / SLICES_PER_S
    _, rep = VU.unring(raw, dev, **kw)
    print(json.dumps(dict(shape=list(shape), datatype='int16', options=dict(axes=list(kw['axes']), shifts=N, window=list(kw['window'])), reps=a.reps,
                          filter_ms_median=filt[0], filter_ms_min=filt[1], lines_x_ms_median=line_x[0], lines_x_ms_min=line_x[1],
                          lines_y_ms_median=line_y[0], lines_y_ms_min=line_y[1], stage_ms_median=whole[0], stage_ms_min=whole[1],
                          shift_bank_tfma_per_s=[fma[0] / line_x[0] * 1e-9, fma[1] / line_y[0] * 1e-9],
                          shift_bank_tflops=[2 * fma[0] / line_x[0] * 1e-9, 2 * fma[1] / line_y[0] * 1e-9],
                          sampling_ms=sampling_ms, share_of_sampling=whole[0] / sampling_ms, moved=rep['moved'], mean_abs_shift=rep['mean_abs_shift'])))


if __name__ == '__main__':
    main()
