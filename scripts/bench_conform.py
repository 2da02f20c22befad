"""Measurements of DESIGN.md section 5.21 (--conform / --antialias): mud_volume_lowpass on a 512 x 512 x 176 int16 volume with the weights
of f = (2.2, 2.2, 1) and of f = (2.2, 2.2, 2.2), alone and followed by the trilinear mud_volume_regrid onto 240 x 240 x 155 (HIP events,
5 warm-ups, median of 30), against device-to-device copies of the same bytes in the same process (the ceiling: a first pass reads 2 and
writes 4 bytes per voxel, a later one reads 4 and writes 4) and the numpy restatement of the low-pass on this host (what it replaces).
The low-pass is timed at the C ABI with everything preallocated, so that the events bracket the kernels and the counter's memset only.  Recorded, not gated: the stage runs once per input per subject.

    python scripts/bench_conform.py [--out profiles/conform_bench.json]
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

SRC, DST = (512, 512, 176), (240, 240, 155)
CASES = {'f=2.2,2.2,1': (2.2, 2.2, 1.0), 'f=2.2,2.2,2.2': (2.2, 2.2, 2.2)}


def timed(fn, samples):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(samples):
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
    ap.add_argument('--samples', type=int, default=30)
    ap.add_argument('--no_host', action='store_true', help='skip the numpy restatement (minutes on a slow host)')
    args = ap.parse_args()
    from mudiff_hip import volume_conform as VCF, volume_regrid as VR
    import volume_conform_ref as CR
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    vol = rng.integers(0, 4000, SRC, dtype=np.int16)
    flat = torch.from_numpy(np.ascontiguousarray(vol.reshape(-1, order='F'))).to(dev)
    n = flat.numel()
    out, scratch = (torch.empty(SRC[2], SRC[1], SRC[0], device=dev, dtype=torch.float32) for _ in range(2))
    res = dict(source=SRC, target=DST, datatype='int16', samples=args.samples, cases={})
    a, b = torch.empty(n * 4, dtype=torch.uint8, device=dev), torch.empty(n * 4, dtype=torch.uint8, device=dev)
    # a copy of k bytes moves 2 k: 3 n bytes = the 6 B per voxel of a first pass, 4 n bytes = the 8 B per voxel of a later pass
    res['copy_of_first_pass_traffic'] = timed(lambda: b[:3 * n].copy_(a[:3 * n]), args.samples)
    res['copy_of_later_pass_traffic'] = timed(lambda: b.copy_(a), args.samples)
    import ctypes as C
    import mudiff_hip
    lib, bad = mudiff_hip.load(), torch.empty(1, device=dev, dtype=torch.int32)

    def lowpass(weights):
        ws = []
        for w in weights:
            ws += [None, 0] if w is None else [w.ctypes.data_as(C.POINTER(C.c_double)), w.size // 2]
        code = lib.mud_volume_lowpass(mudiff_hip.ptr(flat), 4, *SRC, 1.0, 0.0, *ws, mudiff_hip.ptr(out), mudiff_hip.ptr(scratch), mudiff_hip.ptr(bad),
                                      mudiff_hip.stream_ptr())
        assert code == 0, lib.mud_last_error()
    for name, f in CASES.items():
        M = np.diag(list(f) + [1.0])
        plan = VCF.lowpass_plan(M)
        case = dict(factors=list(f), radii=plan['radii'], passes=sum(w is not None for w in plan['weights']))
        case['lowpass'] = timed(lambda: lowpass(plan['weights']), args.samples)

        def both():
            lowpass(plan['weights'])
            return VR.regrid(out.reshape(-1), 16, SRC, 1.0, 0.0, M, DST)
        case['lowpass_and_trilinear'] = timed(both, args.samples)
        case['trilinear_alone'] = timed(lambda: VR.regrid(flat, 4, SRC, 1.0, 0.0, M, DST), args.samples)
        if not args.no_host:
            t0 = time.perf_counter()
            CR.lowpass(vol.astype(np.float32), plan['weights'])
            case['numpy_restatement_s'] = time.perf_counter() - t0
        res['cases'][name] = case
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
