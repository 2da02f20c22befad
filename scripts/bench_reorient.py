"""Measurements of DESIGN.md section 5.20 (--reorient): mud_volume_reorient at 240 x 240 x 155, int16 and fp32 (HIP events, 5 warm-ups,
median of 30 samples; a sample is an event pair around 20 back-to-back launches into one preallocated destination, divided by 20, so
that a 10-microsecond kernel is not timed together with the host's gap between two launches): one row-copy permutation with an x flip
and every transposing permutation with every flip, of which the two slowest are reported; against a device-to-device hipMemcpyAsync of the same bytes in the same process (the ceiling a permutation can
reach) and one contiguous numpy copy of the restatement's transpose / flip view on this host (what the kernel replaces).

    python scripts/bench_reorient.py [--out profiles/reorient_bench.json]
"""
import argparse
import itertools
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
ROWS = ((0, 1, 2), (True, False, False))                 # the row-copy case: the fast axis stays, read backwards
REPS = 20


def timed(fn, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=30)
    args = ap.parse_args()
    import mudiff_hip
    from mudiff_hip import ops, volume_reorient as VO
    lib = mudiff_hip.load()
    import volume_reorient_ref as R
    dev = 'cuda:0'
    out = dict(shape=SHAPE, samples=args.launches, launches_per_sample=REPS, dtypes={})
    for name, width, tdt in (('int16', 2, torch.int16), ('fp32', 4, torch.float32)):
        vol = R.labelled(SHAPE, width)
        flat = torch.from_numpy(np.ascontiguousarray(vol.reshape(-1, order='F')).view(np.int16 if width == 2 else np.float32)).to(dev)
        assert flat.dtype == tdt
        nbytes = flat.numel() * width
        res = dict(bytes_moved=2 * nbytes)
        spare = torch.empty_like(flat)
        res['memcpy_d2d'] = timed(lambda: spare.copy_(flat, non_blocking=True), args.launches)      # hipMemcpyAsync, device to device
        cases = {}
        for perm in itertools.permutations(range(3)):
            for flip in itertools.product((False, True), repeat=3):
                if perm[0] == 0 and (perm, flip) != ROWS:
                    continue
                p = VO.ReorientPlan(perm, flip, SHAPE, np.eye(4), '', '')
                got = ops.volume_reorient(flat, width, SHAPE, p)
                if flip == (True, False, True) or (perm, flip) == ROWS:                             # a few against the restatement
                    want = R.apply(vol, perm, flip)
                    assert np.array_equal(got.cpu().numpy().view(vol.dtype).reshape(p.shape, order='F'), want), (perm, flip)
                del got
                key = ''.join(str(q) for q in perm) + '/' + ''.join('-' if f else '+' for f in flip)
                mask = sum(1 << o for o, f in enumerate(flip) if f)

                def launch():
                    rc = lib.mud_volume_reorient(flat.data_ptr(), width, *SHAPE, *perm, mask, spare.data_ptr(), mudiff_hip.stream_ptr())
                    assert rc == 0, lib.mud_last_error()
                cases[key] = timed(launch, args.launches)
        rows_key = '012/-++'
        worst = sorted((k for k in cases if k != rows_key), key=lambda k: -cases[k]['median_ms'])[:2]
        best = min((k for k in cases if k != rows_key), key=lambda k: cases[k]['median_ms'])
        res['rows_x_flip'] = dict(case=rows_key, **cases[rows_key])
        res['transposing_worst'] = [dict(case=k, **cases[k]) for k in worst]
        res['transposing_best'] = dict(case=best, **cases[best])
        res['transposing_all_median_ms'] = {k: cases[k]['median_ms'] for k in cases if k != rows_key}
        perm, flip = tuple(int(c) for c in worst[0][:3]), tuple(c == '-' for c in worst[0][4:])
        t0 = time.perf_counter()
        np.asfortranarray(VO.apply_host(vol, VO.ReorientPlan(perm, flip, SHAPE, np.eye(4), '', '')))      # x fastest in memory, as the kernel writes
        res['host_numpy_s'] = time.perf_counter() - t0
        for k in ('rows_x_flip',):
            res[k]['vs_memcpy'] = res[k]['median_ms'] / res['memcpy_d2d']['median_ms']
        for c in res['transposing_worst']:
            c['vs_memcpy'] = c['median_ms'] / res['memcpy_d2d']['median_ms']
        out['dtypes'][name] = res
        gbs = lambda ms: 2 * nbytes / (ms * 1e-3) / 1e9                                            # noqa: E731
        print(f"{name}: memcpy d2d {res['memcpy_d2d']['median_ms']:.4f} ms ({gbs(res['memcpy_d2d']['median_ms']):.0f} GB/s) | rows with x flip "
              f"{res['rows_x_flip']['median_ms']:.4f} ms | transposing worst {worst[0]} {cases[worst[0]]['median_ms']:.4f} ms, {worst[1]} "
              f"{cases[worst[1]]['median_ms']:.4f} ms, best {best} {cases[best]['median_ms']:.4f} ms | numpy {res['host_numpy_s'] * 1e3:.1f} ms", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
