"""The two slab kernels of the device intake on one BraTS-sized volume, and the host's z-score moments.

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/profile_zscore_intake.py [--rounds 20] [--json profiles/zscore_intake.json]

Uploads one 240 x 240 x 155 int16 volume (the synthetic subject of scripts/bench_cohort.py), then launches mud_volume_slab_normalise and
mud_volume_slab_zscore on the 155-plane slab alternately, --rounds times each: under rocprofv3's kernel trace the stats table then holds
both kernels' times from one run (they move the same bytes).  Without the profiler the script still reports event-timed medians.  The
host part times volume_intake.zscore_moments on the same volume (median of five calls)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'mu-diff_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

from mudiff_hip import volume_intake as VI  # noqa: E402

SHAPE = (240, 240, 155)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--json', type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'profile_zscore_intake.py measures on a GPU'
    x, y, z = np.meshgrid(*[np.linspace(-1, 1, s, dtype=np.float32) for s in SHAPE], indexing='ij')
    inside = (x / 0.8) ** 2 + (y / 0.85) ** 2 + (z / 0.9) ** 2 < 1
    vol = np.where(inside, np.random.default_rng(100).integers(1, 1500, SHAPE, dtype=np.int16), 0).astype(np.int16)
    raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), VI.NIFTI_I2, '<', 1.0, 0.0, SHAPE, np.eye(4), None)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        mean, std = VI.zscore_moments(raw)
        host.append(time.perf_counter() - t0)
    dev = VI.upload(raw, 'cuda:0')
    rec = VI.CensusRecord.from_bytes(VI.census(dev, raw.code, SHAPE).cpu().numpy().tobytes(), 2)
    lo, den, degenerate = VI.thresholds(rec)
    s0, s1 = 0, SHAPE[2] - 1
    runs = dict(normalise=lambda: VI.slab_normalise(dev, raw.code, SHAPE, 1.0, 0.0, lo, den, degenerate, s0, s1),
                zscore=lambda: VI.slab_zscore(dev, raw.code, SHAPE, 1.0, 0.0, mean, std, s0, s1))
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    nbytes = vol.size * (2 + 4)
    out = dict(what='scripts/profile_zscore_intake.py: slab kernels on one 240 x 240 x 155 int16 volume (all 155 planes), event-timed, and the '
                    'host z-score moments', device=torch.cuda.get_device_name(0), rounds=a.rounds, bytes_moved_per_launch=nbytes,
               event_ms={k: dict(median=statistics.median(v), min=min(v)) for k, v in ms.items()},
               zscore_moments_host_s=dict(median=statistics.median(host), min=min(host), max=max(host)),
               moments=[float(mean), float(std)])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
