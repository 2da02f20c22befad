"""Measurements of DESIGN.md section 5.22 (--align) on a 240 x 240 x 155 int16 head: one level-0 launch of mud_volume_mirror_moments
(every candidate plane of the full grid in one launch, at the coarse stride), one refinement launch (27 candidates) at either stride,
and one whole estimate() search (wall clock around work that ends in a device-to-host copy).  The yardstick is what the library could do
before this kernel: the same candidates evaluated as K separate mud_volume_joint_hist launches with the volume as both the fixed and
the moving side (its 32 x 32 histogram holds the six sums).  HIP events, warm-up, `--launches` timed repetitions, median / min / max; the
two level-0 variants alternate in the timed loop.

    python scripts/bench_align.py [--out profiles/align_bench.json]
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

SHAPE = (240, 240, 155)


def timed(fn, launches, warm=3):
    for _ in range(warm):
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
    return ms


def spread(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), repetitions=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--searches', type=int, default=3)
    args = ap.parse_args()
    import mudiff_hip
    from mudiff_hip import volume_align as VA, volume_coreg as VC, volume_intake as VI
    import volume_align_ref as AR
    dev = 'cuda:0'
    A = AR.affine(SHAPE, (1.0, 1.0, 1.0))                 # 1 mm voxels, slightly oblique
    pose = (7.0, -5.0, 3.0)
    vol = AR.phantom(pose, SHAPE, A=A, scale=3.2)         # the analytic head of the tests at the size of a head: ~140 x 175 x 200 mm
    raw = VI.RawVolume(np.ascontiguousarray(vol.reshape(-1, order='F')), 4, '<', 1.0, 0.0, SHAPE, A, None)
    centre = VC.grid_centre(SHAPE, A)
    lo, hi = VC.value_range(raw)
    bins = VA.DEFAULTS['bins']
    scale = bins / (hi - lo)
    vdev = VI.upload(raw, dev)
    lib = mudiff_hip.load()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731
    d = VA.DEFAULTS
    coarse, fine = d['strides']
    g = np.meshgrid(VA._axis(d['max_deg'], d['step_deg']), VA._axis(d['max_deg'], d['step_deg']), VA._axis(d['max_mm'], d['step_mm']), indexing='ij')
    level0 = np.stack([v.reshape(-1) for v in g], 1)
    near = np.array([(i, j, k) for i in (0, -1, 1) for j in (0, -1, 1) for k in (0, -1, 1)], np.float64) * np.array([0.625, 0.625, 0.5]) + np.array(pose)
    out = dict(shape=SHAPE, dtype='int16', bins=bins, launches=args.launches, candidates_level0=len(level0), strides=[coarse, fine])

    def batched(cand, stride):
        mats = torch.from_numpy(np.ascontiguousarray(VA.mirror_matrices(cand, A, centre).reshape(-1, 12))).to(dev)
        sums = torch.empty(len(cand), 6, dtype=torch.int64, device=dev)

        def launch():
            rc = lib.mud_volume_mirror_moments(vdev.data_ptr(), 4, *SHAPE, 1.0, 0.0, mats.data_ptr(), len(cand), stride, lo, scale, bins, sums.data_ptr(), stream())
            assert rc == 0, lib.mud_last_error()
        return launch, sums

    def one_by_one(cand, stride):
        mats = [(C.c_double * 12)(*m.reshape(-1).tolist()) for m in VA.mirror_matrices(cand, A, centre)]
        hist = torch.empty(len(cand), bins * bins, dtype=torch.int32, device=dev)

        def launch():
            for k, m in enumerate(mats):
                rc = lib.mud_volume_joint_hist(vdev.data_ptr(), 4, *SHAPE, 1.0, 0.0, vdev.data_ptr(), 4, *SHAPE, 1.0, 0.0, m, stride, lo, scale, lo, scale, bins,
                                               hist.data_ptr() + 4 * bins * bins * k, stream())
                assert rc == 0, lib.mud_last_error()
        return launch, hist

    def sums_of(hist):
        h = hist.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, bins, bins)
        i = np.arange(bins, dtype=np.int64)
        ra, rb = h.sum(2), h.sum(1)
        return np.stack([h.sum((1, 2)), (ra * i).sum(1), (rb * i).sum(1), (ra * i * i).sum(1), (rb * i * i).sum(1), (h * np.outer(i, i)).sum((1, 2))], 1)

    for name, cand, stride in (('level0', level0, coarse), ('refine_coarse', near, coarse), ('refine_fine', near, fine)):
        new, sums = batched(cand, stride)
        old, hist = one_by_one(cand, stride)
        t_new, t_old = [], []
        for rep in range(args.launches):                  # alternating, each with its own warm-up launch the first time round
            t_new += timed(new, 1, warm=2 if rep == 0 else 0)
            t_old += timed(old, 1, warm=1 if rep == 0 else 0)
        same = bool(np.array_equal(sums.cpu().numpy(), sums_of(hist)))
        points = VA.sample_points(SHAPE, stride)
        out[name] = dict(candidates=len(cand), stride=stride, sample_points=points, one_launch=spread(t_new), k_joint_hist_launches=spread(t_old),
                         ratio_of_medians=float(np.median(t_old) / np.median(t_new)), same_sums=same,
                         pairs_per_s=float(sums.cpu().numpy()[:, 0].sum() / (np.median(t_new) * 1e-3)))
        print(f"{name}: K {len(cand)} stride {stride}: one launch median {np.median(t_new):.3f} ms (min {min(t_new):.3f}, max {max(t_new):.3f}); "
              f"K joint_hist launches median {np.median(t_old):.3f} ms (min {min(t_old):.3f}, max {max(t_old):.3f}); same sums {same}", flush=True)
    walls, rep = [], None
    kw = {k: v for k, v in d.items() if k != 'bins'}
    for _ in range(args.searches + 1):                    # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, rep = VA.estimate(raw, dev, bins=bins, **kw)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    out['search'] = dict(wall_s_median=float(np.median(walls[1:])), wall_s_min=float(min(walls[1:])), wall_s_max=float(max(walls[1:])), repetitions=args.searches,
                         candidates=rep['candidates'], levels=rep['levels'], found=[rep['yaw_deg'], rep['roll_deg'], rep['offset_mm']],
                         planted=list(pose), r=rep['r'], r_identity=rep['r_identity'], kept=rep['kept'])
    print(f"estimate: median {np.median(walls[1:]):.3f} s (min {min(walls[1:]):.3f}, max {max(walls[1:]):.3f}), {rep['candidates']} candidates in {rep['levels']} levels, "
          f"found {out['search']['found']} for {pose}, r {rep['r']:.4f} (identity {rep['r_identity']:.4f})", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
