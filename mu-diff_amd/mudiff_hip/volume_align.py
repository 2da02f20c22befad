"""The mid-sagittal plane of the inputs on the centre column of the grid (--align; csrc/volume_align.hip: mud_volume_mirror_moments;
DESIGN.md section 5.22).

The checkpoints were trained on heads registered to an atlas: upright, facing forward, the mid-sagittal plane on the centre column.
--conform places its grid in the first input's world, axis-aligned to the scanner, so a head that is turned, tilted or off-centre left
to right reaches the generators with an asymmetry no training slice had.  No atlas is shipped; what needs none is the head's own
bilateral symmetry: the mid-sagittal plane is the plane about which the volume best matches its mirror image.  It fixes yaw, roll and
the lateral offset - three of the six pose parameters.  Pitch and the two in-plane translations need a template and are NOT estimated.

    stored voxels of the first input --upload--> mud_volume_mirror_moments(K candidate planes, stride) --[K, 6] integer sums--> r on the host
    search(): a full grid over (yaw, roll, offset), then 3 x 3 x 3 neighbourhoods at halved steps; every level is one launch
    --> T (world -> world) --> the conform grid's affine becomes T @ conform_affine; every input still goes through ONE regrid_to

Definitions (numpy only, fp64), all in world coordinates, where x is NIfTI's left-right axis whatever the storage order:

    n = Rz(yaw) . Ry(roll) . e_x                       the plane's normal
    c                                                  the world position of the first input's grid centre
    n . (p - c) = t                                    the plane
    H = [I - 2 n n^T | 2 (n . c + t) n]                the mirror through it; a candidate's matrix is inv(A) @ H @ A
    T p = c + R (p - c) + t n,  R = Rz . Ry            the pose transform: it maps the plane x = c_x onto the plane

The score of a candidate is the Pearson correlation of the bin indices of the voxels and of their mirror images over the overlap,
r = (n Sab - Sa Sb) / sqrt((n Saa - Sa^2)(n Sbb - Sb^2)), from the kernel's six integer sums; -inf when fewer than min_overlap of the
sample points are counted (a plane that mirrors most of the head out of the field of view is not a candidate: a condition, not a tuned
value) or when a variance is not positive.  The defaults of the schedule are untuned.
"""
from __future__ import annotations

import numpy as np

from .volume_intake import write_report_json

PARAM_NAMES = ('yaw_deg', 'roll_deg', 'offset_mm')
MAX_BINS = 256
# untuned defaults, in the spirit of the prototype on a small phantom (20 deg / 12 mm, steps 5 deg / 4 mm halved to ~0.3 deg / 0.25 mm)
DEFAULTS = dict(max_deg=20.0, max_mm=12.0, step_deg=5.0, step_mm=4.0, final_deg=0.35, final_mm=0.25, strides=(4, 2), bins=32, min_overlap=0.5)
FINE_AT_DEG = 1.0                                        # the fine stride takes over once the angle step is this small


# ---------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------
def rotation(yaw_deg, roll_deg):
    """R = Rz(yaw) . Ry(roll), 3 x 3."""
    (cz, cy), (sz, sy) = np.cos(np.deg2rad([yaw_deg, roll_deg])), np.sin(np.deg2rad([yaw_deg, roll_deg]))
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    return rz @ ry


def normal(yaw_deg, roll_deg):
    """n = Rz(yaw) . Ry(roll) . e_x."""
    return rotation(yaw_deg, roll_deg)[:, 0].copy()


def mirror_world(params, centre):
    """(yaw, roll [deg], t [mm]) -> the 4 x 4 world matrix H of the mirror through the plane n . (p - c) = t."""
    yaw, roll, t = (float(v) for v in params)
    n, c = normal(yaw, roll), np.asarray(centre, np.float64).reshape(3)
    H = np.eye(4)
    H[:3, :3] -= 2.0 * np.outer(n, n)
    H[:3, 3] = 2.0 * (n @ c + t) * n
    return H


def pose_world(params, centre):
    """(yaw, roll [deg], t [mm]) -> the 4 x 4 world matrix T: T p = c + R (p - c) + t n."""
    yaw, roll, t = (float(v) for v in params)
    R, c = rotation(yaw, roll), np.asarray(centre, np.float64).reshape(3)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = c - R @ c + t * R[:, 0]
    return T


def mirror_matrices(candidates, affine, centre):
    """[K, 3] candidates -> [K, 3, 4] fp64: inv(A) @ H_k @ A, a voxel index of the volume -> the voxel coordinate of its mirror image."""
    A = np.asarray(affine, np.float64)
    Ai = np.linalg.inv(A)
    return np.stack([(Ai @ mirror_world(p, centre) @ A)[:3] for p in np.asarray(candidates, np.float64).reshape(-1, 3)])


def sample_points(shape, stride):
    """The number of sample points of a volume at a stride: every stride-th voxel per axis."""
    return int(np.prod([-(-int(s) // int(stride)) for s in shape]))


def scores(sums, points, min_overlap=DEFAULTS['min_overlap']):
    """[K, 6] integer sums (n, Sa, Sb, Saa, Sbb, Sab) -> [K] fp64 Pearson r; -inf where n < min_overlap * points or a variance is <= 0."""
    s = np.asarray(sums).astype(np.float64).reshape(-1, 6)
    n, sa, sb, saa, sbb, sab = s.T
    va, vb = n * saa - sa * sa, n * sbb - sb * sb
    ok = (n >= float(min_overlap) * float(points)) & (va > 0) & (vb > 0)
    r = np.full(n.shape, -np.inf)
    r[ok] = (n[ok] * sab[ok] - sa[ok] * sb[ok]) / np.sqrt(va[ok] * vb[ok])
    return r


# ---------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------
def _axis(limit, step):
    k = int(np.floor(limit / step + 1e-9))
    return np.arange(-k, k + 1, dtype=np.float64) * step


def schedule(step_deg, step_mm, final_deg, final_mm, strides):
    """[(angle step, offset step, stride)] per level: level 0 at the first steps, then both halved until neither is above its final step;
    the coarse stride until the angle step reaches FINE_AT_DEG, the fine one from there."""
    coarse, fine = int(strides[0]), int(strides[-1])
    levels, d, m = [], float(step_deg), float(step_mm)
    while True:
        levels.append((d, m, fine if d <= FINE_AT_DEG else coarse))
        if d <= final_deg and m <= final_mm:
            return levels
        d, m = d / 2.0, m / 2.0


def search(cost, points, max_deg=DEFAULTS['max_deg'], max_mm=DEFAULTS['max_mm'], step_deg=DEFAULTS['step_deg'], step_mm=DEFAULTS['step_mm'],
           final_deg=DEFAULTS['final_deg'], final_mm=DEFAULTS['final_mm'], strides=DEFAULTS['strides'], min_overlap=DEFAULTS['min_overlap']):
    """The deterministic, batched search.  cost(candidates [K, 3], stride) -> [K, 6] integer sums (the device's, or a host restatement:
    one call per level); points(stride) -> the number of sample points.  Level 0 is the full grid of multiples of the first steps within
    +-max_deg, +-max_deg, +-max_mm; every later level is the 3 x 3 x 3 neighbourhood of the best candidate at halved steps, clipped to the
    range, the best candidate itself first, so that a tie stays put (np.argmax takes the first).
    -> dict(params (None when every candidate of level 0 scored -inf), r, steps (the final ones), candidates, levels, boundary)."""
    levels = schedule(step_deg, step_mm, final_deg, final_mm, strides)
    limit = np.array([max_deg, max_deg, max_mm], np.float64)
    best, r_best, total = None, -np.inf, 0
    for level, (d, m, stride) in enumerate(levels):
        if level == 0:
            g = np.meshgrid(_axis(max_deg, d), _axis(max_deg, d), _axis(max_mm, m), indexing='ij')
            cand = np.stack([v.reshape(-1) for v in g], 1)
            cand = cand[np.argsort(np.abs(cand / np.array([d, d, m])).sum(1), kind='stable')]      # the identity first: ties stay there
        else:
            off = np.array([(i, j, k) for i in (0, -1, 1) for j in (0, -1, 1) for k in (0, -1, 1)], np.float64) * np.array([d, d, m])
            cand = np.clip(best + off, -limit, limit)
        r = scores(cost(cand, stride), points(stride), min_overlap)
        total += len(cand)
        k = int(np.argmax(r))
        if not np.isfinite(r[k]):
            if level == 0:
                return dict(params=None, r=-np.inf, steps=[d, d, m], candidates=total, levels=1, boundary=False)
            continue                                     # (the stride changed under the best candidate: it stays)
        best, r_best = cand[k].copy(), float(r[k])
    d, m, _ = levels[-1]
    boundary = bool((np.abs(best) >= limit - 1e-9).any())
    return dict(params=[float(v) for v in best], r=r_best, steps=[d, d, m], candidates=total, levels=len(levels), boundary=boundary)


def finish(cost, points, centre, **kw):
    """search() and the fallback around a cost function (estimate's device one, or a host restatement) -> (T, report).  T is the
    identity - the input is left unaligned, `kept` is 0 and a warning line is printed - when the best candidate lies on the boundary of
    the search range in any parameter or when every candidate scored -inf.  There is no threshold on r."""
    fine = int(kw.get('strides', DEFAULTS['strides'])[-1])
    min_overlap = kw.get('min_overlap', DEFAULTS['min_overlap'])
    found = search(cost, points, **kw)
    here = [[0.0, 0.0, 0.0]] + ([found['params']] if found['params'] is not None else [])
    sums = np.asarray(cost(np.array(here, np.float64), fine)).reshape(-1, 6)
    r = scores(sums, points(fine), min_overlap)
    kept = found['params'] is not None and not found['boundary']
    params = found['params'] if found['params'] is not None else [0.0, 0.0, 0.0]
    if not kept:
        why = 'no candidate plane keeps enough of the volume in view' if found['params'] is None else \
            'the best plane lies on the boundary of the search range (%s)' % ', '.join(f'{v:g}' for v in params)
        print(f'[align] warning: {why}; the input is left unaligned')
    T = pose_world(params, centre) if kept else np.eye(4)
    report = dict(yaw_deg=params[0], roll_deg=params[1], offset_mm=params[2], r=float(r[-1]) if found['params'] is not None else None,
                  r_identity=float(r[0]) if np.isfinite(r[0]) else None, overlap=float(sums[-1, 0]) / float(points(fine)),
                  candidates=int(found['candidates']) + len(here), levels=int(found['levels']), steps=found['steps'], kept=int(kept),
                  T=np.asarray(T).tolist())
    return T, report


def mirror_moments(dev, meta, mats, stride, lo, scale, bins):
    """mud_volume_mirror_moments -> host int64 [K, 6] (one launch, one small copy).  dev: the flat device array of the stored voxels;
    meta: RawVolume.kernel_meta's (datatype code, shape, slope, inter); mats: [K, 3, 4] fp64 on the host."""
    from . import ops
    code, shape, slope, inter = meta
    return ops.volume_mirror_moments(dev, code, shape, slope, inter, mats, stride, lo, scale, bins).cpu().numpy()


def estimate(raw, device, bins=DEFAULTS['bins'], **kw):
    """The mid-sagittal plane of a RawVolume (its voxels on the host, or on the device already) -> (T, report).  T: the 4 x 4 world
    matrix of the pose (pose_world), the identity when the fallback struck; report: yaw_deg, roll_deg, offset_mm, r (at the plane found),
    r_identity, overlap (the share of the sample points counted at the plane found), candidates, levels, steps, kept, T."""
    from .volume_coreg import grid_centre, value_range
    from .volume_intake import upload
    from .volume_regrid import world_affine_of
    if len(raw.shape) != 3:
        raise ValueError(f'align: expected a 3D volume, got shape {tuple(raw.shape)}')
    A = world_affine_of(raw.affine, raw.header)
    centre = grid_centre(raw.shape, A)
    lo, hi = value_range(raw)
    scale = float(bins) / (hi - lo) if hi > lo else 0.0
    scale = scale if np.isfinite(scale) else 0.0
    meta, dev = raw.kernel_meta('align'), upload(raw, device)

    def cost(candidates, stride):
        return mirror_moments(dev, meta, mirror_matrices(candidates, A, centre), stride, lo, scale, bins)

    T, report = finish(cost, lambda stride: sample_points(raw.shape, stride), centre, **kw)
    report['bins'] = int(bins)
    return T, report


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p = getattr(p, 'late', p)                            # volume.VolumeParser: the main option list is pinned, later stages go here
    p.add_argument('--align', action='store_true',
                   help='with --conform: turn the conform grid so that the mid-sagittal plane of the first input lies on its centre column '
                        '(mudiff_hip.volume_align).  The plane is the one about which the first input best matches its own mirror image '
                        '(correlation of binned intensities, scored for many candidate planes per launch on the GPU); it fixes yaw, roll and '
                        'the left-right offset.  Pitch and the in-plane position need a template and are not estimated.  Every input is still '
                        'resampled once, onto the turned grid; the prediction is written with the oblique affine; align_<t>.json next to it '
                        'holds what was found.  A plane on the boundary of the search range leaves the input unaligned, with a warning.  '
                        'Every default below is untuned')
    d = DEFAULTS
    p.add_argument('--align_max_deg', type=float, default=d['max_deg'], help='largest yaw and roll the search may propose')
    p.add_argument('--align_max_mm', type=float, default=d['max_mm'], help='largest left-right offset the search may propose')
    p.add_argument('--align_step_deg', type=float, default=d['step_deg'], help='the angle step of the first level, a full grid; halved per level')
    p.add_argument('--align_step_mm', type=float, default=d['step_mm'], help='the offset step of the first level; halved per level')
    p.add_argument('--align_final_deg', type=float, default=d['final_deg'], help='the search stops once the angle step is no larger than this ...')
    p.add_argument('--align_final_mm', type=float, default=d['final_mm'], help='... and the offset step no larger than this')
    p.add_argument('--align_strides', nargs=2, type=int, default=list(d['strides']), metavar=('COARSE', 'FINE'),
                   help='sampling strides: the coarse one until the angle step reaches 1 degree, the fine one from there')
    p.add_argument('--align_bins', type=int, default=d['bins'], help=f'intensity bins of the correlation (2 to {MAX_BINS})')
    p.add_argument('--align_min_overlap', type=float, default=d['min_overlap'],
                   help='a candidate plane must keep at least this share of the sample points inside the volume after mirroring')


def options_from(args):
    """A namespace's --align flags (any may be missing) -> IntakeOptions' `align`: the keyword arguments of estimate, or None without
    --align.  ValueError, naming the flag, for values the search cannot run with, and for --align without --conform."""
    get = lambda name: DEFAULTS[name] if getattr(args, 'align_' + name, None) is None else getattr(args, 'align_' + name)      # noqa: E731
    kw = {k: float(get(k)) for k in ('max_deg', 'max_mm', 'step_deg', 'step_mm', 'final_deg', 'final_mm', 'min_overlap')}
    kw.update(strides=tuple(int(s) for s in get('strides')), bins=int(get('bins')))
    for k in ('max_deg', 'max_mm', 'step_deg', 'step_mm', 'final_deg', 'final_mm'):
        if not (np.isfinite(kw[k]) and kw[k] > 0):
            raise ValueError(f'--align_{k} must be positive and finite, got {kw[k]}')
    if kw['max_deg'] >= 90.0:
        raise ValueError(f'--align_max_deg must be below 90, got {kw["max_deg"]}')
    for k, limit in (('step_deg', 'max_deg'), ('step_mm', 'max_mm')):
        if kw[k] > kw[limit]:
            raise ValueError(f'--align_{k} must not exceed --align_{limit}, got {kw[k]} > {kw[limit]}')
    if len(kw['strides']) != 2 or min(kw['strides']) < 1 or kw['strides'][1] > kw['strides'][0]:
        raise ValueError(f'--align_strides takes two positive strides, coarse then fine, got {kw["strides"]}')
    if not 2 <= kw['bins'] <= MAX_BINS:
        raise ValueError(f'--align_bins: 2 to {MAX_BINS} bins, got {kw["bins"]}')
    if not 0.0 < kw['min_overlap'] <= 1.0:
        raise ValueError(f'--align_min_overlap must lie in (0, 1], got {kw["min_overlap"]}')
    on = bool(getattr(args, 'align', False))
    if on and not getattr(args, 'conform', False):
        raise ValueError('--align needs --conform: without it the first input is never resampled')
    return dict(align=kw if on else None)


def align_suffix(reports):
    """What a [done] line gains under --align (nothing otherwise): ` | align=<name>:<yaw>/<roll>deg/<offset>mm`, or `<name>:kept=0`."""
    if not reports:
        return ''
    return ' | align=' + ','.join(f"{name}:{rep['yaw_deg']:.2f}/{rep['roll_deg']:.2f}deg/{rep['offset_mm']:.2f}mm" if rep['kept'] else f'{name}:kept=0'
                                  for name, rep in reports)


def write_reports(reports, output_dir, target):
    """align_<t>.json next to the prediction: {input name: report}.  -> its path."""
    return write_report_json('align', {name: rep for name, rep in reports}, output_dir, target)
