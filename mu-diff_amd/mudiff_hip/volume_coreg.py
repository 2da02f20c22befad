"""Rigid co-registration of the inputs (--coregister; csrc/volume_coreg.hip: mud_volume_joint_hist).

--regrid resamples between grids whose world coordinates already agree.  A patient who moved between two acquisitions breaks that
premise by a few millimetres and degrees that no header records.  With --coregister every input other than the first is aligned to
the first one rigidly (three translations, three rotations) before it is resampled onto the first input's grid:

    stored voxels of both volumes --upload--> mud_volume_joint_hist(M(params), stride) --[bins, bins] counts--> nmi() on the host
    powell() over the six parameters, coarse to fine in the sampling stride --> W --> volume_regrid.regrid_to(..., world=W)

The measure is normalised mutual information (H(F) + H(M)) / H(F, M) of the joint histogram over the overlap of the two volumes.  The
histogram is the device's work (one launch and a copy of bins^2 counts per evaluation); the search is numpy on the host.  W is a world
-> world matrix: the sampling matrix of a candidate is inv(A_moving) @ W @ A_fixed, which for W = I is volume_regrid.grid_matrix.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np
import torch

from . import MudiffHipError, load, ptr, require_gpu
from .volume_intake import DEVICE_DTYPES, upload, write_report_json
from .volume_regrid import _affine44, grid_matrix, world_affine_of

PARAM_NAMES = ('tx_mm', 'ty_mm', 'tz_mm', 'rx_deg', 'ry_deg', 'rz_deg')
MAX_BINS = 64
DEFAULTS = dict(strides=(4, 2, 1), max_mm=20.0, max_deg=15.0)


# ---------------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------------
def joint_hist(fix_dev, fix_raw_meta, mov_dev, mov_raw_meta, M, stride, ranges, bins):
    """mud_volume_joint_hist -> host int64 [bins, bins] (one launch, one small copy).  *_dev: the flat device arrays of the stored voxels;
    *_raw_meta: (datatype code, shape [X,Y,Z], slope, inter) with slope / inter 1 / 0 for an unscaled file; M: fixed voxel index ->
    moving voxel coordinate (4 x 4 or 3 x 4); ranges: (fix_lo, fix_scale, mov_lo, mov_scale) of bin = floor((v - lo) * scale)."""
    require_gpu(fix_dev, mov_dev)
    sides = []
    for dev, (code, shape, slope, inter) in ((fix_dev, fix_raw_meta), (mov_dev, mov_raw_meta)):
        if int(code) not in DEVICE_DTYPES:
            raise MudiffHipError(f'joint_hist: unsupported NIfTI datatype code {code}')
        X, Y, Z = (int(v) for v in shape)
        if dev.numel() != X * Y * Z or dev.element_size() != np.dtype(DEVICE_DTYPES[int(code)]).itemsize or not dev.is_contiguous():
            raise MudiffHipError(f'joint_hist: {dev.numel()} voxels of {dev.element_size()} bytes do not hold a {X} x {Y} x {Z} volume of '
                                 f'datatype {code}')
        sides.append((ptr(dev), int(code), X, Y, Z, float(slope), float(inter)))
    m = np.ascontiguousarray(np.asarray(M, np.float64)[:3, :4])
    if m.shape != (3, 4):
        raise ValueError(f'joint_hist: need a 3 x 4 or 4 x 4 matrix, got {np.shape(M)}')
    bins = int(bins)
    hist = torch.empty(max(bins, 1) * max(bins, 1), device=fix_dev.device, dtype=torch.int32)
    from . import ops
    ops._launch('volume_joint_hist', fix_dev.device, load().mud_volume_joint_hist, *sides[0], *sides[1], (C.c_double * 12)(*m.reshape(-1).tolist()),
                int(stride), *(float(v) for v in ranges), bins, ptr(hist), ops.STREAM,
                nbytes=float(fix_dev.numel() * fix_dev.element_size() + mov_dev.numel() * mov_dev.element_size()) / max(int(stride), 1) ** 3)
    return hist.cpu().numpy().view(np.uint32).astype(np.int64).reshape(bins, bins)


def nmi(hist):
    """(H(F) + H(M)) / H(F, M) of a joint histogram in fp64; 0 for an empty one (and for one whose joint entropy is 0: a single bin)."""
    h = np.asarray(hist, np.float64)
    n = h.sum()
    if not n > 0:
        return 0.0

    def entropy(c):
        p = c[c > 0] / n
        return float(-(p * np.log(p)).sum())

    joint = entropy(h.reshape(-1))
    return (entropy(h.sum(1)) + entropy(h.sum(0))) / joint if joint > 0 else 0.0


def value_range(raw):
    """(lo, hi) of the finite fp32 values the pipeline sees of a RawVolume, as python floats; (0, 0) when it has none."""
    a = np.asarray(raw.data)
    if a.dtype.kind == 'f':
        a = a[np.isfinite(a)]
    if a.size == 0:
        return 0.0, 0.0
    ends = np.array([a.min(), a.max()]).astype(np.float64)
    if raw.scaled:
        ends = ends * raw.slope + raw.inter
    ends = ends.astype(np.float32).astype(np.float64)
    ends = ends[np.isfinite(ends)]
    return (float(ends.min()), float(ends.max())) if ends.size else (0.0, 0.0)


def bin_ranges(fixed_raw, moving_raw, bins):
    """(fix_lo, fix_scale, mov_lo, mov_scale): `bins` equal bins between each volume's finite minimum and maximum (the maximum itself
    is clamped into the last bin); scale 0 - one bin - for a flat volume."""
    out = []
    for raw in (fixed_raw, moving_raw):
        lo, hi = value_range(raw)
        scale = float(bins) / (hi - lo) if hi > lo else 0.0
        out += [lo, scale if np.isfinite(scale) else 0.0]
    return tuple(out)


# ---------------------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------------------
def rigid_world(params, centre):
    """(tx, ty, tz [mm], rx, ry, rz [deg]) -> the 4 x 4 world matrix W: the rotation Rz . Ry . Rx about `centre`, then the translation."""
    p = np.asarray(params, np.float64).reshape(6)
    c = np.asarray(centre, np.float64).reshape(3)
    (cx, cy, cz), (sx, sy, sz) = np.cos(np.deg2rad(p[3:])), np.sin(np.deg2rad(p[3:]))
    rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    W = np.eye(4)
    W[:3, :3] = rz @ ry @ rx
    W[:3, 3] = (c + p[:3]) - W[:3, :3] @ c
    return W


def grid_centre(shape, affine):
    """The world position of a grid's centre voxel coordinate (shape - 1) / 2."""
    a = _affine44(affine, 'affine')
    return a[:3, :3] @ ((np.asarray(shape, np.float64) - 1.0) / 2.0) + a[:3, 3]


def is_identity(W):
    return W is None or bool(np.array_equal(np.asarray(W, np.float64), np.eye(4)))


def sampling_matrix(mov_affine, W, fix_affine):
    """inv(A_mov) @ W @ A_fix: fixed voxel index -> moving voxel coordinate.  W = I gives grid_matrix(A_mov, A_fix) exactly."""
    fix = _affine44(fix_affine, 'fixed affine')
    return grid_matrix(mov_affine, fix if is_identity(W) else _affine44(W, 'world transform') @ fix)


# ---------------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------------
_GOLD = 0.3819660112501051


def _line_max(f, f0, step, xtol, max_eval=60):
    """Maximise f(t) from t = 0 (f(0) = f0): bracket by doubling steps, then Brent's parabolic / golden-section search to |dt| <= xtol.
    -> (t, f(t), evaluations); t = 0 when nothing better is found."""
    g = lambda t: -f(t)                      # noqa: E731  (minimise -f)
    n = 0
    a, fa, b = 0.0, -f0, float(step)
    fb = g(b)
    n += 1
    if fb >= fa:                             # go downhill: swap so that a -> b descends (a flat step, at the box's wall: look the other way)
        a, b, fa, fb = b, a, fb, fa
    c = b + 1.618033988749895 * (b - a)
    fc = g(c)
    n += 1
    while fc < fb and n < max_eval:
        a, fa, b, fb = b, fb, c, fc
        c = b + 1.618033988749895 * (b - a)
        fc = g(c)
        n += 1
    lo, hi = min(a, c), max(a, c)
    x = w = v = b
    fx = fw = fv = fb
    d = e = 0.0
    while n < max_eval:
        mid = 0.5 * (lo + hi)
        tol1 = xtol
        if abs(x - mid) <= 2.0 * tol1 - 0.5 * (hi - lo):
            break
        use_golden = True
        if abs(e) > tol1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0:
                p = -p
            q = abs(q)
            if abs(p) < abs(0.5 * q * e) and q * (lo - x) < p < q * (hi - x):
                e, d = d, p / q
                u = x + d
                if u - lo < 2.0 * tol1 or hi - u < 2.0 * tol1:
                    d = tol1 if mid >= x else -tol1
                use_golden = False
        if use_golden:
            e = (hi if x < mid else lo) - x
            d = _GOLD * e
        u = x + d if abs(d) >= tol1 else x + (tol1 if d > 0 else -tol1)
        fu = g(u)
        n += 1
        if fu < fx:                          # (strictly: a tie - the flat stretch beyond the box's wall - must not move the best point)
            if u >= x:
                lo = x
            else:
                hi = x
            v, fv, w, fw, x, fx = w, fw, x, fx, u, fu
        else:
            if u < x:
                lo = u
            else:
                hi = u
            if fu <= fw or w == x:
                v, fv, w, fw = w, fw, u, fu
            elif fu <= fv or v == x or v == w:
                v, fv = u, fu
    if fx < -f0:
        return x, -fx, n
    return 0.0, f0, n


def powell(cost, x0, step=1.0, xtol=1e-3, ftol=1e-9, max_iter=30, lower=None, upper=None):
    """Maximise cost(x) by Powell's direction-set method: line searches (bracketing + Brent) along a set of directions that starts as
    the axes; after each sweep the direction of the largest gain is replaced by the sweep's net displacement when that promises more.
    Deterministic, numpy only.  `step`: first bracketing step (scalar or per parameter); `xtol`: line-search resolution; `ftol`: a sweep
    that gains less (relatively) ends the search; lower / upper: a box the candidates are clamped to.  -> (x, cost(x), evaluations)."""
    x = np.asarray(x0, np.float64).copy()
    n = x.size
    lower = np.full(n, -np.inf) if lower is None else np.broadcast_to(np.asarray(lower, np.float64), (n,))
    upper = np.full(n, np.inf) if upper is None else np.broadcast_to(np.asarray(upper, np.float64), (n,))
    clamp = lambda v: np.minimum(np.maximum(v, lower), upper)      # noqa: E731
    evals = [0]

    def f(v):
        evals[0] += 1
        return float(cost(clamp(v)))

    x = clamp(x)
    fx = f(x)
    dirs = np.eye(n) * np.broadcast_to(np.asarray(step, np.float64), (n,))[:, None]

    def along(x, fx, d):
        t, ft, _ = _line_max(lambda t: f(x + t * d), fx, 1.0, xtol / max(float(np.abs(d).max()), 1e-300))
        return (clamp(x + t * d), ft) if t != 0.0 else (x, fx)

    for _ in range(int(max_iter)):
        x_start, f_start = x.copy(), fx
        biggest, ibig = 0.0, 0
        for i in range(n):
            x_new, f_new = along(x, fx, dirs[i])
            if f_new - fx > biggest:
                biggest, ibig = f_new - fx, i
            x, fx = x_new, f_new
        if 2.0 * (fx - f_start) <= ftol * (abs(fx) + abs(f_start)) + 1e-300:
            break
        d_new = x - x_start
        if not d_new.any():
            break
        fe = f(x + d_new)
        if fe > f_start:                     # (Numerical Recipes' test with the signs of a maximiser)
            a, b, c = -f_start, -fx, -fe
            if 2.0 * (a - 2.0 * b + c) * (a - b - biggest) ** 2 - biggest * (a - c) ** 2 < 0.0:
                x, fx = along(x, fx, d_new)
                dirs[ibig] = dirs[n - 1]
                dirs[n - 1] = d_new
    return x, fx, evals[0]


def search(cost_at, strides=(4, 2, 1), max_mm=20.0, max_deg=15.0, x0=None):
    """The coarse-to-fine search: cost_at(params, stride) -> NMI.  One powell() per stride, each from the previous result, the first
    bracketing step and the resolution shrinking with the stride; parameters clamped to +-max_mm / +-max_deg.
    -> (params, [evaluations per level])."""
    x = np.zeros(6) if x0 is None else np.asarray(x0, np.float64).copy()
    box = np.array([max_mm] * 3 + [max_deg] * 3, np.float64)
    evals = []
    for s in strides:
        s = int(s)
        x, _, n = powell(lambda p: cost_at(p, s), x, step=float(s), xtol=0.01 * s, ftol=1e-7, max_iter=8, lower=-box, upper=box)
        evals.append(int(n))
    return x, evals


def coregister(fixed_raw, moving_raw, device, strides=(4, 2, 1), bins=32, max_mm=20.0, max_deg=15.0):
    """Rigidly align `moving_raw` to `fixed_raw` (RawVolumes) -> (W, report).  W: 4 x 4 world matrix for volume_regrid.regrid_to's
    `world`; the identity - with a warning, and accepted False in the report - when the search did not improve NMI at stride 1 over
    the identity (the volume then takes the path it takes without --coregister).  report: params (the six numbers, PARAM_NAMES order),
    nmi_identity, nmi_result (both at stride 1), evaluations (per level), strides, bins, accepted, W."""
    for raw in (fixed_raw, moving_raw):
        if len(raw.shape) != 3:
            raise ValueError(f'coregister: expected 3D volumes, got shape {tuple(raw.shape)}')
    bins = int(bins)
    if not 2 <= bins <= MAX_BINS:
        raise ValueError(f'coregister: 2 to {MAX_BINS} bins, got {bins}')
    strides = tuple(int(s) for s in strides)
    if not strides or min(strides) < 1:
        raise ValueError(f'coregister: strides must be positive, got {strides}')
    a_fix, a_mov = world_affine_of(fixed_raw.affine, fixed_raw.header), world_affine_of(moving_raw.affine, moving_raw.header)
    centre = grid_centre(fixed_raw.shape, a_fix)
    ranges = bin_ranges(fixed_raw, moving_raw, bins)
    metas = [r.kernel_meta('joint_hist') for r in (fixed_raw, moving_raw)]
    fix_dev, mov_dev = upload(fixed_raw, device), upload(moving_raw, device)

    def cost_at(params, stride):
        M = sampling_matrix(a_mov, rigid_world(params, centre), a_fix)
        return nmi(joint_hist(fix_dev, metas[0], mov_dev, metas[1], M, stride, ranges, bins))

    return finish(cost_at, centre, strides, bins, max_mm, max_deg)


def finish(cost_at, centre, strides, bins, max_mm, max_deg):
    """search() and the acceptance rule around a cost function (coregister's device one, or a host restatement) -> (W, report)."""
    nmi0 = float(cost_at(np.zeros(6), 1))
    params, evals = search(cost_at, strides, max_mm, max_deg)
    nmi1 = float(cost_at(params, 1))
    accepted = bool(nmi1 > nmi0)
    W = rigid_world(params, centre) if accepted else np.eye(4)
    if not accepted:
        warnings.warn(f'coregister: NMI did not improve over the identity ({nmi1:.6f} vs {nmi0:.6f}); the volume is left where its header '
                      'puts it', RuntimeWarning, stacklevel=3)
    report = dict(params=[float(v) for v in params], param_names=list(PARAM_NAMES), nmi_identity=nmi0, nmi_result=nmi1,
                  evaluations=evals, strides=[int(s) for s in strides], bins=int(bins), accepted=accepted, W=np.asarray(W).tolist())
    return W, report


# ---------------------------------------------------------------------------------------------------
# the pipeline's side
# ---------------------------------------------------------------------------------------------------
def add_flags(p):
    p.add_argument('--coregister', action='store_true',
                   help='rigidly align every input other than the first to the first input (six parameters, normalised mutual '
                        'information, histogram on the GPU: mudiff_hip.volume_coreg), then resample it onto the first input\'s grid '
                        'as --regrid does; coreg_<t>.json next to the prediction holds what was found.  --gt_volume / --eval_mask are '
                        'not registered')
    p.add_argument('--coregister_strides', nargs='+', type=int, default=list(DEFAULTS['strides']),
                   help='sampling strides of the coarse-to-fine search levels')
    p.add_argument('--coregister_max_mm', type=float, default=DEFAULTS['max_mm'], help='largest translation per axis the search may propose')
    p.add_argument('--coregister_max_deg', type=float, default=DEFAULTS['max_deg'], help='largest rotation per axis the search may propose')


def options_from(args):
    """A namespace's --coregister flags (any may be missing) -> IntakeOptions' `coreg`: the keyword arguments of coregister, or None
    without --coregister.  ValueError, naming the flags, for values the search cannot run with."""
    get = lambda name: getattr(args, 'coregister_' + name, None)      # noqa: E731
    kw = dict(strides=tuple(int(s) for s in get('strides') or DEFAULTS['strides']),
              **{k: float(DEFAULTS[k] if get(k) is None else get(k)) for k in ('max_mm', 'max_deg')})
    if min(kw['strides']) < 1 or kw['max_mm'] < 0 or kw['max_deg'] < 0:
        raise ValueError('--coregister_strides must be positive, --coregister_max_mm / --coregister_max_deg not negative')
    return dict(coreg=kw if getattr(args, 'coregister', False) else None)


def coreg_suffix(reports):
    """What a [done] line gains under --coregister (nothing otherwise): ` | coreg=<name>:<mm>mm/<deg>deg,...`, the lengths of the
    translation and of the rotation vector of each registered input."""
    if not reports:
        return ''
    parts = []
    for name, rep in reports:
        p = np.asarray(rep['params'], np.float64) if rep['accepted'] else np.zeros(6)
        parts.append(f'{name}:{np.linalg.norm(p[:3]):.2f}mm/{np.linalg.norm(p[3:]):.2f}deg')
    return ' | coreg=' + ','.join(parts)


def write_reports(reports, output_dir, target):
    """coreg_<t>.json next to the prediction: {input name: report}.  -> its path."""
    return write_report_json('coreg', {name: rep for name, rep in reports}, output_dir, target)
